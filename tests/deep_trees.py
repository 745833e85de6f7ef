"""Meshes whose octrees are deeper or wider than any asset's, for tests/test_deep_trees_cpu.py and
tests/test_gpu_deep_trees.py, and helpers that read an exported tree (Octree.export(), or the
oracle's tree_arrays() put the same way). numpy only, fixed seeds, nothing is read from disk.

The traversal keeps levels 0-7 of its mask stack in one u64 and levels 8-14 in another; the
near-first pass of bounce rays and ray queries is taken only for trees of depth <= 8 with fewer than
2^16 inner nodes; an upload rejects a node at depth 16. NESTED and WIDE name the trees that sit on
each side of those limits; tests/test_deep_trees_cpu.py pins their depths and inner-node counts."""
import numpy as np

F = np.float32
FOCUS = (0.37, -0.21, -0.53)
# Sizes. The reference's triangle test drops a triangle whose determinant (twice its area, times the
# cosine to the ray) is below 1e-4, and a hit nearer than 1e-4. So that the innermost shell's
# triangles (about size * s0 / 2^15 across) and the grid's (scale * cell) can still be hit, the
# outermost shell is 2^14 wide and a grid cell 1.
S0 = 16384.0
CELL = 1.0

# name -> (nested() arguments, leaf size, depth of the tree). Depth = the deepest node's, root 0.
NESTED = {
    "d8": (dict(levels=8, per=60, seed=8), 8, 8),     # the fullest register stack of the near-first pass
    "d9": (dict(levels=9, per=60, seed=8), 8, 9),     # one level into the high half; falls back by depth
    "d15": (dict(levels=15, per=60, seed=8), 8, 15),  # the deepest tree an upload accepts
    "d16": (dict(levels=16, per=60, seed=8), 8, 16),  # rejected: ATR_E_TREE_DEPTH
}
# name -> (wide() arguments, leaf size): depth <= 8 on both, inner nodes on either side of 2^16
WIDE = {
    "wide": (dict(g=72, seed=1), 2),
    "twin": (dict(g=64, seed=1), 2),
}


def obj_text(tri):
    """OBJ text of (n, 3, 3) float32 triangles, three vertices of its own for each (%.9g: exact)."""
    tri = np.asarray(tri, F).reshape(-1, 9)
    n = len(tri)
    v = "\n".join(map("v %.9g %.9g %.9g\nv %.9g %.9g %.9g\nv %.9g %.9g %.9g".__mod__, map(tuple, tri.tolist())))
    i = np.arange(1, 3 * n + 1).reshape(n, 3)
    f = "\n".join(map("f %d %d %d".__mod__, map(tuple, i.tolist())))
    return v + "\n" + f + "\n"


def nested_triangles(levels, per, seed, s0=S0, ratio=0.5, size=0.25, focus=FOCUS):
    """Level k: `per` triangles with centres uniform in the cube of half-side h = s0 * ratio**k around
    the focus, corners within size * h of the centre. The build splits at the area-weighted centroid,
    which the outer shells keep near the focus: each build level peels off about one shell."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(levels):
        h = s0 * ratio ** k
        c = np.asarray(focus) + rng.uniform(-h, h, (per, 1, 3))
        out.append(c + rng.uniform(-1.0, 1.0, (per, 3, 3)) * (size * h))
    return np.concatenate(out).astype(F)


def nested(levels, per, seed, **kw):
    return obj_text(nested_triangles(levels, per, seed, **kw))


def wide_triangles(g, seed, scale=0.1, jitter=0.25, cell=CELL, focus=FOCUS):
    """A g x g x g grid of cells of side `cell` centred on the focus, one triangle in each: its centre
    the cell's centre moved by up to jitter * cell per axis, its corners within scale * cell of that.
    The triangles are disjoint (jitter + scale < 0.5)."""
    rng = np.random.default_rng(seed)
    ax = (np.arange(g) - (g - 1) / 2.0) * cell
    c = np.stack(np.meshgrid(ax, ax, ax, indexing="ij"), -1).reshape(-1, 1, 3) + np.asarray(focus)
    c = c + rng.uniform(-jitter, jitter, c.shape) * cell
    return (c + rng.uniform(-1.0, 1.0, (len(c), 3, 3)) * (scale * cell)).astype(F)


def wide(g, seed, **kw):
    return obj_text(wide_triangles(g, seed, **kw))


_texts = {}


def leaf_size(name):
    return NESTED[name][1] if name in NESTED else WIDE[name][1]


def text(name):
    """The OBJ text of a tree of NESTED or WIDE (formatted once per process: the wide ones take seconds)."""
    if name not in _texts:
        _texts[name] = nested(**NESTED[name][0]) if name in NESTED else wide(**WIDE[name][0])
    return _texts[name]


# ---- an exported tree: bounds (n, 6) f32, children (n,) i32 (0: a leaf; else the first of 8 children) ----

def node_depths(children):
    """The depth of each node, the root at 0."""
    children = np.asarray(children)
    depth = np.full(len(children), -1, np.int32)
    depth[0] = 0
    level = np.array([0])
    while len(level):
        c = children[level]
        inner = c != 0
        kids = (c[inner][:, None] + np.arange(8)[None, :]).ravel()
        depth[kids] = np.repeat(depth[level[inner]] + 1, 8)
        level = kids
    assert (depth >= 0).all()
    return depth


def deepest_inner(bounds, children):
    """(node, depth, box) of the deepest inner node (the first in node order among equals)."""
    depth = node_depths(children)
    d = np.where(np.asarray(children) != 0, depth, -1)
    i = int(np.argmax(d))
    assert d[i] >= 0, "the root is a leaf"
    return i, int(d[i]), np.array(bounds[i], F)


def centre(box):
    box = np.asarray(box, np.float64)
    return tuple(float(x) for x in (box[:3] + box[3:]) * 0.5)


def deep_leaves(children, count, min_depth, limit=64):
    """The leaves that hold triangles at depth min_depth or more: at most `limit` of them, evenly
    strided in node order."""
    depth = node_depths(children)
    idx = np.flatnonzero((np.asarray(children) == 0) & (np.asarray(count) > 0) & (depth >= min_depth))
    assert len(idx), min_depth
    if len(idx) > limit:
        idx = idx[np.linspace(0, len(idx) - 1, limit).astype(np.int64)]
    return idx


def leaf_boxes(bounds, children, count, min_depth, limit=64):
    """The boxes of deep_leaves()."""
    return [np.array(bounds[i], F) for i in deep_leaves(children, count, min_depth, limit)]


def leaf_triangle_boxes(children, first, count, verts, min_depth, limit=64):
    """The bounding box of the first triangle of each of deep_leaves(): a target for rays that are to
    hit inside a deep leaf, where its triangles fill little of the leaf's box."""
    out = []
    for i in deep_leaves(children, count, min_depth, limit):
        v = np.asarray(verts[first[i]], F).reshape(3, 3)
        out.append(np.concatenate([v.min(axis=0), v.max(axis=0)]).astype(F))
    return out


def inner_depth_at(bounds, children, points):
    """For each point, the depth of the deepest inner node whose (closed) box holds it; -1 outside the
    root's box or where the root is a leaf."""
    bounds, children = np.asarray(bounds, F), np.asarray(children)
    p = np.asarray(points, F).reshape(-1, 3)

    def holds(node):
        b = bounds[node]
        return ((p >= b[:, :3]) & (p <= b[:, 3:])).all(axis=1)

    cur = np.zeros(len(p), np.int64)
    out = np.where(holds(cur) & (children[0] != 0), 0, -1).astype(np.int32)
    live = out == 0
    while live.any():
        nxt = np.full(len(p), -1, np.int64)
        for k in range(8):
            kid = np.where(live, children[cur] + k, 0)
            go = live & (nxt < 0) & (children[kid] != 0) & holds(kid)
            nxt[go] = kid[go]
        live = nxt >= 0
        cur = np.where(live, nxt, cur)
        out[live] += 1
    return out
