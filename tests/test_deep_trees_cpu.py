"""The generated trees of tests/deep_trees.py, pinned on the CPU: their exact depths (8, 9, 15, 16)
and inner-node counts (one tree at 2^16 or more, its twin below), so that a change in a generator
cannot move tests/test_gpu_deep_trees.py back to shallow trees without a failure here; the host build
of each nested tree against the oracle's, bit for bit; export -> from_nodes -> export at depth 15 and
16; and the share of an inside camera's primary rays that scan a leaf at depth 9 or more (the cap
the GPU test's deep-walk claim rests on). No compute call touches a GPU here."""
import numpy as np
import pytest

from atray_amd import engine as E
from oracle import oracle as O
from tests import deep_trees as D

IMG_W, IMG_H = 64, 48
# inner nodes of each tree (oracle build and host build agree: asserted below)
INNER = {"d8": 56, "d9": 62, "d15": 100, "d16": 104, "wide": 90045, "twin": 37470}
FACING = (-0.1, -0.5, -1.0)

_eparts, _oparts, _exports = {}, {}, {}


def epart(name):
    """The engine's (mesh, tree, box) of a generated tree (cached). The mesh stays where it was
    generated: no translate_to."""
    if name not in _eparts:
        m = E.Mesh.parse_obj(D.text(name))
        _eparts[name] = (m, E.Octree.build(m, D.leaf_size(name)), m.aabb())
    return _eparts[name]


def opart(name, material=1):
    """The oracle's one-model scene of a generated tree (cached)."""
    if (name, material) not in _oparts:
        _oparts[name, material] = O.Scene(obj_text=D.text(name), center=None, max_faces=D.leaf_size(name),
                                          model_material=material)
    return _oparts[name, material]


def exported(name):
    """Octree.export() of the host build (cached, read-only)."""
    if name not in _exports:
        ex = epart(name)[1].export()
        for a in ex:
            a.setflags(write=False)
        _exports[name] = ex
    return _exports[name]


def inside_camera(name):
    """Eye at the centre of the deepest inner node's box: every primary ray starts at the bottom of
    the tree and walks the deep levels first."""
    bounds, children = exported(name)[:2]
    return dict(eye=D.centre(D.deepest_inner(bounds, children)[2]), facing=FACING)


def outside_camera(name):
    """Eye outside the mesh, looking at the focus the shells close in on."""
    off = [(0.19, 0.51, 1.40)[k] * D.S0 for k in range(3)] if name in D.NESTED else (7.0, 18.0, 50.0)
    return dict(eye=tuple(f + o for f, o in zip(D.FOCUS, off)), facing=tuple(-o for o in off))


def deep_scan_share(name, min_depth=9, **cam):
    """The share of a camera's primary rays that scan a leaf at depth min_depth or more (oracle)."""
    nodes = opart(name).tree_arrays()[0]
    depth = D.node_depths(nodes["children"])
    leaves, _ = opart(name).leaf_trace(O.Camera(IMG_W, IMG_H, **cam), cap=64)
    deep = (leaves >= 0) & (depth[np.maximum(leaves, 0)] >= min_depth)
    return float(deep.any(axis=2).mean())


@pytest.mark.parametrize("name", list(D.NESTED))
def test_nested_depths_are_exact(name):
    st = epart(name)[1].stats()
    assert st["depth"] == D.NESTED[name][2], st
    assert st["inner"] == INNER[name], st
    bounds, children = exported(name)[:2]
    depth = D.node_depths(children)
    assert int(depth.max()) == st["depth"]
    assert D.deepest_inner(bounds, children)[1] == st["depth"] - 1  # the deepest nodes are leaves


def test_nested_depths_cover_the_limits():
    assert sorted(v[2] for v in D.NESTED.values()) == [8, 9, 15, 16]


def test_wide_trees_straddle_the_inner_node_limit():
    wide, twin = epart("wide")[1].stats(), epart("twin")[1].stats()
    assert wide["inner"] == INNER["wide"] >= 65536 and wide["depth"] <= 8, wide
    assert twin["inner"] == INNER["twin"] < 65536 and twin["depth"] <= 8, twin
    assert wide["depth"] == 8 and twin["depth"] == 7


@pytest.mark.parametrize("name", list(D.NESTED))
def test_host_build_bit_identical_to_oracle(name):
    m, t, box = epart(name)
    s = opart(name)
    assert np.array_equal(box.view(np.uint32), s.surrounding_aabb.view(np.uint32))
    st, os_ = t.stats(), s.tree_stats()
    for k in ["nodes", "inner", "leaves", "empty_leaves", "leaf_prim_refs", "max_leaf"]:
        assert st[k] == os_[k], k
    bounds, children, first, count, verts, face = exported(name)
    nodes, otri, oface = s.tree_arrays()
    assert np.array_equal(bounds[:, :3].view(np.uint32), nodes["bmin"].view(np.uint32))
    assert np.array_equal(bounds[:, 3:].view(np.uint32), nodes["bmax"].view(np.uint32))
    assert np.array_equal(children, nodes["children"])
    leaf = children == 0
    assert np.array_equal(first[leaf], nodes["prim_off"][leaf])
    assert np.array_equal(count[leaf], nodes["prim_cnt"][leaf])
    assert np.array_equal(verts.view(np.uint32), otri.view(np.uint32))
    assert np.array_equal(face, oface)
    assert int(D.node_depths(nodes["children"]).max()) == st["depth"]


@pytest.mark.parametrize("name", ["d15", "d16"])
def test_export_from_nodes_roundtrip_at_depth(name):
    ex = exported(name)
    t = E.Octree.from_nodes(*ex)  # depth 16 is a valid tree: only an upload rejects it
    assert t.stats() == epart(name)[1].stats()
    for n, a, b in zip(["bounds", "children", "leaf_first", "leaf_count", "prim_vertices", "prim_face"], ex, t.export()):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), n


@pytest.mark.parametrize("name", ["d9", "d15"])
def test_inside_camera_scans_deep_leaves(name):
    """At least 90 % of the inside camera's primary rays scan a leaf at depth 9 or more, so a render
    from it does walk the levels kept in the high half of the mask stack."""
    share = deep_scan_share(name, **inside_camera(name))
    assert share >= 0.9, share


def test_tree_helpers_on_a_hand_made_tree():
    """node_depths, deepest_inner and inner_depth_at on a two-level tree written out by hand."""
    def kids(lo, hi, v):
        out = []
        for k in range(8):
            bit = (k >> 2, (k >> 1) & 1, k & 1)
            out.append([v[a] if bit[a] else lo[a] for a in range(3)] + [hi[a] if bit[a] else v[a] for a in range(3)])
        return out

    b = [[0, 0, 0, 8, 8, 8]] + kids((0, 0, 0), (8, 8, 8), (4, 4, 4))
    b += kids((4, 4, 4), (8, 8, 8), (6, 6, 6))  # child 7 of the root is inner
    bounds = np.array(b, np.float32)
    children = np.zeros(17, np.int32)
    children[0], children[8] = 1, 9
    assert D.node_depths(children).tolist() == [0] + [1] * 8 + [2] * 8
    node, depth, box = D.deepest_inner(bounds, children)
    assert (node, depth, box.tolist()) == (8, 1, [4, 4, 4, 8, 8, 8])
    pts = [(1, 1, 1), (5, 5, 5), (7, 5, 7), (9, 1, 1), (3, 7, 7)]
    assert D.inner_depth_at(bounds, children, pts).tolist() == [0, 1, 1, -1, 0]
    assert len(D.leaf_boxes(bounds, children, np.ones(17, np.uint32), 2, limit=3)) == 3
