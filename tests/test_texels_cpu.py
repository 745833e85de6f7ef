"""The lightmap texels' reference (tests/texel_ref.py, tests/c/texel_ref.c) pinned without a GPU: the
coverage rule against an independent numpy restatement and against float64 geometry, watertightness
on jittered UV grids with vertices snapped onto texel centres, ties and rejected faces, the normals
against a numpy f32 restatement of shade.h's scene_finish, and the dilation on a hand-worked case.
tests/test_gpu_texels.py then holds the device to this reference bit for bit.

Covered counts of the loader's meshes (numpy restatement == reference):
    Cube  1x1 0 of 1,  7x5 22 of 35,  64x64 2,709 of 4,096,  200x120 16,040 of 24,000
    Deer  1x1 1 of 1,  7x5 30 of 35,  64x64 3,127 of 4,096,  200x120 18,410 of 24,000"""
import numpy as np
import pytest

from atray_amd import engine as E
from atray_amd.assets import asset_path
from tests import texel_ref as TX

F = np.float32
NONE = 0xFFFFFFFF
SIZES = [(1, 1), (7, 5), (64, 64), (200, 120)]
COUNTS = {("Cube", 1, 1): 0, ("Cube", 7, 5): 22, ("Cube", 64, 64): 2709, ("Cube", 200, 120): 16040,
          ("Deer", 1, 1): 1, ("Deer", 7, 5): 30, ("Deer", 64, 64): 3127, ("Deer", 200, 120): 18410}

_arrays = {}


def arrays(asset):
    """Mesh.arrays() of a golden asset (cached; read-only)."""
    if asset not in _arrays:
        _arrays[asset] = tuple(np.array(a) for a in E.Mesh.load_obj(asset_path(asset)).arrays())
        for a in _arrays[asset]:
            a.setflags(write=False)
    return _arrays[asset]


def parse(text):
    return tuple(np.array(a) for a in E.Mesh.parse_obj(text).arrays())


# ---------------------------------------------------------------- numpy restatement of the rule
def centres(w, h):
    px = (np.arange(w, dtype=F) + F(0.5)) / F(w)
    py = (np.arange(h, dtype=F) + F(0.5)) / F(h)
    return np.broadcast_to(px[None, :], (h, w)).copy(), np.broadcast_to(py[:, None], (h, w)).copy()


def np_edge(p0, p1, px, py):
    s = F(1)
    if p1[0] < p0[0] or (p1[0] == p0[0] and p1[1] < p0[1]):
        p0, p1, s = p1, p0, F(-1)
    return s * ((p1[0] - p0[0]) * (py - p0[1]) - (p1[1] - p0[1]) * (px - p0[0]))


def np_usable(T, ft):
    if (ft < 0).any() or (ft >= len(T)).any():
        return None
    a, b, c = (T[i, :2].astype(F) for i in ft)
    if not np.isfinite(np.concatenate([a, b, c])).all():
        return None
    with np.errstate(all="ignore"):
        area2 = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    if area2 == 0 or np.isnan(area2):
        return None
    return a, b, c, F(1) if area2 > 0 else F(-1)


def np_face_cover(T, ft, px, py):
    """(covered mask, e1, e2, den) of one face over all centres, or None for an unusable face."""
    u = np_usable(T, ft)
    if u is None:
        return None
    a, b, c, g = u
    with np.errstate(all="ignore"):
        e0, e1, e2 = g * np_edge(b, c, px, py), g * np_edge(c, a, px, py), g * np_edge(a, b, px, py)
        den = (e0 + e1) + e2
    return (e0 >= 0) & (e1 >= 0) & (e2 >= 0) & (den > 0), e1, e2, den


def np_map(arr, w, h):
    """The lowest usable covering face per texel ((h, w) uint32, NONE = not covered) and how many
    usable faces cover each texel."""
    T, FT = arr[2], arr[4]
    px, py = centres(w, h)
    m = np.full((h, w), NONE, np.uint32)
    n = np.zeros((h, w), np.int32)
    for f in range(len(FT)):
        r = np_face_cover(T, FT[f], px, py)
        if r is None:
            continue
        m[(m == NONE) & r[0]] = f
        n += r[0]
    return m, n


def ref_map(r, w, h):
    m = np.full(w * h, NONE, np.uint32)
    m[r["texel"]] = r["face"]
    return m.reshape(h, w)


def check_structure(r, w, h):
    """slot and texel describe each other; texel is ascending."""
    k = len(r["texel"])
    assert (np.diff(r["texel"].astype(np.int64)) > 0).all()
    assert np.array_equal(r["slot"][r["texel"]], np.arange(k))
    assert (r["slot"] >= 0).sum() == k and (r["slot"][r["slot"] < 0] == -1).all()


# ---------------------------------------------------------------- synthetic UV grids
def grid_obj(n, w, h, seed=7):
    """An n x n grid of UV quads over [0,1]^2 as OBJ text: interior vertices jittered by +-0.3/n, every
    second vertex of the diagonal snapped exactly onto a texel centre of a w x h map, each quad two
    triangles with the diagonal and the winding alternating. The surface is a gentle height field."""
    rng = np.random.default_rng(seed)
    uv = np.zeros((n + 1, n + 1, 2))
    for j in range(n + 1):
        for i in range(n + 1):
            u, v = i / n, j / n
            if 0 < i < n and 0 < j < n:
                u += rng.uniform(-0.3, 0.3) / n
                v += rng.uniform(-0.3, 0.3) / n
                if i == j and i % 2 == 1:  # onto the nearest centre, in the reference's f32 arithmetic
                    ci, cj = min(int(u * w), w - 1), min(int(v * h), h - 1)
                    u, v = float((F(ci) + F(0.5)) / F(w)), float((F(cj) + F(0.5)) / F(h))
            uv[j, i] = u, v
    lines = []
    for j in range(n + 1):
        for i in range(n + 1):
            u, v = uv[j, i]
            lines.append(f"v {u * 2 - 1:.9g} {0.2 * np.sin(3 * u) * np.cos(2 * v):.9g} {v * 2 - 1:.9g}")
    for j in range(n + 1):
        for i in range(n + 1):
            lines.append(f"vt {float(F(uv[j, i, 0])):.9g} {float(F(uv[j, i, 1])):.9g}")
    idx = lambda i, j: j * (n + 1) + i + 1  # noqa: E731
    for j in range(n):
        for i in range(n):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            tris = [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
            if (i + 2 * j) % 3 == 0:
                tris[1] = tris[1][::-1]  # mixed winding
            if (i * 5 + j) % 4 == 0:
                tris[0] = tris[0][::-1]
            for t in tris:
                lines.append("f " + " ".join(f"{k}/{k}" for k in t))
    return "\n".join(lines) + "\n"


# ---------------------------------------------------------------- coverage of the loader's meshes
@pytest.mark.parametrize("asset", ["Cube", "Deer"])
def test_coverage_of_loaded_meshes(asset):
    arr = arrays(asset)
    V, _, T, FV, FT, _ = arr
    assert len(T) > 0
    extent = float(np.abs(V.max(0) - V.min(0)).max())
    for w, h in SIZES:
        r = TX.mesh_texels(arr, w, h)
        check_structure(r, w, h)
        m, _ = np_map(arr, w, h)
        print(f"{asset} {w}x{h}: {len(r['texel'])} of {w * h} covered (numpy restatement {(m != NONE).sum()})")
        assert np.array_equal(ref_map(r, w, h), m)
        assert len(r["texel"]) == (m != NONE).sum() == COUNTS[asset, w, h]
        if not len(r["texel"]):
            continue
        # the centre inside the face's UV triangle, in float64: at most 1e-6 outside any edge
        t = r["texel"].astype(np.int64)
        p = np.stack([(F(0.5) + (t % w).astype(F)) / F(w), (F(0.5) + (t // w).astype(F)) / F(h)], 1).astype(np.float64)
        tri = T[FT[r["face"]]][:, :, :2].astype(np.float64)  # (k, 3, 2)
        a, b, c = tri[:, 0], tri[:, 1], tri[:, 2]
        sgn = np.sign((b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0]))
        for p0, p1 in ((a, b), (b, c), (c, a)):
            e = (p1[:, 0] - p0[:, 0]) * (p[:, 1] - p0[:, 1]) - (p1[:, 1] - p0[:, 1]) * (p[:, 0] - p0[:, 0])
            assert (sgn * e / np.hypot(*(p1 - p0).T) >= -1e-6).all()
        u, v = r["bary"][:, 0], r["bary"][:, 1]
        assert (u >= 0).all() and (v >= 0).all() and (u + v <= F(1) + F(2.0 ** -20)).all()
        # the point on the face's plane, within 1e-5 of the mesh's extent
        A, B, Cc = (V[FV[r["face"], q]].astype(np.float64) for q in range(3))
        nrm = np.cross(B - A, Cc - A)
        nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
        assert (np.abs(((r["point"].astype(np.float64) - A) * nrm).sum(1)) <= 1e-5 * extent).all()
        want = A + (B - A) * u[:, None].astype(np.float64) + (Cc - A) * v[:, None].astype(np.float64)
        assert (np.abs(r["point"] - want) <= 1e-5 * extent).all()


# ---------------------------------------------------------------- watertight
@pytest.mark.parametrize("n", [3, 8, 20])
def test_grids_are_watertight(n):
    for w, h in [(1, 1), (7, 5), (64, 64), (257, 129)]:
        arr = parse(grid_obj(n, w, h))
        assert len(arr[3]) == 2 * n * n
        r = TX.mesh_texels(arr, w, h)
        check_structure(r, w, h)
        assert len(r["texel"]) == w * h, f"{w * h - len(r['texel'])} empty texels"
        m, cnt = np_map(arr, w, h)
        assert np.array_equal(ref_map(r, w, h), m)  # wherever two faces cover a centre, the lower index wins
        assert (cnt >= 1).all()
        if (w, h) == (64, 64) and n > 3:
            # the snapped vertices landed on centres exactly, so ties between faces are exercised
            px, py = centres(w, h)
            on = [(px == t[0]) & (py == t[1]) for t in arr[2][:, :2]]
            assert sum(o.any() for o in on) >= 1 and (cnt >= 2).any()


# ---------------------------------------------------------------- ties and rejects
QUAD = """v 0 0 0
v 1 0 0
v 1 0 1
v 0 0 1
v 0 1 0
vt 0.05 0.1
vt 0.9 0.15
vt 0.85 0.95
vt 0.1 0.8
f 1/1 2/2 3/3
f 1/1 3/3 4/4
"""


def test_identical_uvs_lowest_index_wins():
    arr = parse(QUAD + "f 1/1 2/2 3/3\nf 5/1 3/3 4/4\n")
    for w, h in [(7, 5), (64, 64)]:
        r = TX.mesh_texels(arr, w, h)
        base = TX.mesh_texels(parse(QUAD), w, h)
        assert len(r["texel"]) > 0 and r["face"].max() <= 1
        for k in TX.KEYS:
            assert TX.same_bits(r[k], base[k]), k


@pytest.mark.parametrize("extra", [
    "f 1/1 2 3/3\n",                                     # a missing vt
    "vt 0.5 0.5\nvt 0.5 0.5\nf 1/5 2/6 3/5\n",            # zero area
    "vt 0.2 0.2\nvt 0.8 0.8\nvt 0.5 0.5\nf 1/5 2/6 3/7\n",  # collinear: zero area
    "vt 0.3 0.5\nf 1/5 2/2 3/3\n",                       # a NaN UV (patched in below: OBJ text cannot hold one)
    "vt 1e999 0.5\nf 1/5 2/2 3/3\n",                     # an infinite UV, or whatever the parser makes of it
    "vt 5.1 5.2\nvt 5.9 5.3\nvt 5.5 5.95\nf 1/5 2/6 3/7\n",  # UVs at 5..6: nothing inside the map
])
def test_rejected_faces_leave_the_others_alone(extra):
    """The extra face comes first, so it would win every tie; the other faces move up by one."""
    head, faces = QUAD.split("f ", 1)
    nvt = extra.count("vt ")
    text = head + "".join(ln + "\n" for ln in extra.splitlines() if ln.startswith("vt")) + \
        [ln for ln in extra.splitlines() if ln.startswith("f ")][0] + "\nf " + faces
    arr = parse(text)
    assert len(arr[3]) == 3 and len(arr[2]) == 4 + nvt
    if "0.3 0.5" in extra:
        assert len(TX.mesh_texels(arr, 7, 5)["face"]) and TX.mesh_texels(arr, 7, 5)["face"].min() == 0  # usable as parsed
        arr[2][4, 0] = np.nan
    if "1e999" in extra and np.isfinite(arr[2]).all():
        arr[2][4, 0] = np.inf
    for w, h in [(7, 5), (64, 64)]:
        r, base = TX.mesh_texels(arr, w, h), TX.mesh_texels(parse(QUAD), w, h)
        assert len(base["texel"]) > 0
        assert np.array_equal(r["face"], base["face"] + 1)
        for k in ("slot", "texel", "bary", "point", "normal"):
            assert TX.same_bits(r[k], base[k]), k


# ---------------------------------------------------------------- normals
def np_unit(n):
    l2 = (n[:, 0] * n[:, 0]) + (n[:, 1] * n[:, 1]) + (n[:, 2] * n[:, 2])
    with np.errstate(all="ignore"):
        return n * (F(1) / np.sqrt(l2))[:, None]


def np_normals(arr, face, bary):
    """shade.h's scene_finish for a model hit at (face, u, v), in numpy f32 operations."""
    V, N, _, FV, _, FN = arr
    u, v = bary[:, 0:1], bary[:, 1:2]
    if len(N):  # smooth: the mesh has normals
        na, nb, nc = (N[FN[face, q]] for q in range(3))
        n = (na * ((F(1) - u) - v) + nb * u) + nc * v
    else:
        v0, v1, v2 = (V[FV[face, q]] for q in range(3))
        a, b = v0 - v1, v0 - v2
        n = np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                      a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)
    return np_unit(n.astype(F))


@pytest.mark.parametrize("asset", ["Cube", "Deer"])
def test_normals_are_the_renderers(asset):
    arr = arrays(asset)
    assert (len(arr[1]) > 0) == (asset == "Cube")  # Cube has vn: the smooth path; Deer has none: flat
    r = TX.mesh_texels(arr, 64, 64)
    want = np_normals(arr, r["face"], r["bary"])
    assert TX.same_bits(r["normal"], want)
    assert np.isfinite(r["normal"]).all()
    assert (np.abs((r["normal"].astype(np.float64) ** 2).sum(1) - 1) < 1e-6).all()
    fl = TX.mesh_texels(arr, 64, 64, flip=True)
    assert ((fl["normal"].view(np.uint32) ^ r["normal"].view(np.uint32)) == 0x80000000).all()
    for k in ("slot", "texel", "face", "bary", "point"):
        assert TX.same_bits(fl[k], r[k]), k


# ---------------------------------------------------------------- dilation
def test_dilation_hand_worked():
    """5 x 5, seeds at (0, 0) = (1, 2, 3) and (3, 2) = (10, 20, 30), fill (-1, -2, -3)."""
    w = h = 5
    texel = np.array([0, 2 * 5 + 3], np.int32)
    vals = np.array([[1, 2, 3], [10, 20, 30]], F)
    fill = (-1, -2, -3)
    A, B, FILL = np.array([1, 2, 3], F), np.array([10, 20, 30], F), np.array(fill, F)
    img = [TX.texels_to_image(vals, texel, w, h, p, fill) for p in range(5)]
    at = lambda p, x, y: img[p][y, x]  # noqa: E731
    # no pass: the two seeds, everything else the fill
    assert np.array_equal(at(0, 0, 0), A) and np.array_equal(at(0, 3, 2), B)
    assert (img[0].reshape(-1, 3) == FILL).all(1).sum() == 23
    # one pass: the seeds' rings, each with one neighbour: (0 + v) / 1
    for x, y in [(1, 0), (0, 1), (1, 1)]:
        assert np.array_equal(at(1, x, y), A)
    for x in (2, 3, 4):
        for y in (1, 2, 3):
            assert np.array_equal(at(1, x, y), B)
    assert (img[1].reshape(-1, 3) == FILL).all(1).sum() == 25 - 4 - 9
    # two passes: (2, 0) sees (1, 0), then (1, 1), (2, 1), (3, 1) of the first pass -- (3, 0) was empty
    # when the pass began: (((0 + 1) + 1) + 10) + 10 = 22 over 4
    assert np.array_equal(at(2, 2, 0), np.array([22, 44, 66], F) / F(4))
    # (1, 2): (0, 1), (1, 1), (2, 1); (2, 2); (2, 3): 1 + 1 + 10 + 10 + 10 over 5
    assert np.array_equal(at(2, 1, 2), np.array([32, 64, 96], F) / F(5))
    assert np.array_equal(at(2, 0, 2), A)  # (0, 1) and (1, 1): (1 + 1) / 2
    empty2 = {(x, y) for y in range(h) for x in range(w) if np.array_equal(at(2, x, y), FILL)}
    assert empty2 == {(0, 3), (0, 4)}
    # the texels of earlier passes keep their values
    for p in (1, 2, 3, 4):
        assert np.array_equal(at(p, 0, 0), A) and np.array_equal(at(p, 3, 2), B) and np.array_equal(at(p, 1, 1), A)
    # three passes fill the map; one pass beyond full changes nothing and leaves no fill
    assert not (img[3].reshape(-1, 3) == FILL).all(1).any()
    assert np.array_equal(img[3].view(np.uint32), img[4].view(np.uint32))
    assert np.array_equal(img[3].view(np.uint32), TX.texels_to_image(vals, texel, w, h, 64, fill).view(np.uint32))


def test_dilation_sums_in_dy_then_dx_order():
    """Neighbours 1, 1e8, -1e8 in dx order: ((0 + 1) + 1e8) + -1e8 = 0 in f32; the reverse order gives 1.
    The same three down a column pin the dy order."""
    vals = np.array([[1, 1, 1], [1e8, 1e8, 1e8], [-1e8, -1e8, -1e8]], F)
    row = TX.texels_to_image(vals, np.array([0, 1, 2], np.int32), 3, 2, 1)
    assert np.array_equal(row[1, 1], np.zeros(3, F))
    # the end texels see two neighbours each: (0 + 1) + 1e8 over 2, and (0 + 1e8) + -1e8 over 2
    assert np.array_equal(row[1, 0], np.full(3, F(1e8) / F(2))) and np.array_equal(row[1, 2], np.zeros(3, F))
    col = TX.texels_to_image(vals, np.array([0, 2, 4], np.int32), 2, 3, 1)
    assert np.array_equal(col[1, 1], np.zeros(3, F))
    rev = TX.texels_to_image(vals[::-1].copy(), np.array([0, 2, 4], np.int32), 2, 3, 1)
    assert np.array_equal(rev[1, 1], np.full(3, F(1) / F(3)))
