"""atr_gather_occlusion and atr_gather_directions without a GPU: the symbols, their bindings and the
NULL-context answer; the host sampler against the reference of the GPU tests (tests/gather_ref.py)
and against a numpy restatement built from the oracle's RNG, bit for bit; the reference's counts
against the occlusion reference on its own directions; surface_points. Also the point sets the GPU
tests share (points)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import gather_ref as GR  # noqa: E402
from tests import occlusion_ref as OR  # noqa: E402
from tests import ray_sets as R  # noqa: E402
from tests import test_gpu_trace_rays as TR  # noqa: E402

F = np.float32
INV_U32 = F(2.328306437e-10)  # engine.h kInvU32Max
SEED = 0x853C49E6748FEA9B
N_HITS, N_INSIDE = 257, 65

_points = {}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def np_dot(a, b):  # engine.h:50
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def np_unit(v):
    """engine.h unit() with the correctly rounded f32 square root (through f64)."""
    v = np.asarray(v, F)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = F(1.0) / np.sqrt(R.len2(v).astype(np.float64)).astype(F)
        return (v * inv[:, None]).astype(F)


def np_surface_points(orig, dirs, t, normal):
    """bounce_shade's convention (scan.h): p = o + d * t, n negated where dot(-d, n) < 0."""
    p = (orig + (dirs * t[:, None]).astype(F)).astype(F)
    att = np_dot(-dirs, normal)
    return p, np.where((att < 0)[:, None], -normal, normal).astype(F)


def np_directions(normals, nsamples, first_sample=0, point_base=0, seed=0):
    """The sampler from oracle.pcg_sequence / om_path_rng in numpy f32: (dirs, traced)."""
    normals = np.asarray(normals, F)
    n = len(normals)
    u = np.empty((n, nsamples, 3), np.uint32)
    L = O.lib()
    for i in range(n):
        for s in range(nsamples):
            st, stream = C.c_uint64(), C.c_uint64()
            L.om_path_rng(C.c_uint64(seed), point_base + i, first_sample + s, C.byref(st), C.byref(stream))
            u[i, s] = O.pcg_sequence(st.value, stream.value, 3)
    r = (F(-1.0) + F(2.0) * (u.astype(F) * INV_U32).astype(F)).astype(F)
    v = (r + normals[:, None, :]).astype(F).reshape(-1, 3)
    d = np_unit(v)
    nn = np.repeat(normals, nsamples, axis=0)
    with np.errstate(invalid="ignore"):
        traced = R.passes(np.zeros_like(d), d) & (np_dot(d, nn) > 0)
    ok = np.repeat(R.passes(np.zeros_like(normals), normals), nsamples)
    d[~ok] = 0
    traced &= ok
    return d.reshape(n, nsamples, 3), traced.astype(np.uint8).reshape(n, nsamples)


def points(name):
    """The point set of a scene (cached, read-only): the hit points and flipped normals of the first 257
    hits of its aimed batch (the oracle's trace, shade.h's normal restated in numpy, the numpy
    surface_points), then 65 points inside the focus box with random unit normals. (p, n)."""
    if name not in _points:
        sc = TR.SCENES[name]
        orig, dirs = (a[:1200] for a in TR.rays(name, "aimed"))
        face, t, uv, _ = sc.oracle().trace(orig, dirs)
        if sc.names:
            kind, model, _ = TR.derived(name, orig, dirs)
            nrm = TR.shade_normal(sc, orig, dirs, {"kind": kind, "model": model, "face": face, "t": t, "uv": uv})
        else:  # spheres and planes alone: the sphere that holds the hit point, else the plane's normal
            kind = np.where(t < R.MAX_FLOAT, E.ATR_RAY_PLANE, E.ATR_RAY_SKY)
            at = (orig + (dirs * t[:, None]).astype(F)).astype(F)
            nrm = np.broadcast_to(np.asarray(sc.planes[0][0], F), at.shape).copy()
            for c, r, _ in sc.spheres:
                v = at - np.asarray(c, F)
                with np.errstate(invalid="ignore", over="ignore"):
                    on = np.abs(np.sqrt(R.len2(v)) - F(r)) < F(1e-3)
                nrm[on] = np_unit(v[on])
        hit = np.flatnonzero(kind != E.ATR_RAY_SKY)[:N_HITS]
        assert len(hit) == N_HITS, (name, len(hit))
        p, n = np_surface_points(orig[hit], dirs[hit], t[hit], nrm[hit])
        q, m = R.inside(TR.focus(name), N_INSIDE, 26)
        p, n = np.concatenate([p, q]).astype(F), np.concatenate([n, m]).astype(F)
        assert R.passes(p, n).all(), name
        p.setflags(write=False)
        n.setflags(write=False)
        _points[name] = (p, n)
    return _points[name]


# ---- the entry points ----------------------------------------------------------------------------------

def test_library_exports_the_gather():
    for name in ("atr_gather_occlusion", "atr_gather_directions"):
        assert name in E.EXPORTS and hasattr(E.lib(), name)
    for name in ("gather_directions", "surface_points"):
        assert callable(getattr(E, name))
    for name in ("gather_occlusion", "ambient_occlusion"):
        assert callable(getattr(E.Engine, name))


def test_bindings():
    args, res = E.signatures()["atr_gather_occlusion"]
    assert len(args) == 12 and res is C.c_int
    assert args[4] is C.c_int64 and args[5] is C.c_int32 and args[6] is C.c_uint32 and args[7] is C.c_int64
    assert args[8] is C.c_uint64 and args[10] is C.c_int32
    assert [f[0] for f in E.atr_gather_out._fields_] == ["visible", "occluded", "mask", "dirs", "traced_rays"]
    assert C.sizeof(E.atr_gather_out) == 40
    args, res = E.signatures()["atr_gather_directions"]
    assert len(args) == 8 and res is C.c_int and args[1] is C.c_int64 and args[2] is C.c_int32


def test_null_context_is_invalid_without_a_device():
    f = E.lib().atr_gather_occlusion
    out = E.atr_gather_out()
    assert f(None, None, None, None, 0, 16, 0, 0, 0, C.byref(out), E.ATR_KERNEL_AUTO, None) == -1
    assert f(None, None, None, None, 5, 16, 0, 0, 0, None, E.ATR_KERNEL_AUTO, None) == -1


def test_directions_range_checks():
    g = E.lib().atr_gather_directions
    nrm = np.array([[0, 0, 1]], F)
    d, t = np.zeros((1, 4, 3), F), np.zeros((1, 4), np.uint8)
    p = lambda a: a.ctypes.data  # noqa: E731
    assert g(p(nrm), 1, 4, 0, 0, 0, p(d), p(t)) == 0
    assert g(p(nrm), 0, 4, 0, 0, 0, None, None) == 0 and g(None, 0, 4, 0, 0, 0, None, None) == 0
    for npts, ns, first, base in ((1, 0, 0, 0), (1, 65537, 0, 0), (1, 4, 2 ** 24 - 3, 0), (1, 4, 0, -1),
                                  (1, 4, 0, 2 ** 39), (-1, 4, 0, 0), (2 ** 15, 65536, 0, 0)):
        assert g(p(nrm), npts, ns, first, base, 0, None, None) == -1, (npts, ns, first, base)
    assert g(None, 1, 4, 0, 0, 0, p(d), p(t)) == -1
    assert g(p(nrm), 1, 4, 2 ** 24 - 4, 2 ** 39 - 1, 0, p(d), p(t)) == 0  # both at their upper ends


# ---- the sampler: host function == reference == numpy ------------------------------------------------

def normal_sets():
    rng = np.random.default_rng(51)
    axis = np.array([[1, 0, 0], [0, -1, 0], [0, 0, 1], [-0.0, 0.0, -1.0]], F)
    diag = np_unit(np.array([[1, 1, 1], [1, -1, 0], [-1, 2, -3], [0.0, 1, 1e-3]], F))
    return {"axis": axis, "diagonal": diag, "random": R.random_dirs(9, rng)}


@pytest.mark.parametrize("which", ["axis", "diagonal", "random"])
@pytest.mark.parametrize("first,base,seed", [(0, 0, 0), (5, 1000, SEED), (2 ** 24 - 40, 2 ** 39 - 9, 3)])
def test_directions_match_reference_and_numpy(which, first, base, seed):
    nrm = normal_sets()[which][:2 ** 39 - base]
    ns = 40
    d, t = E.gather_directions(nrm, ns, first, base, seed)
    rd, rt = GR.directions(nrm, ns, first, base, seed)
    nd, nt = np_directions(nrm, ns, first, base, seed)
    assert d.shape == (len(nrm), ns, 3) and t.shape == (len(nrm), ns) and t.dtype == np.uint8
    assert np.array_equal(bits(d), bits(rd)) and np.array_equal(t, rt)
    assert np.array_equal(bits(d), bits(nd)) and np.array_equal(t, nt)
    assert R.passes(np.zeros((t.sum(), 3), F), d[t == 1]).all()
    if which == "axis":
        assert (t == 1).all()  # an axis normal's samples stay above its plane
    print(which, "below the plane or invalid:", int((t == 0).sum()), "of", t.size)


def test_directions_reach_below_the_plane_for_oblique_normals():
    nrm = np.concatenate([normal_sets()["diagonal"], normal_sets()["random"]])
    _, t = E.gather_directions(nrm, 512, seed=SEED)
    share = 1.0 - t.mean(axis=1)
    print("untraced share per normal", np.round(share, 4).tolist())
    assert (share > 0).any() and share.max() < 0.08  # the issue's numpy figure: 3.0-4.3 %


def test_directions_split_invariance():
    nrm = normal_sets()["random"]
    whole_d, whole_t = E.gather_directions(nrm, 100, 7, 50, SEED)
    for fn in (GR.directions, np_directions):  # the whole, then every cut, against it
        d, t = fn(nrm, 100, 7, 50, SEED)
        assert np.array_equal(bits(d), bits(whole_d)) and np.array_equal(t, whole_t), fn.__name__
    for cut in (1, 4, 8):  # a point cut
        a = E.gather_directions(nrm[:cut], 100, 7, 50, SEED)
        b = E.gather_directions(nrm[cut:], 100, 7, 50 + cut, SEED)
        assert np.array_equal(bits(np.concatenate([a[0], b[0]])), bits(whole_d))
        assert np.array_equal(np.concatenate([a[1], b[1]]), whole_t)
    for cut in (1, 37, 64):  # a sample cut
        a = E.gather_directions(nrm, cut, 7, 50, SEED)
        b = E.gather_directions(nrm, 100 - cut, 7 + cut, 50, SEED)
        assert np.array_equal(bits(np.concatenate([a[0], b[0]], axis=1)), bits(whole_d))
        assert np.array_equal(np.concatenate([a[1], b[1]], axis=1), whole_t)


def test_bad_normals_come_back_zero_and_unflagged():
    nrm = normal_sets()["random"].copy()
    nrm[2] *= F(1.001)  # not unit
    nrm[5, 1] = np.nan
    nrm[7] = 0
    good = np.ones(len(nrm), bool)
    good[[2, 5, 7]] = False
    for fn in (E.gather_directions, GR.directions, np_directions):
        d, t = fn(nrm, 33, 0, 0, SEED)
        assert (bits(d[~good]) == 0).all() and (t[~good] == 0).all(), fn.__name__
        want = E.gather_directions(nrm[good], 33, 0, 0, SEED)
        for k, row in enumerate(np.flatnonzero(good)):  # the neighbours: their own streams
            solo = E.gather_directions(nrm[row:row + 1], 33, 0, int(row), SEED)
            assert np.array_equal(bits(d[row]), bits(solo[0][0])) and np.array_equal(t[row], solo[1][0])
        assert want[0].shape == (int(good.sum()), 33, 3)


# ---- the reference's gather against the occlusion reference ---------------------------------------------

@pytest.mark.parametrize("ns,with_tmax", [(7, False), (64, True), (100, True)])
def test_reference_counts_are_sums_of_the_occlusion_reference(ns, with_tmax):
    sc = TR.SCENES["mixed"].oracle()
    p, n = points("mixed")
    tm = None
    if with_tmax:
        box = TR.boxes("mixed")[0]
        tm = np.random.default_rng(5).uniform(0.02, 0.6, len(p)).astype(F) * np.sqrt(R.len2((box[3:] - box[:3])[None]))[0]
    g = GR.gather(sc, p, n, ns, tm, 3, 11, SEED)
    d, t = E.gather_directions(n, ns, 3, 11, SEED)
    assert np.array_equal(bits(g["dirs"]), bits(d)) and np.array_equal(g["flags"], t)
    flat = t.reshape(-1) == 1
    o = np.repeat(p, ns, axis=0)[flat]
    tt = None if tm is None else np.repeat(tm, ns)[flat]
    occ = np.zeros(len(p) * ns, np.uint8)
    occ[flat] = OR.occluded(sc, o, d.reshape(-1, 3)[flat], tt)
    vis = np.zeros(len(p) * ns, np.uint8)
    vis[flat] = 1 - occ[flat]
    assert np.array_equal(g["occluded"], occ.reshape(-1, ns).sum(axis=1).astype(np.uint32))
    assert np.array_equal(g["visible"], vis.reshape(-1, ns).sum(axis=1).astype(np.uint32))
    assert g["traced"] == int(flat.sum())
    words = (ns + 31) // 32
    padded = np.zeros((len(p), words * 32), np.uint8)
    padded[:, :ns] = vis.reshape(-1, ns)
    want = (padded.reshape(len(p), words, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=2)
    assert np.array_equal(g["mask"], want.astype(np.uint32))
    assert g["visible"].sum() > 0 and g["occluded"].sum() > 0 and (t == 0).any()


def test_reference_zeroes_invalid_points():
    sc = TR.SCENES["mixed"].oracle()
    p, n = (a[:6].copy() for a in points("mixed"))
    tm = np.full(6, 3.0, F)
    p[1, 2] = np.nan
    n[2] *= F(1.01)
    tm[3], tm[4] = 0.0, np.nan
    g = GR.gather(sc, p, n, 33, tm, 0, 0, SEED)
    bad = [1, 2, 3, 4]
    for k in ("visible", "occluded", "mask", "flags"):
        assert (g[k][bad] == 0).all(), k
    assert (bits(g["dirs"][bad]) == 0).all()
    solo = GR.gather(sc, p[5:6], n[5:6], 33, tm[5:6], 0, 5, SEED)
    for k in ("visible", "occluded", "mask"):
        assert np.array_equal(g[k][5:6], solo[k])


# ---- surface_points -----------------------------------------------------------------------------------------

def test_surface_points():
    rng = np.random.default_rng(52)
    o = rng.uniform(-50, 50, (1025, 3)).astype(F)
    d, n = R.random_dirs(1025, rng), R.random_dirs(1025, rng)
    t = rng.uniform(1e-3, 300.0, 1025).astype(F)
    p, m = (a.numpy() for a in E.surface_points(*(torch.from_numpy(a) for a in (o, d, t, n))))
    wp, wn = np_surface_points(o, d, t, n)
    assert np.array_equal(bits(p), bits(wp)) and np.array_equal(bits(m), bits(wn))
    flipped = (bits(m) != bits(n)).any(axis=1)
    assert 300 < flipped.sum() < 725  # both cases are there
    assert (np_dot(-d, m) >= 0).all()
    with pytest.raises(ValueError):
        E.surface_points(torch.from_numpy(o).double(), torch.from_numpy(d), torch.from_numpy(t), torch.from_numpy(n))
    with pytest.raises(ValueError):
        E.surface_points(torch.from_numpy(o), torch.from_numpy(d), torch.from_numpy(t[:-1]), torch.from_numpy(n))
