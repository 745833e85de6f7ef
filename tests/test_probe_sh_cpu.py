"""atr_probe_sh without a GPU: the symbols, their bindings, the NULL-context answer and the host
functions' range checks; the host sampler (atr_probe_directions) against the reference of the GPU tests
(tests/probe_sh_ref.py), cut by points and by samples, and its statistics against derived bounds; the
host basis (atr_sh_basis) against a numpy restatement and hand-worked values; the reference against
itself (cuts through sum, the fallback at max_tries 1, invalid probes) and against the numpy
restatement of the ordered sums; and the coverage conditions of the GPU tests' probe sets, asserted
here on the reference alone, so a parity test cannot pass on paths that never bounce. Also the probe
sets and reference outputs the GPU tests share (probes, want)."""
import ctypes as C
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from tests import probe_sh_ref as PR  # noqa: E402
from tests import ray_sets as R  # noqa: E402
from tests import test_gather_cpu as GC  # noqa: E402
from tests import test_gpu_trace_rays as TR  # noqa: E402

F = np.float32
SEED = GC.SEED
NAMES = ("mixed", "ties", "soup", "nomodel")
# (nsamples, bounce_limit) of the GPU parity test: around the resolve's rows of 64 slots
CONFIGS = ((1, 1), (7, 5), (63, 2), (64, 3), (65, 2), (129, 2))
PER_PROBE = ("sh", "sum", "ray_casts", "invalid")
PER_SAMPLE = ("sample_rgb", "dirs")
LIFT = F(0.05)
N_HITS, N_INSIDE = 200, 51
INSIDE, APART, NAN = 0, 1, 2  # the hand-placed probes at the head of every set; the last probe is infinite
FAR = 5000.0

_probes, _want = {}, {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def centre(box):
    return ((box[:3] + box[3:]) * F(0.5)).astype(F)


def probes(name):
    """The probe set of a scene (cached, read-only), 255 points: three hand-placed ones -- INSIDE a
    closed shape (mixed: the Cube's centre, a closed mesh; ties: the Monkey's box centre; soup: its box
    centre; nomodel: the second sphere's centre), APART from everything (ties, soup: 5,000 above the
    model, where no sample meets it; mixed, nomodel: 400 above the origin, over the floor and the Deer)
    and one with a NaN coordinate --, then the first 200 hit points and the first 51 inside points of
    test_gather_cpu.points(name) lifted 0.05 along their normals, then a point at infinity."""
    if name not in _probes:
        p, n = GC.points(name)
        keep = np.r_[0:N_HITS, GC.N_HITS:GC.N_HITS + N_INSIDE]
        lifted = (p[keep] + (n[keep] * LIFT).astype(F)).astype(F)
        bx = TR.boxes(name)
        inside = centre(bx[2] if name == "nomodel" else bx[1])
        if name in ("ties", "soup"):
            apart = centre(bx[0]) + np.array([0.0, FAR, 0.0], F)
        else:
            apart = np.array([0.0, 400.0, 0.0], F)
        q = np.concatenate([[inside, apart, [0.5, np.nan, -3.0]], lifted, [[np.inf, 0.0, -np.inf]]]).astype(F)
        assert len(q) == 255
        q.setflags(write=False)
        _probes[name] = q
    return _probes[name]


def want(name, ns, bl, first=0, base=0):
    """The reference's outputs on a scene's probe set (computed once, read-only)."""
    key = (name, ns, bl, first, base)
    if key not in _want:
        start = None
        if first:
            start = {"sum": np.zeros((255, 27), F), "ray_casts": np.zeros(255, np.uint32)}
        w = PR.probe_sh(TR.SCENES[name].oracle(), probes(name), ns, bl, SEED, first, base, start)
        for a in w.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _want[key] = w
    return _want[key]


def traced_of(w, bl, rows=slice(None)):
    """What the probes `rows` add to traced_rays: a sample traces its hits and, unless it ran to the
    limit, the segment that reached the sky."""
    sc = w["sample_casts"][rows]
    sc = sc[sc != PR.UNTRACED].astype(np.int64)
    return int((sc + (sc < bl)).sum())


# ---- the entry points ------------------------------------------------------------------------------------

def test_library_exports_the_probes():
    for name in ("atr_probe_sh", "atr_probe_directions", "atr_sh_basis"):
        assert name in E.EXPORTS and hasattr(E.lib(), name)
    for name in ("probe_directions", "sh_basis", "probe_grid", "sh_irradiance"):
        assert callable(getattr(E, name))
    assert callable(E.Engine.probe_sh)


def test_bindings():
    args, res = E.signatures()["atr_probe_sh"]
    assert len(args) == 11 and res is C.c_int
    assert args[2] is C.c_int64 and args[3] is C.c_int32 and args[4] is C.c_uint32 and args[5] is C.c_int64
    assert args[6] is C.c_int32 and args[7] is C.c_uint64 and args[9] is C.c_int32
    assert [f[0] for f in E.atr_probe_sh_out._fields_] == [
        "sh", "sum", "ray_casts", "invalid", "sample_rgb", "dirs", "traced_rays"]
    assert C.sizeof(E.atr_probe_sh_out) == 56
    args, res = E.signatures()["atr_probe_directions"]
    assert len(args) == 7 and res is C.c_int and args[0] is C.c_int64 and args[1] is C.c_int32
    assert args[2] is C.c_uint32 and args[3] is C.c_int64 and args[4] is C.c_uint64
    args, res = E.signatures()["atr_sh_basis"]
    assert len(args) == 3 and res is C.c_int and args[1] is C.c_int64


def test_null_context_is_invalid_without_a_device():
    f = E.lib().atr_probe_sh
    out = E.atr_probe_sh_out()
    assert f(None, None, 0, 1, 0, 0, 1, 0, C.byref(out), -1, None) == -1
    assert f(None, None, 5, 1, 0, 0, 1, 0, None, -1, None) == -1


def test_host_range_checks():
    g = E.lib().atr_probe_directions
    d, t = np.zeros((1, 4, 3), F), np.zeros((1, 4), np.uint8)
    p = lambda a: a.ctypes.data  # noqa: E731
    assert g(1, 4, 0, 0, 0, p(d), p(t)) == 0
    assert g(1, 4, 0, 0, 0, None, None) == 0 and g(0, 4, 0, 0, 0, None, None) == 0
    for npts, ns, first, base in ((1, 0, 0, 0), (1, -1, 0, 0), (1, 65537, 0, 0), (1, 4, 2 ** 24 - 3, 0), (1, 4, 0, -1),
                                  (1, 4, 0, 2 ** 32), (2, 4, 0, 2 ** 32 - 1), (-1, 4, 0, 0), (2 ** 31, 1, 0, 0),
                                  (2 ** 15, 65536, 0, 0)):
        assert g(npts, ns, first, base, 0, None, None) == -1, (npts, ns, first, base)
    assert g(1, 4, 2 ** 24 - 4, 2 ** 32 - 1, 0, p(d), p(t)) == 0  # both at their upper ends
    want_d, want_t = PR.directions(1, 4, 2 ** 24 - 4, 2 ** 32 - 1, 0)
    assert np.array_equal(bits(d), bits(want_d)) and np.array_equal(t, want_t)
    b = E.lib().atr_sh_basis
    y = np.zeros((4, 9), F)
    assert b(p(d), 4, p(y)) == 0 and b(None, 0, None) == 0
    assert b(p(d), -1, p(y)) == -1 and b(None, 4, p(y)) == -1 and b(p(d), 4, None) == -1
    with pytest.raises(ValueError):
        E.sh_basis(np.zeros((3, 2), F))
    with pytest.raises(ValueError):
        E.probe_grid((0, 0, 0), (1, 1, 1), (2, 0, 2))


# ---- the host sampler -------------------------------------------------------------------------------------

@pytest.mark.parametrize("first,base,seed", [(0, 0, 0), (5, 1000, SEED), (2 ** 24 - 40, 2 ** 32 - 9, 3)])
def test_directions_match_the_reference(first, base, seed):
    n, ns = 9, 40
    d, t = E.probe_directions(n, ns, first, base, seed)
    rd, rt = PR.directions(n, ns, first, base, seed)
    assert d.shape == (n, ns, 3) and t.shape == (n, ns) and t.dtype == np.uint8
    assert np.array_equal(bits(d), bits(rd)) and np.array_equal(t, rt)
    assert R.passes(np.zeros((n * ns, 3), F), d.reshape(-1, 3)).all()  # the 2^-20 test of a caller's ray
    assert t.min() >= 1 and t.max() <= 32 and (t > 1).any()


def test_directions_split_invariance():
    whole_d, whole_t = E.probe_directions(9, 100, 7, 50, SEED)
    for cut in (1, 4, 8):  # a probe cut
        a = E.probe_directions(cut, 100, 7, 50, SEED)
        b = E.probe_directions(9 - cut, 100, 7, 50 + cut, SEED)
        assert np.array_equal(bits(np.concatenate([a[0], b[0]])), bits(whole_d))
        assert np.array_equal(np.concatenate([a[1], b[1]]), whole_t)
    for cut in (1, 37, 64):  # a sample cut
        a = E.probe_directions(9, cut, 7, 50, SEED)
        b = E.probe_directions(9, 100 - cut, 7 + cut, 50, SEED)
        assert np.array_equal(bits(np.concatenate([a[0], b[0]], axis=1)), bits(whole_d))
        assert np.array_equal(np.concatenate([a[1], b[1]], axis=1), whole_t)


def test_sampler_statistics():
    """N = 2^16 samples. The basis is orthonormal over the sphere, so under the uniform density 1/(4 pi)
    Yk (k >= 1) has mean 0 and variance 1/(4 pi): its sample mean lies within 6 sqrt(1/(4 pi N)) of 0.
    A try is accepted with probability p = 0.5236 (the unit ball in the cube; the excluded core of
    radius 2^-5 takes 2^-15 of it), so tries is geometric with mean 1/p and variance (1 - p)/p^2 =
    1.738: its sample mean lies within 6 sqrt(1.738/N) of 1/0.5236."""
    n = 2 ** 16
    d, t = E.probe_directions(256, 256, 0, 0, SEED)
    y = E.sh_basis(d.reshape(-1, 3)).astype(np.float64)
    mean = y.mean(axis=0)
    bound = 6.0 * math.sqrt(1.0 / (4.0 * math.pi * n))
    print("mean Yk", np.round(mean, 5).tolist(), "bound", round(bound, 5))
    assert (np.abs(mean[1:]) <= bound).all(), mean
    tm = float(t.astype(np.float64).mean())
    tb = 6.0 * math.sqrt(1.738 / n)
    print("mean tries", tm, "expected", 1 / 0.5236, "bound", tb)
    assert abs(tm - 1.0 / 0.5236) <= tb
    assert t.max() <= 32


# ---- the basis ---------------------------------------------------------------------------------------------

def test_basis_matches_numpy():
    rng = np.random.default_rng(61)
    d = np.concatenate([R.random_dirs(1025, rng), E.probe_directions(4, 64, 0, 0, SEED)[0].reshape(-1, 3)])
    y = E.sh_basis(d)
    assert y.shape == (len(d), 9) and y.dtype == F
    assert np.array_equal(bits(y), bits(PR.np_basis(d)))
    assert E.sh_basis(d.reshape(-1, 3, 3)).shape == (len(d) // 3, 3, 9)


def test_basis_hand_worked():
    c0, c1, c2, c6, c8 = F(0.282094792), F(0.488602512), F(1.092548431), F(0.315391565), F(0.546274215)
    two = F(c6 * F(2.0))
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F)
    hand = np.array([
        # Y0  Y1   Y2   Y3   Y4 Y5 Y6    Y7 Y8
        [c0, 0, 0, c1, 0, 0, -c6, 0, c8],
        [c0, 0, 0, -c1, 0, 0, -c6, 0, c8],
        [c0, c1, 0, 0, 0, 0, -c6, 0, -c8],
        [c0, -c1, 0, 0, 0, 0, -c6, 0, -c8],
        [c0, 0, c1, 0, 0, 0, two, 0, 0],
        [c0, 0, -c1, 0, 0, 0, two, 0, 0]], F)
    assert np.array_equal(E.sh_basis(axes), hand)  # values; a zero's sign is free
    s = F(1.0) / np.sqrt(F(3.0))
    y = E.sh_basis(np.array([[s, s, s]], F))[0].astype(np.float64)
    want = [0.282094792, 0.488602512 / math.sqrt(3), 0.488602512 / math.sqrt(3), 0.488602512 / math.sqrt(3),
            1.092548431 / 3, 1.092548431 / 3, 0.0, 1.092548431 / 3, 0.0]
    assert np.abs(y - want).max() <= 2e-7, y  # a few f32 roundings of values below 0.5


def test_irradiance_of_a_constant_radiance_is_pi_times_it():
    """Radiance L from every direction projects on Y0 alone, sh[0] = L sqrt(4 pi); the cosine lobe turns
    it into pi L for every normal."""
    sh = np.zeros((9, 3), F)
    sh[0] = F(math.sqrt(4.0 * math.pi)) * np.array([0.5, 1.0, 2.0], F)
    nrm = R.random_dirs(17, np.random.default_rng(62))
    e = E.sh_irradiance(sh, nrm)
    assert e.shape == (17, 3)
    assert np.abs(e - math.pi * np.array([0.5, 1.0, 2.0])).max() <= 1e-5
    assert E.sh_irradiance(np.stack([sh, sh]), nrm).shape == (2, 17, 3)
    with pytest.raises(ValueError):
        E.sh_irradiance(np.zeros((27,), F), nrm)


def test_probe_grid():
    g = E.probe_grid((0, 10, -1), (1, 20, 1), (3, 2, 1))
    assert g.dtype == F and g.shape == (6, 3)
    assert g.tolist() == [[0, 10, 0], [0.5, 10, 0], [1, 10, 0], [0, 20, 0], [0.5, 20, 0], [1, 20, 0]]


# ---- the reference itself ---------------------------------------------------------------------------------

def test_reference_sums_are_the_numpy_restatement():
    for name, ns, bl in (("mixed", 7, 5), ("nomodel", 65, 2)):
        w = want(name, ns, bl)
        ok = w["invalid"] == 0
        s = PR.np_sums(w["sample_rgb"][ok], w["dirs"][ok])
        assert np.array_equal(bits(s), bits(w["sum"][ok])), name
        assert np.array_equal(bits(PR.np_sh(s, ns)), bits(w["sh"][ok])), name
        d, t = E.probe_directions(255, ns, 0, 0, SEED)
        assert np.array_equal(bits(d[ok]), bits(w["dirs"][ok])) and np.array_equal(t[ok], w["tries"][ok])
        assert w["traced"] == traced_of(w, bl)


def test_reference_is_split_invariant():
    sc = TR.SCENES["mixed"].oracle()
    p = probes("mixed")
    ns, bl, base = 7, 5, 1000
    w = want("mixed", ns, bl, 0, base)
    a = PR.probe_sh(sc, p[:100], ns, bl, SEED, 0, base)
    b = PR.probe_sh(sc, p[100:], ns, bl, SEED, 0, base + 100)
    for k in PER_PROBE + PER_SAMPLE:
        assert np.array_equal(bits(np.concatenate([a[k], b[k]])), bits(w[k])), k
    assert a["traced"] + b["traced"] == w["traced"]
    a = PR.probe_sh(sc, p, 3, bl, SEED, 0, base)
    b = PR.probe_sh(sc, p, 4, bl, SEED, 3, base, start=a)
    good = w["invalid"] == 0
    for k in ("sum", "ray_casts", "invalid"):
        assert np.array_equal(bits(b[k]), bits(w[k])), k
    assert np.array_equal(bits(b["sh"][good]), bits(w["sh"][good]))  # an invalid probe's is not written later
    for k in PER_SAMPLE:
        assert np.array_equal(bits(np.concatenate([a[k], b[k]], axis=1)), bits(w[k])), k
    assert a["traced"] + b["traced"] == w["traced"]
    assert not np.array_equal(bits(a["sum"][good]), bits(w["sum"][good]))  # the second range adds


def test_reference_reaches_the_fallback_with_one_try():
    sc = TR.SCENES["mixed"].oracle()
    p = probes("mixed")[:40]
    one = PR.probe_sh(sc, p, 33, 2, SEED, max_tries=1)
    full = PR.probe_sh(sc, p, 33, 2, SEED)
    good = one["invalid"] == 0
    fell = (one["tries"] == 2) & good[:, None]
    took = (one["tries"] == 1) & good[:, None]
    assert fell.sum() > 300 and took.sum() > 300 and (fell | took)[good].all()
    assert np.array_equal(one["dirs"][fell], np.broadcast_to(np.array([0, 0, 1], F), (int(fell.sum()), 3)))
    assert np.array_equal(took, (full["tries"] == 1) & good[:, None])
    assert np.array_equal(bits(one["dirs"][took]), bits(full["dirs"][took]))
    assert np.array_equal(bits(one["sample_rgb"][took]), bits(full["sample_rgb"][took]))
    assert np.array_equal(bits(PR.np_sums(one["sample_rgb"][good], one["dirs"][good])), bits(one["sum"][good]))
    assert (full["tries"][good] <= 32).all()


def test_reference_handles_invalid_probes():
    sc = TR.SCENES["mixed"].oracle()
    p = probes("mixed")[:40].copy()
    p[17] = -np.inf
    p[39, 2] = np.nan
    bad = [NAN, 17, 39]
    good = np.setdiff1d(np.arange(40), bad)
    w = PR.probe_sh(sc, p, 7, 5, SEED)
    assert w["invalid"].tolist() == [int(i in bad) for i in range(40)]
    for k in ("sh", "sum", "ray_casts", "sample_rgb", "dirs", "tries", "first_kind"):
        assert (bits(w[k][bad]) == 0).all(), k
    assert (w["sample_casts"][bad] == PR.UNTRACED).all()
    clean = want("mixed", 7, 5)
    for k in PER_PROBE + PER_SAMPLE:
        assert np.array_equal(bits(w[k][good]), bits(clean[k][good])), k
    rng = np.random.default_rng(4)
    start = {"sum": rng.uniform(0, 4, (40, 27)).astype(F), "ray_casts": rng.integers(0, 50, 40).astype(np.uint32)}
    m = PR.probe_sh(sc, p, 2, 5, SEED, 7, 0, start)
    for k in ("sum", "ray_casts"):
        assert np.array_equal(bits(m[k][bad]), bits(start[k][bad])), k
        assert not np.array_equal(bits(m[k][good]), bits(start[k][good])), k
    assert (bits(m["sh"][bad]) == PR.SENTINEL).all() and m["invalid"][bad].all()
    assert (bits(m["sample_rgb"][bad]) == 0).all() and (bits(m["dirs"][bad]) == 0).all()


# ---- the coverage conditions of the GPU probe sets --------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_gpu_probe_sets_reach_every_level_and_every_branch(name):
    """On the reference alone, for the sets and configurations of tests/test_gpu_probe_sh.py: every
    bounce level is reached in every configuration; first segments reach the sky and every kind of
    surface the scene has; the two non-finite probes are invalid and nothing else is; the INSIDE probe
    sees out of its closed mesh (mixed: no first hit on the Cube from its centre, which the culled
    triangle test lets through) or, in a sphere, nothing but that sphere (nomodel); the APART probe sees
    only sky where that can be (ties, soup -- over an infinite plane half the sphere is floor)."""
    sc = TR.SCENES[name]
    p = probes(name)
    for ns, bl in CONFIGS:
        w = want(name, ns, bl)
        casts = w["sample_casts"]
        levels = [int((casts == k).sum()) for k in range(bl + 1)]
        print(name, (ns, bl), "casts", levels)
        assert min(levels[1:]) >= 1, (ns, bl, levels)
        assert w["invalid"].tolist() == [int(i in (NAN, 254)) for i in range(255)]
        assert (w["tries"][w["invalid"] == 0] <= 32).all()  # no test reaches the fallback
    w = want(name, 129, 2)
    kind = w["first_kind"]
    count = {k: int((kind == k).sum()) for k in (PR.TRI, PR.SPHERE, PR.PLANE, PR.SKY)}
    print(name, "first segments", count)
    assert count[PR.SKY] >= 100
    assert (count[PR.TRI] >= 100) == bool(sc.names) and (count[PR.TRI] > 0) == bool(sc.names)
    assert (count[PR.SPHERE] >= 100) == bool(sc.spheres) and (count[PR.PLANE] >= 100) == bool(sc.planes)
    if name in ("ties", "soup"):
        assert (kind[APART] == PR.SKY).all() and (w["ray_casts"][APART] == 0)
    else:
        assert set(np.unique(kind[APART])) >= {PR.SKY, PR.PLANE}
    if name == "mixed":
        cube = sc.parts()[0]
        o = np.repeat(p[INSIDE][None], 129, axis=0)
        f_in = cube.trace(o, np.ascontiguousarray(w["dirs"][INSIDE]))[0]
        assert (f_in == R.MISS).all()  # out through the back faces
        lo, hi = TR.boxes(name)[1][:3], TR.boxes(name)[1][3:]
        assert (p[INSIDE] > lo).all() and (p[INSIDE] < hi).all()
        out = np.flatnonzero((kind[3:] == PR.TRI).any(axis=1))[:8] + 3  # probes outside do hit it
        hits = sum(int((cube.trace(np.repeat(p[i][None], 129, axis=0), np.ascontiguousarray(w["dirs"][i]))[0]
                        != R.MISS).sum()) for i in out)
        assert hits > 0
    if name == "nomodel":
        assert (kind[INSIDE] == PR.SPHERE).all()
