"""atr_gather_radiance without a GPU: the symbol, its binding and the NULL-context answer; the reference
of the GPU tests (tests/gather_radiance_ref.py: the gather's direction, then the oracle's own cast_ray on
the same stream) against the host sampler, against the occlusion gather's reference and against itself
cut by points and by samples; and the coverage conditions of the GPU tests' batches, asserted here on
the reference alone, so a parity test cannot pass on paths that never bounce. Also the reference
outputs the GPU tests share (want)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from tests import gather_radiance_ref as GRR  # noqa: E402
from tests import gather_ref as GR  # noqa: E402
from tests import test_gather_cpu as GC  # noqa: E402
from tests import test_gpu_trace_rays as TR  # noqa: E402

F = np.float32
SEED = GC.SEED
NAMES = ("mixed", "ties", "soup", "nomodel")
CONFIGS = ((1, 1), (7, 5), (64, 3), (100, 2))  # (nsamples, bounce_limit) of the GPU parity test
PER_POINT = ("rgb", "sum", "samples", "ray_casts", "invalid")
PER_SAMPLE = ("sample_rgb", "dirs")

_want = {}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == F else a


def want(name, ns, bl, first=0, base=0):
    """The reference's outputs on a scene's point set (computed once, read-only)."""
    key = (name, ns, bl, first, base)
    if key not in _want:
        w = GRR.gather_radiance(TR.SCENES[name].oracle(), *GC.points(name), ns, bl, SEED, first, base)
        for a in w.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _want[key] = w
    return _want[key]


# ---- the entry point ------------------------------------------------------------------------------------

def test_library_exports_the_gather():
    assert "atr_gather_radiance" in E.EXPORTS and hasattr(E.lib(), "atr_gather_radiance")
    assert callable(E.Engine.gather_radiance)


def test_binding():
    args, res = E.signatures()["atr_gather_radiance"]
    assert len(args) == 12 and res is C.c_int
    assert args[3] is C.c_int64 and args[4] is C.c_int32 and args[5] is C.c_uint32 and args[6] is C.c_int64
    assert args[7] is C.c_int32 and args[8] is C.c_uint64 and args[10] is C.c_int32
    assert [f[0] for f in E.atr_gather_radiance_out._fields_] == [
        "rgb", "sum", "samples", "ray_casts", "invalid", "sample_rgb", "dirs", "traced_rays"]
    assert C.sizeof(E.atr_gather_radiance_out) == 64


def test_null_context_is_invalid_without_a_device():
    f = E.lib().atr_gather_radiance
    out = E.atr_gather_radiance_out()
    assert f(None, None, None, 0, 1, 0, 0, 1, 0, C.byref(out), -1, None) == -1
    assert f(None, None, None, 5, 1, 0, 0, 1, 0, None, -1, None) == -1


# ---- the reference against the sampler and the occlusion gather ------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_reference_directions_and_flags_are_the_samplers(name):
    _, n = GC.points(name)
    for ns, bl, first, base in ((7, 5, 0, 0), (33, 1, 5, 1000)):
        start = None
        if first:
            start = {"sum": np.zeros((len(n), 3), F), "samples": np.zeros(len(n), np.uint32)}
            w = GRR.gather_radiance(TR.SCENES[name].oracle(), *GC.points(name), ns, bl, SEED, first, base, start)
        else:
            w = want(name, ns, bl)
        d, t = E.gather_directions(n, ns, first, base, SEED)
        assert np.array_equal(bits(w["dirs"]), bits(d)) and np.array_equal(w["flags"], t)
        assert np.array_equal(w["samples"], t.sum(axis=1).astype(np.uint32))
        assert (w["sample_casts"][t == 0] == GRR.UNTRACED).all() and (w["sample_casts"][t == 1] <= bl).all()
        assert (bits(w["sample_rgb"])[t == 0] == 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_reference_with_one_bounce_counts_what_the_occlusion_gather_counts(name):
    """Consequence 1 on the references: samples == visible + occluded, and with bounce_limit 1 a traced
    sample casts 1 iff it hits anything, which an unbounded occlusion query answers too."""
    sc = TR.SCENES[name].oracle()
    p, n = GC.points(name)
    ns, first, base = 33, 5, 1000
    start = {"sum": np.zeros((len(p), 3), F), "samples": np.zeros(len(p), np.uint32)}
    w = GRR.gather_radiance(sc, p, n, ns, 1, SEED, first, base, start)
    g = GR.gather(sc, p, n, ns, None, first, base, SEED)
    assert np.array_equal(w["samples"], g["visible"] + g["occluded"])
    assert np.array_equal(w["ray_casts"], g["occluded"])
    assert w["traced"] == g["traced"] and g["occluded"].sum() > 0 and g["visible"].sum() > 0


def test_reference_is_split_invariant():
    sc = TR.SCENES["mixed"].oracle()
    p, n = GC.points("mixed")
    ns, bl, base = 7, 5, 1000
    w = want("mixed", ns, bl, 0, base)
    a = GRR.gather_radiance(sc, p[:100], n[:100], ns, bl, SEED, 0, base)
    b = GRR.gather_radiance(sc, p[100:], n[100:], ns, bl, SEED, 0, base + 100)
    for k in PER_POINT + PER_SAMPLE:
        assert np.array_equal(bits(np.concatenate([a[k], b[k]])), bits(w[k])), k
    assert a["traced"] + b["traced"] == w["traced"]
    a = GRR.gather_radiance(sc, p, n, 3, bl, SEED, 0, base)
    b = GRR.gather_radiance(sc, p, n, 4, bl, SEED, 3, base, start=a)
    for k in PER_POINT:
        assert np.array_equal(bits(b[k]), bits(w[k])), k
    for k in PER_SAMPLE:
        assert np.array_equal(bits(np.concatenate([a[k], b[k]], axis=1)), bits(w[k])), k
    assert a["traced"] + b["traced"] == w["traced"]
    assert (a["samples"] < w["samples"]).any()  # the second range adds samples: the divisor moves


def test_reference_leaves_invalid_points_alone_after_the_first_range():
    sc = TR.SCENES["mixed"].oracle()
    p, n = (a[:40].copy() for a in GC.points("mixed"))
    p[3, 1] = np.nan
    p[17] = np.inf
    n[20] = 0
    n[39] *= F(1.001)
    bad = [3, 17, 20, 39]
    good = np.setdiff1d(np.arange(40), bad)
    w = GRR.gather_radiance(sc, p, n, 7, 5, SEED)
    assert w["invalid"].tolist() == [int(i in bad) for i in range(40)]
    for k in ("rgb", "sum", "samples", "ray_casts", "sample_rgb", "dirs", "flags"):
        assert (bits(w[k][bad]) == 0).all(), k
    assert (w["sample_casts"][bad] == GRR.UNTRACED).all()
    clean = want("mixed", 7, 5)
    for k in PER_POINT + PER_SAMPLE:
        assert np.array_equal(bits(w[k][good]), bits(clean[k][good])), k
    rng = np.random.default_rng(4)
    start = {"sum": rng.uniform(0, 4, (40, 3)).astype(F), "samples": rng.integers(0, 9, 40).astype(np.uint32),
             "ray_casts": rng.integers(0, 50, 40).astype(np.uint32)}
    m = GRR.gather_radiance(sc, p, n, 2, 5, SEED, 7, 0, start)
    for k in ("sum", "samples", "ray_casts"):
        assert np.array_equal(bits(m[k][bad]), bits(start[k][bad])), k
        assert not np.array_equal(bits(m[k][good]), bits(start[k][good])), k
    assert (bits(m["rgb"][bad]) == GRR.SENTINEL).all() and m["invalid"][bad].all()
    assert (bits(m["sample_rgb"][bad]) == 0).all() and (bits(m["dirs"][bad]) == 0).all()


# ---- the coverage conditions of the GPU batches ----------------------------------------------------------

def level_counts(w, bl):
    sc = w["sample_casts"]
    return [int((sc == k).sum()) for k in range(bl + 1)]


@pytest.mark.parametrize("name", NAMES)
def test_gpu_batches_reach_every_level_and_every_branch(name):
    p, _ = GC.points(name)
    assert len(p) == 322
    w75, w643, w11 = want(name, 7, 5), want(name, 64, 3), want(name, 1, 1)
    c75, c643 = level_counts(w75, 5), level_counts(w643, 3)
    untraced = int((w75["flags"] == 0).sum())
    empty = int((w11["samples"] == 0).sum())
    print(name, "casts at (7, 5)", c75, "untraced", untraced, "casts at (64, 3)", c643,
          "points without a sample at (1, 1)", empty)
    if name in ("mixed", "soup"):
        assert min(c75) >= 16, c75
    assert min(c643) >= 16, c643
    assert untraced >= 30
    assert empty >= 5 and (bits(w11["rgb"])[w11["samples"] == 0] == 0).all()
    assert not w75["invalid"].any()
