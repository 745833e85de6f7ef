"""atr_radiance_rays without a GPU: the symbol, its binding and the answers that need no device; the
reference of the GPU tests (tests/radiance_ref.py: the oracle's own cast_ray per (ray, sample)) and
camera_rays against the oracle's render, bit for bit; the coverage condition of every parity batch of
the GPU tests (asserted here on the reference alone, so those tests cannot pass vacuously); the
reference's split invariance. Also the ray batches the GPU tests share (batch)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import radiance_ref as RR  # noqa: E402
from tests import ray_sets as R  # noqa: E402
from tests import test_gpu_trace_rays as TR  # noqa: E402
from tests.test_gpu_scenes import MIXED, SOUP_SC  # noqa: E402

F = np.float32
SEED = 0x853C49E6748FEA9B
KINDS = {"aimed": 1025, "second": 257, "axis": 257, "inside": 257}  # the parity batches and their sizes
CONFIGS = ((1, 1), (2, 5), (7, 2), (64, 3))  # (nsamples, bounce_limit); 64 samples on the 257-ray batches only
POOL = 30000  # generator rays a batch is chosen from
PICK = (2, 5)  # the configuration whose levels the choice serves: the deepest, with the fewest paths

_batches, _want = {}, {}


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def configs(kind):
    return [c for c in CONFIGS if c[0] != 64 or KINDS[kind] == 257]


def pool(name, kind):
    """POOL rays of a batch's generator (tests/ray_sets.py, the seeds of tests/test_gpu_trace_rays.py)."""
    if kind == "aimed":
        return R.aimed(TR.boxes(name), POOL, 21)
    if kind == "second":
        ao, ad = R.aimed(TR.boxes(name), 2 * POOL, 21)
        return R.second_generation(ao, ad, TR.SCENES[name].oracle().trace(ao, ad)[1], 22, POOL)
    if kind == "axis":
        return R.axis(TR.boxes(name), POOL, 23)
    return R.inside(TR.focus(name), POOL, 24)


def batch(name, kind):
    """A parity batch (cached, read-only): (orig, dirs). The first rays of the generator as they come,
    except that positions are given to rays that take a path to a bounce level the batch still lacks
    (radiance_ref.pick on PICK's streams): few rays of a mostly convex scene bounce four times, and
    a 257-ray batch of the generator alone never shows 50 of them. To keep the choice quick, the rays
    past the batch's own are first thinned to those that bounce twice at all in a two-sample trial."""
    if (name, kind) not in _batches:
        sc, n = TR.SCENES[name].oracle(), KINDS[kind]
        po, pd = (np.ascontiguousarray(a, F) for a in pool(name, kind))
        assert len(po) == POOL and R.passes(po, pd).all()
        trial = RR.radiance(sc, po[n:], pd[n:], 2, PICK[1], seed=1)["sample_casts"]
        rich = n + np.flatnonzero((trial >= 2).any(axis=1))
        keep = np.concatenate([np.arange(n), rich])
        idx = keep[RR.pick(sc, po[keep], pd[keep], n, PICK[0], PICK[1], SEED)]
        o, d = np.ascontiguousarray(po[idx]), np.ascontiguousarray(pd[idx])
        o.setflags(write=False)
        d.setflags(write=False)
        _batches[name, kind] = (o, d)
    return _batches[name, kind]


def want(name, kind, ns, bl):
    """The reference's outputs of a parity batch (computed once, read-only)."""
    key = (name, kind, ns, bl)
    if key not in _want:
        w = RR.radiance(TR.SCENES[name].oracle(), *batch(name, kind), ns, bl, SEED)
        for a in w.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _want[key] = w
    return _want[key]


# ---- the entry point ------------------------------------------------------------------------------------

def test_library_exports_the_query():
    assert "atr_radiance_rays" in E.EXPORTS and hasattr(E.lib(), "atr_radiance_rays")
    assert callable(E.camera_rays) and callable(E.Engine.radiance_rays)


def test_binding():
    args, res = E.signatures()["atr_radiance_rays"]
    assert len(args) == 12 and res is C.c_int
    assert args[3] is C.c_int64 and args[4] is C.c_int32 and args[5] is C.c_uint32 and args[6] is C.c_int64
    assert args[7] is C.c_int32 and args[8] is C.c_uint64 and args[10] is C.c_int32
    assert [f[0] for f in E.atr_radiance_out._fields_] == ["rgb", "sum", "ray_casts", "invalid", "traced_rays"]
    assert C.sizeof(E.atr_radiance_out) == 40


def test_null_context_is_invalid_without_a_device():
    f = E.lib().atr_radiance_rays
    out = E.atr_radiance_out()
    assert f(None, None, None, 0, 1, 0, 0, 1, 0, C.byref(out), -1, None) == -1
    assert f(None, None, None, 5, 1, 0, 0, 1, 0, None, -1, None) == -1


# ---- camera_rays and the reference against the oracle's render ---------------------------------------

@pytest.mark.parametrize("sc,spp,bounces", [(MIXED, 2, 5), (MIXED, 7, 2), (SOUP_SC, 2, 5)],
                         ids=["mixed-2-5", "mixed-7-2", "soup-2-5"])
def test_reference_on_camera_rays_equals_the_oracle_render(sc, spp, bounces):
    W, H = 40, 24
    orig, dirs = E.camera_rays(E.camera(W, H, spp, bounces))
    assert orig.shape == dirs.shape == (W * H, 3) and orig.dtype == dirs.dtype == F
    assert R.passes(orig, dirs).all()
    rgb, _, casts, ctr = sc.oracle().render(O.Camera(W, H, spp=spp, bounces=bounces), SEED)
    r = RR.radiance(sc.oracle(), orig, dirs, spp, bounces, SEED)
    assert np.array_equal(bits(r["rgb"]), bits(rgb.reshape(-1, 3)))
    assert np.array_equal(r["ray_casts"], casts.reshape(-1))
    assert r["n_rays"] == ctr["n_rays"] and r["nvalid"] == W * H and not r["invalid"].any()
    assert (casts > 0).sum() >= 50 and (casts == 0).sum() >= 50  # hits and sky are both in view


def test_camera_rays_of_other_cameras():
    """An eye, a facing and an h_fov of its own, portrait: the first-hit outputs of the oracle's render
    of that camera are those of an oracle trace of camera_rays."""
    kw = dict(eye=(0.4, 1.0, 0.5), facing=(-0.2, -0.3, -1.0), h_fov=0.6)
    W, H = 24, 40
    orig, dirs = E.camera_rays(E.camera(W, H, **kw))
    face, t, _ = MIXED.oracle().primary_hits(O.Camera(W, H, **kw))
    f2, t2, _, _ = MIXED.oracle().trace(orig, dirs)
    assert np.array_equal(bits(t2), bits(t.reshape(-1))) and np.array_equal(f2, face.reshape(-1))


# ---- coverage of the GPU tests' parity batches -----------------------------------------------------------

@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("name", list(TR.SCENES))
def test_parity_batches_reach_every_bounce_level(name, kind):
    """At least 50 paths end at the sky after each of 1 .. bounce_limit - 1 bounces and at least 50 run
    to the limit, in every configuration of every batch -- also on `nomodel`, whose two spheres and
    plane do reach every level (asserted like the others). Sky first segments are there too."""
    o, d = batch(name, kind)
    assert o.shape == d.shape == (KINDS[kind], 3) and R.passes(o, d).all()
    for ns, bl in configs(kind):
        w = want(name, kind, ns, bl)
        h = np.bincount(w["sample_casts"].reshape(-1), minlength=bl + 1)
        print(name, kind, ns, bl, h.tolist())
        assert len(h) == bl + 1 and (h[1:] >= 50).all(), (name, kind, ns, bl, h.tolist())
        assert h[0] >= 5, (name, kind, ns, bl, h.tolist())  # the all-sky shortcut is exercised
        assert w["traced"] == w["n_rays"] - len(o) * (ns - 1) and not w["invalid"].any()


# ---- the reference's own split invariance --------------------------------------------------------------------

def test_reference_split_invariance():
    sc = TR.SCENES["mixed"].oracle()
    o, d = batch("mixed", "second")
    ns, bl, base = 7, 5, 1000
    whole = RR.radiance(sc, o, d, ns, bl, SEED, 0, base)
    for cut in (1, 100):  # a ray cut: ray_base advanced by the cut
        a = RR.radiance(sc, o[:cut], d[:cut], ns, bl, SEED, 0, base)
        b = RR.radiance(sc, o[cut:], d[cut:], ns, bl, SEED, 0, base + cut)
        for k in ("sum", "rgb"):
            assert np.array_equal(bits(np.concatenate([a[k], b[k]])), bits(whole[k])), (cut, k)
        assert np.array_equal(np.concatenate([a["ray_casts"], b["ray_casts"]]), whole["ray_casts"])
        assert a["traced"] + b["traced"] == whole["traced"]
    a = RR.radiance(sc, o, d, 3, bl, SEED, 0, base)  # a sample cut: continued through sum and ray_casts
    b = RR.radiance(sc, o, d, 4, bl, SEED, 3, base, sum=a["sum"], ray_casts=a["ray_casts"])
    for k in ("sum", "rgb"):
        assert np.array_equal(bits(b[k]), bits(whole[k])), k
    assert np.array_equal(b["ray_casts"], whole["ray_casts"])
    assert (bits(a["rgb"]) != bits(whole["rgb"])).any()  # the first part alone is another mean
    other = RR.radiance(sc, o, d, ns, bl, SEED, 0, base + 1)
    assert (bits(other["sum"]) != bits(whole["sum"])).any()  # the streams do depend on ray_base


def test_reference_leaves_invalid_rays_alone():
    sc = TR.SCENES["mixed"].oracle()
    o, d = (a[:6].copy() for a in batch("mixed", "second"))
    o[1, 2] = np.nan
    d[2] *= F(1.01)
    d[4] = 0
    r = RR.radiance(sc, o, d, 3, 2, SEED)
    bad = [1, 2, 4]
    assert r["invalid"].tolist() == [0, 1, 1, 0, 1, 0] and r["nvalid"] == 3
    assert (bits(r["rgb"][bad]) == 0).all() and (bits(r["sum"][bad]) == 0).all() and (r["ray_casts"][bad] == 0).all()
    solo = RR.radiance(sc, o[5:6], d[5:6], 3, 2, SEED, 0, 5)
    assert np.array_equal(bits(r["sum"][5:6]), bits(solo["sum"]))
    more = RR.radiance(sc, o, d, 2, 2, SEED, 3, sum=r["sum"], ray_casts=r["ray_casts"])
    assert (bits(more["sum"][bad]) == 0).all() and (bits(more["rgb"][bad]) == RR.SENTINEL).all()
