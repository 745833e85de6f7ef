"""atr_radiance_rays on the GPU: every output (sum, rgb, ray_casts, invalid, traced_rays) for exact
equality with the reference of tests/radiance_ref.py (the oracle's own cast_ray per (ray, sample);
validated without a GPU in tests/test_radiance_cpu.py, which also asserts that the batches used here
reach every bounce level): every scene, batch, sample count, bounce limit and queue order; wave and
group tails; many batches; the render itself on the camera's rays; split invariance; invalid rays;
partial outputs; streams; arguments; the render paths after a call. Every buffer is filled with a
sentinel first and guarded on both sides. Needs an MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from tests import radiance_ref as RR  # noqa: E402
from tests import test_gpu_trace_rays as TR  # noqa: E402
from tests import test_radiance_cpu as RC  # noqa: E402
from tests.test_gpu_parity import eng, run  # noqa: E402,F401
from tests.test_gpu_scenes import MIXED, SOUP_SC, W as SW, H as SH, ref, same as same_render  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SEED = RC.SEED
ALL = ("rgb", "sum", "ray_casts", "invalid")
PER = {"rgb": 12, "sum": 12, "ray_casts": 4, "invalid": 1}  # bytes per ray
G = 256  # guard bytes around every output buffer
FILL = 0xAB


def dev():
    return torch.device("cuda", 0)


class Bufs:
    """The four output buffers of n rays with G guard bytes on both sides, filled with 0xAB, and the
    traced-ray accumulator, started at 5."""

    def __init__(self, n):
        self.n = n
        self.buf = {k: torch.full((n * PER[k] + 2 * G,), FILL, dtype=torch.uint8, device=dev()) for k in ALL}
        self.traced = torch.full((1,), 5, dtype=torch.int64, device=dev())

    def ptr(self, k):
        return self.buf[k].data_ptr() + G

    def out(self, names=ALL, traced=True):
        return E.atr_radiance_out(*[self.ptr(k) if k in names else None for k in ALL],
                                  self.traced.data_ptr() if traced else None)

    def put(self, k, a):
        """Start values (sum, ray_casts of an earlier range)."""
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.buf[k][G:G + len(raw)] = torch.from_numpy(raw.copy()).to(dev())

    def get(self, k):
        a = self.buf[k].cpu().numpy()
        n = self.n * PER[k]
        assert (a[:G] == FILL).all() and (a[G + n:] == FILL).all(), (k, "guard bytes")
        a = a[G:G + n].copy()
        if k == "invalid":
            return a
        return a.view(np.uint32).reshape((self.n, 3) if PER[k] == 12 else (self.n,))


def raw_call(eng, o, d, n, ns, bl, out, first=0, base=0, seed=SEED, sort_bits=-1, stream=None):
    q = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None  # noqa: E731
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    return E.lib().atr_radiance_rays(eng.h, q(o), q(d), n, ns, first, base, bl, C.c_uint64(seed),
                                     C.byref(out) if out is not None else None, sort_bits,
                                     C.c_void_p(stream) if stream else None)


def radiance(eng, orig, dirs, ns, bl, first=0, base=0, seed=SEED, sort_bits=-1, start=None, stream=None, wait=True):
    """One call with all outputs into guarded buffers: {name: uint32 bits (invalid: bytes)} and the
    traced count. start: the earlier range's outputs when first > 0."""
    o = torch.from_numpy(np.array(orig, F)).to(dev())  # copies: the cached batches are read-only
    d = torch.from_numpy(np.array(dirs, F)).to(dev())
    b = Bufs(len(orig))
    if start is not None:
        b.put("sum", start["sum"])
        b.put("ray_casts", start["ray_casts"])
    torch.cuda.current_stream().synchronize()  # the fills and copies above, ahead of a call on another stream
    assert raw_call(eng, o, d, len(orig), ns, bl, b.out(), first, base, seed, sort_bits, stream) == 0
    if not wait:
        return b, (o, d)
    rc, done = eng.wait()
    assert rc == 0 and done == 0, (rc, done)
    torch.cuda.synchronize()
    return host(b)


def host(b):
    res = {k: b.get(k) for k in ALL}
    res["traced"] = int(b.traced.item()) - 5
    return res


def same(got, w, what, rows=slice(None), traced=True):
    for k in ALL:
        want = w[k][rows] if k == "invalid" else np.ascontiguousarray(w[k][rows]).view(np.uint32)
        bad = np.flatnonzero((got[k] != want).reshape(len(want), -1).any(axis=1))
        assert len(bad) == 0, (what, k, len(bad), bad[:6].tolist(), got[k][bad[:6]].tolist(), want[bad[:6]].tolist())
    if traced:
        assert got["traced"] == w["traced"], (what, "traced", got["traced"], w["traced"])


# ---- 1. parity -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", list(RC.KINDS))
@pytest.mark.parametrize("name", list(TR.SCENES))
def test_parity_with_reference(eng, name, kind):
    o, d = RC.batch(name, kind)
    TR.SCENES[name].upload(eng)
    for ns, bl in RC.configs(kind):
        w = RC.want(name, kind, ns, bl)
        for sb in (0, 5):
            same(radiance(eng, o, d, ns, bl, sort_bits=sb), w, (name, kind, ns, bl, sb))


# ---- 2. tails ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("ns", [1, 7])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_parity_at_wave_and_group_tails(eng, n, ns):
    MIXED.upload(eng)
    o, d = (a[:n] for a in RC.batch("mixed", "second"))
    w = RR.radiance(MIXED.oracle(), o, d, ns, 5, SEED)
    for sb in (0, 5, -1):
        same(radiance(eng, o, d, ns, 5, sort_bits=sb), w, (n, ns, sb))


# ---- 3. many batches -----------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,n,ns,bl", [("aimed", 1025, 7, 5), ("second", 65, 64, 3)])
def test_small_batches_change_no_output(eng, kind, n, ns, bl):
    MIXED.upload(eng)
    o, d = (a[:n] for a in RC.batch("mixed", kind))
    w = RR.radiance(MIXED.oracle(), o, d, ns, bl, SEED)
    base = eng.tuning()
    whole = radiance(eng, o, d, ns, bl)
    same(whole, w, (kind, "default tuning"))
    try:
        eng.set_tuning(path_batch_log2=12)
        groups, per_batch = (n + 63) // 64, max(1, 4096 // (64 * ns))
        if kind == "aimed":
            assert groups > per_batch  # 17 groups of 448 paths, 9 to a batch
        for sb in (0, 5):
            got = radiance(eng, o, d, ns, bl, sort_bits=sb)
            same(got, w, (kind, "2^12-path batches", sb))
            for k in ALL:
                assert np.array_equal(got[k], whole[k]), (kind, sb, k)
    finally:
        eng.set_tuning(**base)


# ---- 4. the render ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("sc,spp,bl", [(MIXED, 2, 5), (SOUP_SC, 7, 2)], ids=["mixed", "soup"])
def test_camera_rays_give_the_render(eng, sc, spp, bl):
    """rgb and ray_casts of atr_render_start_ex (AUTO, IMAGE), bit for bit. With one sample and one
    bounce, the rays whose ray_casts is 0 are the render's misses: its hit_face misses on `soup`; on
    `mixed`, whose sphere and plane are hit with no face, the pixels whose hit_t is the miss record's
    (there a ray_casts of 0 also implies a hit_face miss)."""
    W, H = 64, 40
    sc.upload(eng)
    orig, dirs = E.camera_rays(E.camera(W, H, spp, bl))
    r = run(eng, E.camera(W, H, spp, bl))
    for sb in (0, -1):
        got = radiance(eng, orig, dirs, spp, bl, sort_bits=sb)
        assert np.array_equal(got["rgb"], r["rgb"].reshape(-1, 3).view(np.uint32)), sb
        assert np.array_equal(got["ray_casts"], r["casts"].reshape(-1)), sb
        assert not got["invalid"].any()
    r1 = run(eng, E.camera(W, H, 1, 1))
    got = radiance(eng, orig, dirs, 1, 1)
    sky = got["ray_casts"] == 0
    miss_face, miss_t = r1["face"].reshape(-1) == E.MISS, r1["t"].reshape(-1) == E.MAX_FLOAT
    assert 50 <= sky.sum() <= W * H - 50
    assert np.array_equal(sky, miss_t) and not (sky & ~miss_face).any()
    if sc is SOUP_SC:
        assert np.array_equal(sky, miss_face)
    assert np.array_equal(got["rgb"], r1["rgb"].reshape(-1, 3).view(np.uint32))
    assert got["traced"] == r1["traced"] == W * H


# ---- 5. split invariance -------------------------------------------------------------------------------

def test_split_invariance(eng):
    MIXED.upload(eng)
    o, d = RC.batch("mixed", "second")
    ns, bl, base = 7, 5, 1000
    w = RR.radiance(MIXED.oracle(), o, d, ns, bl, SEED, 0, base)
    for sb in (0, 5):
        same(radiance(eng, o, d, ns, bl, 0, base, sort_bits=sb), w, ("ray_base", sb))
        a = radiance(eng, o[:100], d[:100], ns, bl, 0, base, sort_bits=sb)  # cut at ray 100
        b = radiance(eng, o[100:], d[100:], ns, bl, 0, base + 100, sort_bits=sb)
        same(a, w, ("head", sb), slice(0, 100), traced=False)
        same(b, w, ("tail", sb), slice(100, None), traced=False)
        assert a["traced"] + b["traced"] == w["traced"]
        a = radiance(eng, o, d, 3, bl, 0, base, sort_bits=sb)  # samples [0, 3) then [3, 7) through sum
        wa = RR.radiance(MIXED.oracle(), o, d, 3, bl, SEED, 0, base)
        same(a, wa, ("samples 0-2", sb))
        b = radiance(eng, o, d, 4, bl, 3, base, sort_bits=sb, start=a)
        same(b, w, ("samples 3-6", sb), traced=False)
        assert a["traced"] + b["traced"] == w["traced"] + len(o)  # the first segment once per call
    # first_sample > 0 against the reference's own continuation, from start values of no earlier call
    rng = np.random.default_rng(3)
    start = {"sum": rng.uniform(0, 4, (len(o), 3)).astype(F), "ray_casts": rng.integers(0, 50, len(o)).astype(np.uint32)}
    wc = RR.radiance(MIXED.oracle(), o, d, 5, 3, SEED, 11, base, sum=start["sum"], ray_casts=start["ray_casts"])
    same(radiance(eng, o, d, 5, 3, 11, base, start=start), wc, "first_sample 11")


# ---- 6. invalid rays -------------------------------------------------------------------------------------

def test_invalid_rays_sit_between_valid_ones(eng):
    MIXED.upload(eng)
    o, d = (a[:130].copy() for a in RC.batch("mixed", "second"))
    clean_o, clean_d = o.copy(), d.copy()
    o[0, 1] = np.nan
    o[31] = np.inf
    d[63] = 0
    d[64] *= F(1.01)
    bad = [0, 31, 63, 64]
    good = np.setdiff1d(np.arange(130), bad)
    for ns, bl in ((1, 1), (7, 5)):
        w = RR.radiance(MIXED.oracle(), o, d, ns, bl, SEED)
        assert w["invalid"][bad].all() and w["nvalid"] == 126
        got = radiance(eng, o, d, ns, bl)
        same(got, w, (ns, bl))
        assert got["invalid"].tolist() == [int(i in bad) for i in range(130)]
        for k in ("rgb", "sum", "ray_casts"):
            assert (got[k][bad] == 0).all(), k
        clean = radiance(eng, clean_o, clean_d, ns, bl)  # the neighbours: a run without the bad rays
        for k in ALL:
            assert np.array_equal(got[k][good], clean[k][good]), k
        assert got["traced"] < clean["traced"] and got["traced"] == w["traced"]
        # a later range leaves an invalid ray's sum and ray_casts (and its rgb) as they are
        more = radiance(eng, o, d, 2, bl, ns, start=got)
        wm = RR.radiance(MIXED.oracle(), o, d, 2, bl, SEED, ns, sum=w["sum"], ray_casts=w["ray_casts"])
        for k in ("sum", "ray_casts"):
            assert (more[k][bad] == 0).all() and np.array_equal(more[k], np.ascontiguousarray(wm[k]).view(np.uint32)), k
        assert (more["rgb"][bad] == 0xABABABAB).all() and more["invalid"][bad].all()
        assert np.array_equal(more["rgb"][good], wm["rgb"].view(np.uint32)[good])


# ---- 7. partial outputs --------------------------------------------------------------------------------------

def test_only_the_requested_outputs_are_written(eng):
    MIXED.upload(eng)
    n, ns, bl = 70, 7, 3
    on, dn = (a[:n].copy() for a in RC.batch("mixed", "second"))
    dn[5] = 0  # an invalid ray among them: its zeros are written under the same rule
    w = RR.radiance(MIXED.oracle(), on, dn, ns, bl, SEED)
    o, d = torch.from_numpy(on).to(dev()), torch.from_numpy(dn).to(dev())
    calls = 0
    for names, traced in [((k,), False) for k in ALL] + [((), True), (ALL, True), (("rgb", "invalid"), True)]:
        b = Bufs(n)
        assert raw_call(eng, o, d, n, ns, bl, b.out(names, traced)) == 0
        assert eng.wait() == (0, 0)
        torch.cuda.synchronize()
        calls += 1
        for k in ALL:
            got = b.get(k)
            if k in names:
                want = w[k] if k == "invalid" else np.ascontiguousarray(w[k]).view(np.uint32)
                assert np.array_equal(got, want), (names, k)
            else:
                assert (got.view(np.uint8) == FILL).all(), (names, k)
        assert int(b.traced.item()) == 5 + (w["traced"] if traced else 0), names  # one accumulator, added to
    assert calls == 7


# ---- 8. streams ------------------------------------------------------------------------------------------------

def test_two_streams_without_a_wait_between(eng):
    MIXED.upload(eng)
    o, d = RC.batch("mixed", "aimed")
    s1, s2 = torch.cuda.Stream(dev()), torch.cuda.Stream(dev())
    torch.cuda.synchronize()
    a = radiance(eng, o, d, 7, 2, stream=s1.cuda_stream, wait=False)
    b = radiance(eng, o, d, 2, 5, stream=s2.cuda_stream, wait=False)  # takes over or opens a workspace
    c = radiance(eng, o, d, 1, 1, stream=s1.cuda_stream, wait=False)
    rc, done = eng.wait()
    assert (rc, done) == (0, 0) and eng.last_kernel_ms() > 0
    torch.cuda.synchronize()
    same(host(a[0]), RC.want("mixed", "aimed", 7, 2), "stream 1")
    same(host(b[0]), RC.want("mixed", "aimed", 2, 5), "stream 2")
    same(host(c[0]), RC.want("mixed", "aimed", 1, 1), "stream 1 again")
    assert 1 <= eng.workspace_info()["workspaces"] <= 4


# ---- 9. arguments ------------------------------------------------------------------------------------------------

def test_arguments(eng):
    MIXED.upload(eng)
    n, ns, bl = 9, 3, 2
    on, dn = (a[:n] for a in RC.batch("mixed", "second"))
    o, d = torch.from_numpy(on.copy()).to(dev()), torch.from_numpy(dn.copy()).to(dev())
    b = Bufs(n)
    out, inv = b.out(), -1
    assert raw_call(eng, o, d, n, ns, bl, None) == inv
    assert raw_call(eng, None, d, n, ns, bl, out) == inv
    assert raw_call(eng, o, None, n, ns, bl, out) == inv
    assert raw_call(eng, o, d, -1, ns, bl, out) == inv
    assert raw_call(eng, o, d, 2 ** 31, ns, bl, out) == inv
    for bad_ns in (0, -1, 65537):
        assert raw_call(eng, o, d, n, bad_ns, bl, out) == inv
    assert raw_call(eng, o, d, n, ns, bl, out, first=2 ** 24 - ns + 1) == inv
    assert raw_call(eng, o, d, n, ns, bl, out, base=-1) == inv
    assert raw_call(eng, o, d, n, ns, bl, out, base=2 ** 32 - n + 1) == inv
    for bad_bl in (0, -1, 65):
        assert raw_call(eng, o, d, n, ns, bad_bl, out) == inv
    for bad_sb in (-2, 1, 8):
        assert raw_call(eng, o, d, n, ns, bl, out, sort_bits=bad_sb) == inv
    assert raw_call(eng, o, d, n, ns, bl, b.out(("rgb", "ray_casts", "invalid")), first=1) == inv  # no sum
    assert raw_call(eng, o, d, n, ns, bl, b.out((), False)) == inv  # nothing to write
    assert raw_call(eng, o, d, 0, ns, bl, out) == 0 and raw_call(eng, None, None, 0, ns, bl, None) == 0
    torch.cuda.synchronize()
    for k in ALL:
        assert (b.get(k).view(np.uint8) == FILL).all()
    assert int(b.traced.item()) == 5  # nothing was written
    # the ranges at their upper ends
    start = {"sum": np.zeros((n, 3), F), "ray_casts": np.zeros(n, np.uint32)}
    w = RR.radiance(MIXED.oracle(), on, dn, ns, 64, SEED, 2 ** 24 - ns, 2 ** 32 - n, sum=start["sum"],
                    ray_casts=start["ray_casts"])
    for sb in (0, 2, 7):
        same(radiance(eng, on, dn, ns, 64, 2 ** 24 - ns, 2 ** 32 - n, sort_bits=sb, start=start), w, ("upper ends", sb))
    with pytest.raises(ValueError):
        eng.radiance_rays(o.t().contiguous().t(), d, ns, bl)  # not contiguous
    with pytest.raises(ValueError):
        eng.radiance_rays(o.double(), d, ns, bl)
    with pytest.raises(ValueError):
        eng.radiance_rays(o, d[:-1], ns, bl)
    with pytest.raises(ValueError):
        eng.radiance_rays(o, d, ns, bl, want=("rgb", "hits"))
    with pytest.raises(ValueError):
        eng.radiance_rays(o, d, ns, bl, first_sample=3)  # no sum to continue
    fresh = E.Engine(0)
    try:
        assert raw_call(fresh, o, d, n, ns, bl, out) == -4  # ATR_E_NOSCENE
    finally:
        fresh.close()


def test_engine_method(eng):
    """Engine.radiance_rays: the default outputs, and a sample range continued through sum."""
    MIXED.upload(eng)
    on, dn = RC.batch("mixed", "second")
    o, d = torch.from_numpy(on.copy()).to(dev()), torch.from_numpy(dn.copy()).to(dev())
    w = RC.want("mixed", "second", 7, 2)
    out, traced = eng.radiance_rays(o, d, 7, 2, seed=SEED)
    assert eng.wait() == (0, 0)
    torch.cuda.synchronize()
    assert sorted(out) == ["invalid", "ray_casts", "rgb"]
    assert np.array_equal(out["rgb"].cpu().numpy().view(np.uint32), w["rgb"].view(np.uint32))
    assert np.array_equal(out["ray_casts"].cpu().numpy().view(np.uint32), w["ray_casts"])
    assert not out["invalid"].cpu().numpy().any() and int(traced.item()) == w["traced"]
    a, _ = eng.radiance_rays(o, d, 3, 2, seed=SEED, want=("sum", "ray_casts"))
    b, _ = eng.radiance_rays(o, d, 4, 2, seed=SEED, first_sample=3, sum=a["sum"], ray_casts=a["ray_casts"],
                             want=("rgb",))
    assert eng.wait() == (0, 0)
    torch.cuda.synchronize()
    assert b["sum"] is a["sum"] and np.array_equal(b["sum"].cpu().numpy().view(np.uint32), w["sum"].view(np.uint32))
    assert np.array_equal(b["rgb"].cpu().numpy().view(np.uint32), w["rgb"].view(np.uint32))
    assert np.array_equal(b["ray_casts"].cpu().numpy().view(np.uint32), w["ray_casts"])


# ---- 10. the render paths after a call ------------------------------------------------------------------------

def test_wait_timing_and_a_render_right_after(eng):
    """atr_render_wait reports no tiles for the call and atr_last_kernel_ms times it; a render issued
    right after it on the same stream, with no wait between, takes the workspace over and still equals
    the oracle's."""
    MIXED.upload(eng)
    o, d = RC.batch("mixed", "aimed")
    b, keep = radiance(eng, o, d, 7, 2, wait=False)
    r = run(eng, E.camera(SW, SH, 2, 5))  # its own wait covers the render: one tile
    same_render(r, ref(MIXED, SW, SH, 2, 5), "render after a radiance call")
    same(host(b), RC.want("mixed", "aimed", 7, 2), "the call before the render")
    got = radiance(eng, o, d, 2, 5)
    ms = eng.last_kernel_ms()
    assert 0 < ms < 10000
    assert eng.wait() == (0, 0)  # tiles_done 0 after a radiance call
    same(got, RC.want("mixed", "aimed", 2, 5), "after the render")
    assert 1 <= eng.workspace_info()["workspaces"] <= 4
