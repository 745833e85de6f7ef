"""atr_gather_radiance on the GPU: every output (rgb, sum, samples, ray_casts, invalid, sample_rgb, dirs,
traced_rays) for exact equality with the reference of tests/gather_radiance_ref.py (the gather's
direction, then the oracle's own cast_ray on the same stream; validated without a GPU in
tests/test_gather_radiance_cpu.py, which also asserts that the batches used here reach every bounce
level, hold untraced samples and hold points without a traced sample): every scene, sample count,
bounce limit and queue order; wave, point and row tails; many batches and a point larger than a batch;
the occlusion gather's counts; split invariance; invalid points; partial outputs and arguments;
streams and the render paths after a call. Every buffer is filled with a sentinel first and guarded on
both sides. Needs an MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from tests import gather_radiance_ref as GRR  # noqa: E402
from tests import test_gather_radiance_cpu as GC  # noqa: E402
from tests import test_gpu_trace_rays as TR  # noqa: E402
from tests import test_radiance_cpu as RC  # noqa: E402
from tests.test_gather_cpu import points  # noqa: E402
from tests.test_gpu_parity import eng, run  # noqa: E402,F401
from tests.test_gpu_scenes import MIXED, W as SW, H as SH, ref, same as same_render  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SEED = GC.SEED
POINT = ("rgb", "sum", "samples", "ray_casts", "invalid")
SAMPLE = ("sample_rgb", "dirs")
ALL = POINT + SAMPLE  # atr_gather_radiance_out's order
PER = {"rgb": 12, "sum": 12, "samples": 4, "ray_casts": 4, "invalid": 1}  # bytes per point
G = 256  # guard bytes around every output buffer
FILL = 0xAB


def dev():
    return torch.device("cuda", 0)


class Bufs:
    """The seven output buffers of n points x ns samples with G guard bytes on both sides, filled with
    0xAB, and the traced-ray accumulator, started at 5."""

    def __init__(self, n, ns):
        self.n, self.ns = n, ns
        self.size = {k: n * PER[k] if k in PER else n * ns * 12 for k in ALL}
        self.buf = {k: torch.full((self.size[k] + 2 * G,), FILL, dtype=torch.uint8, device=dev()) for k in ALL}
        self.traced = torch.full((1,), 5, dtype=torch.int64, device=dev())

    def ptr(self, k):
        return self.buf[k].data_ptr() + G

    def out(self, names=ALL, traced=True):
        return E.atr_gather_radiance_out(*[self.ptr(k) if k in names else None for k in ALL],
                                         self.traced.data_ptr() if traced else None)

    def put(self, k, a):
        """Start values (sum, samples, ray_casts of an earlier range)."""
        raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        self.buf[k][G:G + len(raw)] = torch.from_numpy(raw.copy()).to(dev())

    def get(self, k):
        a = self.buf[k].cpu().numpy()
        n = self.size[k]
        assert (a[:G] == FILL).all() and (a[G + n:] == FILL).all(), (k, "guard bytes")
        a = a[G:G + n].copy()
        if k == "invalid":
            return a
        a = a.view(np.uint32)
        return a.reshape(self.n, self.ns, 3) if k in SAMPLE else a.reshape((self.n, 3) if PER[k] == 12 else (self.n,))


def raw_call(eng, p, n, npoints, ns, bl, out, first=0, base=0, seed=SEED, sort_bits=-1, stream=None):
    q = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None  # noqa: E731
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    return E.lib().atr_gather_radiance(eng.h, q(p), q(n), npoints, ns, first, base, bl, C.c_uint64(seed),
                                       C.byref(out) if out is not None else None, sort_bits,
                                       C.c_void_p(stream) if stream else None)


def gather(eng, p, n, ns, bl, first=0, base=0, seed=SEED, sort_bits=-1, start=None, stream=None, wait=True):
    """One call with all outputs into guarded buffers: {name: uint32 bits (invalid: bytes)} and the
    traced count. start: the earlier range's outputs when first > 0."""
    tp = torch.from_numpy(np.array(p, F)).to(dev())  # copies: the cached sets are read-only
    tn = torch.from_numpy(np.array(n, F)).to(dev())
    b = Bufs(len(p), ns)
    if start is not None:
        for k in ("sum", "samples", "ray_casts"):
            b.put(k, start[k])
    torch.cuda.current_stream().synchronize()  # the fills and copies above, ahead of a call on another stream
    assert raw_call(eng, tp, tn, len(p), ns, bl, b.out(), first, base, seed, sort_bits, stream) == 0
    if not wait:
        return b, (tp, tn)
    rc, done = eng.wait()
    assert rc == 0 and done == 0, (rc, done)
    torch.cuda.synchronize()
    return host(b)


def host(b):
    res = {k: b.get(k) for k in ALL}
    res["traced"] = int(b.traced.item()) - 5
    return res


def same(got, w, what, rows=slice(None), traced=True, names=ALL):
    for k in names:
        want = GC.bits(w[k][rows])
        bad = np.flatnonzero((got[k] != want).reshape(len(want), -1).any(axis=1))
        head = bad[:6]
        assert len(bad) == 0, (what, k, len(bad), head.tolist(), got[k][head].reshape(len(head), -1)[:, :6].tolist(),
                               want[head].reshape(len(head), -1)[:, :6].tolist())
    if traced:
        assert got["traced"] == w["traced"], (what, "traced", got["traced"], w["traced"])


# ---- 1. parity -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(GC.NAMES))
def test_parity_with_reference(eng, name):
    p, n = points(name)
    TR.SCENES[name].upload(eng)
    for ns, bl in GC.CONFIGS:
        w = GC.want(name, ns, bl)
        for sb in (0, 5):
            same(gather(eng, p, n, ns, bl, sort_bits=sb), w, (name, ns, bl, sb))


# ---- 2. tails ----------------------------------------------------------------------------------------

TAILS = [(npts, ns) for npts in (1, 2, 63, 64, 65) for ns in (1, 7, 65)] + [
    (npts, ns) for npts in (1, 3) for ns in (63, 64, 129)]


@pytest.mark.parametrize("npts,ns", TAILS)
def test_parity_at_wave_point_and_row_tails(eng, npts, ns):
    """A point crossing wave boundaries, several points in one wave, and the resolve's row tails."""
    MIXED.upload(eng)
    p, n = (a[:npts] for a in points("mixed"))
    w = GRR.gather_radiance(MIXED.oracle(), p, n, ns, 5, SEED)
    for sb in (0, 5, -1):
        same(gather(eng, p, n, ns, 5, sort_bits=sb), w, (npts, ns, sb))


# ---- 3. many batches -----------------------------------------------------------------------------------

@pytest.mark.parametrize("npts,ns,bl", [(322, 100, 2), (3, 5000, 3)])
def test_small_batches_change_no_output(eng, npts, ns, bl):
    """2^12-path batches: 322 points x 100 samples run as many batches of 40 whole points; one point of
    5,000 samples is larger than the tuned batch and is a batch of its own."""
    MIXED.upload(eng)
    p, n = (a[:npts] for a in points("mixed"))
    w = GC.want("mixed", ns, bl) if npts == 322 else GRR.gather_radiance(MIXED.oracle(), p, n, ns, bl, SEED)
    base = eng.tuning()
    whole = gather(eng, p, n, ns, bl)
    same(whole, w, (npts, ns, "default tuning"))
    try:
        eng.set_tuning(path_batch_log2=12)
        assert npts > max(1, 4096 // ns)  # more than one batch
        for sb in (0, 5):
            got = gather(eng, p, n, ns, bl, sort_bits=sb)
            same(got, w, (npts, ns, "2^12-path batches", sb))
            for k in ALL:
                assert np.array_equal(got[k], whole[k]), (npts, ns, sb, k)
    finally:
        eng.set_tuning(**base)


# ---- 4. the occlusion gather's counts ----------------------------------------------------------------------

@pytest.mark.parametrize("name", list(GC.NAMES))
def test_counts_equal_the_occlusion_gathers(eng, name):
    """Consequence 1, device against device: samples == visible + occluded, and with one bounce
    ray_casts == occluded; the directions are the same bits."""
    TR.SCENES[name].upload(eng)
    p, n = points(name)
    ns, first, base = 33, 5, 1000
    tp, tn = torch.from_numpy(np.array(p, F)).to(dev()), torch.from_numpy(np.array(n, F)).to(dev())
    occ, otr = eng.gather_occlusion(tp, tn, ns, None, first, base, SEED, outputs=("visible", "occluded", "dirs"))
    assert eng.wait() == (0, 0)
    torch.cuda.synchronize()
    vis, oc = (occ[k].cpu().numpy().view(np.uint32) for k in ("visible", "occluded"))
    start = {"sum": np.zeros((len(p), 3), F), "samples": np.zeros(len(p), np.uint32),
             "ray_casts": np.zeros(len(p), np.uint32)}
    for bl in (1, 3):
        got = gather(eng, p, n, ns, bl, first, base, start=start)
        assert np.array_equal(got["samples"], vis + oc), bl
        assert np.array_equal(got["dirs"], occ["dirs"].cpu().numpy().view(np.uint32)), bl
        if bl == 1:
            assert np.array_equal(got["ray_casts"], oc)
            assert got["traced"] == int(otr.item())
    assert oc.sum() > 0 and vis.sum() > 0


# ---- 5. split invariance -------------------------------------------------------------------------------

def test_split_invariance(eng):
    MIXED.upload(eng)
    p, n = points("mixed")
    base = 1000
    w = GC.want("mixed", 7, 5, 0, base)
    for sb in (0, 5):
        same(gather(eng, p, n, 7, 5, 0, base, sort_bits=sb), w, ("point_base", sb))
        a = gather(eng, p[:100], n[:100], 7, 5, 0, base, sort_bits=sb)  # cut at point 100
        b = gather(eng, p[100:], n[100:], 7, 5, 0, base + 100, sort_bits=sb)
        same(a, w, ("head", sb), slice(0, 100), traced=False)
        same(b, w, ("tail", sb), slice(100, None), traced=False)
        assert a["traced"] + b["traced"] == w["traced"]
        for ns, cut, bl in ((7, 3, 5), (100, 64, 2)):  # samples [0, cut) then [cut, ns) through sum, samples, ray_casts
            ww = GC.want("mixed", ns, bl, 0, base)
            a = gather(eng, p, n, cut, bl, 0, base, sort_bits=sb)
            same(a, GRR.gather_radiance(MIXED.oracle(), p, n, cut, bl, SEED, 0, base), ("first range", ns, sb))
            b = gather(eng, p, n, ns - cut, bl, cut, base, sort_bits=sb, start=a)
            same(b, ww, ("second range", ns, sb), traced=False, names=POINT)
            for k in SAMPLE:
                assert np.array_equal(np.concatenate([a[k], b[k]], axis=1), GC.bits(ww[k])), (k, ns, sb)
            assert a["traced"] + b["traced"] == ww["traced"]
    # first_sample > 0 against the reference's own continuation, from start values of no earlier call
    rng = np.random.default_rng(3)
    start = {"sum": rng.uniform(0, 4, (len(p), 3)).astype(F), "samples": rng.integers(0, 9, len(p)).astype(np.uint32),
             "ray_casts": rng.integers(0, 50, len(p)).astype(np.uint32)}
    wc = GRR.gather_radiance(MIXED.oracle(), p, n, 5, 3, SEED, 11, base, start)
    same(gather(eng, p, n, 5, 3, 11, base, start=start), wc, "first_sample 11")


# ---- 6. invalid points -------------------------------------------------------------------------------------

def test_invalid_points_sit_between_valid_ones(eng):
    MIXED.upload(eng)
    p, n = (a[:130].copy() for a in points("mixed"))
    clean_p, clean_n = p.copy(), n.copy()
    p[0, 1] = np.nan
    p[31] = np.inf
    n[63] = 0
    n[64] *= F(1.001)
    bad = [0, 31, 63, 64]
    good = np.setdiff1d(np.arange(130), bad)
    for ns, bl in ((1, 1), (7, 5)):
        w = GRR.gather_radiance(MIXED.oracle(), p, n, ns, bl, SEED)
        assert w["invalid"][bad].all() and w["invalid"].sum() == 4
        got = gather(eng, p, n, ns, bl)
        same(got, w, (ns, bl))
        assert got["invalid"].tolist() == [int(i in bad) for i in range(130)]
        for k in ("rgb", "sum", "samples", "ray_casts", "sample_rgb", "dirs"):
            assert (got[k][bad] == 0).all(), k
        clean = gather(eng, clean_p, clean_n, ns, bl)  # the neighbours: a run without the bad points
        for k in ALL:
            assert np.array_equal(got[k][good], clean[k][good]), k
        assert got["traced"] < clean["traced"] and got["traced"] == w["traced"]
        # a later range leaves an invalid point's sum, samples, ray_casts and rgb as they are
        more = gather(eng, p, n, 2, bl, ns, start=got)
        wm = GRR.gather_radiance(MIXED.oracle(), p, n, 2, bl, SEED, ns, 0, start=w)
        same(more, wm, ("later range", ns, bl), names=("sum", "samples", "ray_casts", "invalid") + SAMPLE)
        for k in ("sum", "samples", "ray_casts"):
            assert (more[k][bad] == 0).all(), k
        assert (more["rgb"][bad] == 0xABABABAB).all() and more["invalid"][bad].all()
        assert np.array_equal(more["rgb"][good], GC.bits(wm["rgb"])[good])


# ---- 7. partial outputs and arguments ----------------------------------------------------------------------

def test_only_the_requested_outputs_are_written(eng):
    MIXED.upload(eng)
    npts, ns, bl = 70, 7, 3
    pn, nn = (a[:npts].copy() for a in points("mixed"))
    nn[5] = 0  # an invalid point among them: its zeros are written under the same rule
    w = GRR.gather_radiance(MIXED.oracle(), pn, nn, ns, bl, SEED)
    p, n = torch.from_numpy(pn).to(dev()), torch.from_numpy(nn).to(dev())
    calls = 0
    for names, traced in [((k,), False) for k in ALL] + [((), True), (ALL, True), (("rgb", "dirs"), True)]:
        b = Bufs(npts, ns)
        assert raw_call(eng, p, n, npts, ns, bl, b.out(names, traced)) == 0
        assert eng.wait() == (0, 0)
        torch.cuda.synchronize()
        calls += 1
        for k in ALL:
            got = b.get(k)
            if k in names:
                assert np.array_equal(got, GC.bits(w[k])), (names, k)
            else:
                assert (got.view(np.uint8) == FILL).all(), (names, k)
        assert int(b.traced.item()) == 5 + (w["traced"] if traced else 0), names  # one accumulator, added to
    assert calls == 10


def test_arguments(eng):
    MIXED.upload(eng)
    npts, ns, bl = 9, 3, 2
    pn, nn = (a[:npts] for a in points("mixed"))
    p, n = torch.from_numpy(pn.copy()).to(dev()), torch.from_numpy(nn.copy()).to(dev())
    b = Bufs(npts, ns)
    out, inv = b.out(), -1
    assert raw_call(eng, p, n, npts, ns, bl, None) == inv
    assert raw_call(eng, None, n, npts, ns, bl, out) == inv
    assert raw_call(eng, p, None, npts, ns, bl, out) == inv
    assert raw_call(eng, p, n, -1, ns, bl, out) == inv
    assert raw_call(eng, p, n, 2 ** 31, 1, bl, out) == inv
    assert raw_call(eng, p, n, 2 ** 15, 65536, bl, out) == inv  # npoints x nsamples == 2^31
    for bad_ns in (0, -1, 65537):
        assert raw_call(eng, p, n, npts, bad_ns, bl, out) == inv
    assert raw_call(eng, p, n, npts, ns, bl, out, first=2 ** 24 - ns + 1) == inv
    assert raw_call(eng, p, n, npts, ns, bl, out, base=-1) == inv
    assert raw_call(eng, p, n, npts, ns, bl, out, base=2 ** 32 - npts + 1) == inv
    for bad_bl in (0, -1, 65):
        assert raw_call(eng, p, n, npts, ns, bad_bl, out) == inv
    for bad_sb in (-2, 1, 8):
        assert raw_call(eng, p, n, npts, ns, bl, out, sort_bits=bad_sb) == inv
    assert raw_call(eng, p, n, npts, ns, bl, b.out([k for k in ALL if k != "sum"]), first=1) == inv  # no sum
    assert raw_call(eng, p, n, npts, ns, bl, b.out([k for k in ALL if k != "samples"]), first=1) == inv  # no samples
    assert raw_call(eng, p, n, npts, ns, bl, b.out((), False)) == inv  # nothing to write
    assert raw_call(eng, p, n, 0, ns, bl, out) == 0 and raw_call(eng, None, None, 0, ns, bl, None) == 0
    torch.cuda.synchronize()
    for k in ALL:
        assert (b.get(k).view(np.uint8) == FILL).all()
    assert int(b.traced.item()) == 5  # nothing was written
    # the ranges at their upper ends
    start = {"sum": np.zeros((npts, 3), F), "samples": np.zeros(npts, np.uint32),
             "ray_casts": np.zeros(npts, np.uint32)}
    w = GRR.gather_radiance(MIXED.oracle(), pn, nn, ns, 64, SEED, 2 ** 24 - ns, 2 ** 32 - npts, start)
    for sb in (0, 2, 7):
        got = gather(eng, pn, nn, ns, 64, 2 ** 24 - ns, 2 ** 32 - npts, sort_bits=sb, start=start)
        same(got, w, ("upper ends", sb))
    w = GRR.gather_radiance(MIXED.oracle(), pn[:1], nn[:1], 65536, 2, SEED)  # the most samples a point can have
    same(gather(eng, pn[:1], nn[:1], 65536, 2), w, "65,536 samples")
    with pytest.raises(ValueError):
        eng.gather_radiance(p.t().contiguous().t(), n, ns, bl)  # not contiguous
    with pytest.raises(ValueError):
        eng.gather_radiance(p.double(), n, ns, bl)
    with pytest.raises(ValueError):
        eng.gather_radiance(p, n[:-1], ns, bl)
    with pytest.raises(ValueError):
        eng.gather_radiance(p, n, ns, bl, want=("rgb", "hits"))
    with pytest.raises(ValueError):
        eng.gather_radiance(p, n, ns, bl, first_sample=3)  # nothing to continue
    fresh = E.Engine(0)
    try:
        assert raw_call(fresh, p, n, npts, ns, bl, out) == -4  # ATR_E_NOSCENE
    finally:
        fresh.close()


def test_engine_method(eng):
    """Engine.gather_radiance: the default outputs, and a sample range continued through start."""
    MIXED.upload(eng)
    pn, nn = points("mixed")
    p, n = torch.from_numpy(pn.copy()).to(dev()), torch.from_numpy(nn.copy()).to(dev())
    w = GC.want("mixed", 7, 5)
    out, traced = eng.gather_radiance(p, n, 7, 5, seed=SEED)
    assert eng.wait() == (0, 0)
    torch.cuda.synchronize()
    assert sorted(out) == ["invalid", "rgb", "samples"]
    assert np.array_equal(out["rgb"].cpu().numpy().view(np.uint32), GC.bits(w["rgb"]))
    assert np.array_equal(out["samples"].cpu().numpy().view(np.uint32), w["samples"])
    assert not out["invalid"].cpu().numpy().any() and int(traced.item()) == w["traced"]
    a, _ = eng.gather_radiance(p, n, 3, 5, seed=SEED, want=("sum", "samples", "ray_casts", "sample_rgb"))
    b, _ = eng.gather_radiance(p, n, 4, 5, seed=SEED, first_sample=3, want=("rgb", "sample_rgb"),
                               start={k: a[k] for k in ("sum", "samples", "ray_casts")})
    assert eng.wait() == (0, 0)
    torch.cuda.synchronize()
    assert b["sum"] is a["sum"] and b["samples"] is a["samples"]
    for k in ("sum", "rgb", "samples", "ray_casts"):
        assert np.array_equal(b[k].cpu().numpy().view(np.uint32), GC.bits(w[k])), k
    both = torch.cat([a["sample_rgb"], b["sample_rgb"]], dim=1).cpu().numpy()
    assert np.array_equal(both.view(np.uint32), GC.bits(w["sample_rgb"]))


# ---- 8. streams and the render paths after a call ----------------------------------------------------------

def test_a_stream_of_its_own_then_a_render_and_a_radiance_call(eng):
    """A call on a non-default stream; atr_render_wait reports no tiles for it and atr_last_kernel_ms
    times it. A PATHS render and an atr_radiance_rays call on the same context afterwards still equal
    their references."""
    from tests import test_gpu_radiance as GRAD
    MIXED.upload(eng)
    p, n = points("mixed")
    s1 = torch.cuda.Stream(dev())
    torch.cuda.synchronize()
    a = gather(eng, p, n, 7, 5, stream=s1.cuda_stream, wait=False)
    b = gather(eng, p, n, 64, 3, wait=False)  # torch's current stream: takes over or opens a workspace
    rc, done = eng.wait()
    assert (rc, done) == (0, 0) and 0 < eng.last_kernel_ms() < 10000
    torch.cuda.synchronize()
    same(host(a[0]), GC.want("mixed", 7, 5), "its own stream")
    same(host(b[0]), GC.want("mixed", 64, 3), "the current stream")
    c = gather(eng, p, n, 7, 5, wait=False)
    r = run(eng, E.camera(SW, SH, 2, 5), variant=E.ATR_KERNEL_PATHS)  # no wait between: takes the workspace over
    same_render(r, ref(MIXED, SW, SH, 2, 5), "PATHS render after a gather")
    same(host(c[0]), GC.want("mixed", 7, 5), "the call before the render")
    o, d = RC.batch("mixed", "aimed")
    GRAD.same(GRAD.radiance(eng, o, d, 2, 5), RC.want("mixed", "aimed", 2, 5), "radiance after a gather")
    same(gather(eng, p, n, 7, 5), GC.want("mixed", 7, 5), "after both")
    assert 1 <= eng.workspace_info()["workspaces"] <= 4
