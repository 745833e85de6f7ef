"""atr_probe_sh on the GPU: every output (sh, sum, ray_casts, invalid, sample_rgb, dirs, traced_rays) for
exact equality with the reference of tests/probe_sh_ref.py (the sphere sampler, then the oracle's own
cast_ray on the same stream, projected in sample order; validated without a GPU in
tests/test_probe_sh_cpu.py, which also asserts that the probe sets used here reach every bounce level,
every kind of surface, a probe inside a closed mesh, one that sees only sky and non-finite ones): every
scene, the sample counts around the resolve's rows of 64, the probe counts around a block's four waves;
the device's own ties (atr_trace_rays on the generated directions, a sky-only scene against numpy and
against pi x emission); split invariance by probes, samples, queue order, batch size and stream;
every subset of the output pointers; invalid probes; arguments. Every buffer is filled with a sentinel
first and guarded on both sides. Needs an MI355X (-m gpu). No test reaches the sampler's 32-try
fallback on the device (about 1e-10 per sample): the reference reaches it with max_tries 1."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from tests import probe_sh_ref as PR  # noqa: E402
from tests import ray_sets as R  # noqa: E402
from tests import test_probe_sh_cpu as PC  # noqa: E402
from tests import test_gpu_trace_rays as TR  # noqa: E402
from tests.test_gather_cpu import points  # noqa: E402
from tests.test_gpu_parity import eng  # noqa: E402,F401
from tests.test_gpu_scenes import MATS, MIXED, Sc  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SEED = PC.SEED
PROBE = ("sh", "sum", "ray_casts", "invalid")
SAMPLE = ("sample_rgb", "dirs")
ALL = PROBE + SAMPLE  # atr_probe_sh_out's order
PER = {"sh": 108, "sum": 108, "ray_casts": 4, "invalid": 1}  # bytes per probe
G = 256  # guard bytes around every output buffer
FILL = 0xAB
SKY_ONLY = Sc([], [], MATS)


def dev():
    return torch.device("cuda", 0)


class Bufs:
    """The six output buffers of n probes x ns samples with G guard bytes on both sides, filled with
    0xAB, and the traced-ray accumulator, started at 5."""

    def __init__(self, n, ns):
        self.n, self.ns = n, ns
        self.size = {k: n * PER[k] if k in PER else n * ns * 12 for k in ALL}
        self.buf = {k: torch.full((self.size[k] + 2 * G,), FILL, dtype=torch.uint8, device=dev()) for k in ALL}
        self.traced = torch.full((1,), 5, dtype=torch.int64, device=dev())

    def ptr(self, k):
        return self.buf[k].data_ptr() + G

    def out(self, names=ALL, traced=True):
        return E.atr_probe_sh_out(*[self.ptr(k) if k in names else None for k in ALL],
                                  self.traced.data_ptr() if traced else None)

    def put(self, k, a):
        """Start values (sum, ray_casts of an earlier range)."""
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
        if k in SAMPLE:
            return a.reshape(self.n, self.ns, 3)
        return a.reshape((self.n, 27) if PER[k] == 108 else (self.n,))


def raw_call(eng, p, npoints, ns, bl, out, first=0, base=0, seed=SEED, sort_bits=-1, stream=None):
    if stream is None:
        stream = torch.cuda.current_stream().cuda_stream
    return E.lib().atr_probe_sh(eng.h, C.c_void_p(p.data_ptr()) if p is not None else None, npoints, ns, first, base,
                                bl, C.c_uint64(seed), C.byref(out) if out is not None else None, sort_bits,
                                C.c_void_p(stream) if stream else None)


def probe(eng, p, ns, bl, first=0, base=0, seed=SEED, sort_bits=-1, start=None, stream=None, wait=True):
    """One call with all outputs into guarded buffers: {name: uint32 bits (invalid: bytes)} and the
    traced count. start: the earlier range's outputs when first > 0."""
    tp = torch.from_numpy(np.array(p, F)).to(dev())  # a copy: the cached sets are read-only
    b = Bufs(len(p), ns)
    if start is not None:
        for k in ("sum", "ray_casts"):
            b.put(k, start[k])
    torch.cuda.current_stream().synchronize()  # the fills and copies above, ahead of a call on another stream
    assert raw_call(eng, tp, len(p), ns, bl, b.out(), first, base, seed, sort_bits, stream) == 0
    if not wait:
        return b, tp
    rc, done = eng.wait()
    assert rc == 0 and done == 0, (rc, done)
    torch.cuda.synchronize()
    return host(b)


def host(b):
    res = {k: b.get(k) for k in ALL}
    res["traced"] = int(b.traced.item()) - 5
    return res


def same(got, w, what, rows=slice(None), traced=None, names=ALL):
    for k in names:
        want = PC.bits(w[k][rows])
        bad = np.flatnonzero((got[k] != want).reshape(len(want), -1).any(axis=1))
        head = bad[:6]
        assert len(bad) == 0, (what, k, len(bad), head.tolist(), got[k][head].reshape(len(head), -1)[:, :6].tolist(),
                               want[head].reshape(len(head), -1)[:, :6].tolist())
    if traced is not None:
        assert got["traced"] == traced, (what, "traced", got["traced"], traced)


# ---- 1. parity -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(PC.NAMES))
def test_parity_with_reference(eng, name):
    """Every configuration on the first 1, 3, 4 and 5 probes (the hand-placed ones: inside, apart,
    non-finite) and on the whole set; a probe's outputs do not depend on its neighbours, so the
    reference of a subset is the whole set's rows."""
    p = PC.probes(name)
    TR.SCENES[name].upload(eng)
    for ns, bl in PC.CONFIGS:
        w = PC.want(name, ns, bl)
        for npts in (1, 3, 4, 5, len(p)):
            rows = slice(0, npts)
            same(probe(eng, p[:npts], ns, bl), w, (name, ns, bl, npts), rows, PC.traced_of(w, bl, rows))
        assert PC.traced_of(w, bl) == w["traced"]
    first, base = 11, 1000
    w = PC.want(name, 7, 5, first, base)
    start = {"sum": np.zeros((len(p), 27), F), "ray_casts": np.zeros(len(p), np.uint32)}
    assert PR.SENTINEL == 0x01010101 * FILL  # an invalid probe's sh: unwritten by the reference and by the device
    same(probe(eng, p, 7, 5, first, base, start=start), w, (name, "first_sample, point_base"), traced=w["traced"])


# ---- 2. the device's own ties --------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(PC.NAMES))
def test_one_bounce_counts_equal_trace_rays(eng, name):
    """Consequence 1, device against device: with bounce_limit 1 a sample casts 1 iff its first segment
    hits anything, which atr_trace_rays answers on the generated directions; a miss's colour is the
    sky's emission."""
    TR.SCENES[name].upload(eng)
    p = PC.probes(name)
    ns = 65
    got = probe(eng, p, ns, 1)
    ok = np.flatnonzero(got["invalid"] == 0)
    assert len(ok) == len(p) - 2
    d = got["dirs"][ok].view(F).reshape(-1, 3)
    o = np.repeat(np.asarray(p)[ok], ns, axis=0)
    assert R.passes(o, d).all()
    hit = TR.query(eng, o, d, outputs=("t",))["t"].reshape(len(ok), ns) < R.MAX_FLOAT
    assert np.array_equal(got["ray_casts"][ok], hit.sum(axis=1).astype(np.uint32))
    assert hit.any() and not hit.all()
    sky = PC.bits(np.asarray(TR.SCENES[name].materials[0][0], F))
    assert (got["sample_rgb"][ok][~hit] == sky).all()
    assert got["traced"] == len(ok) * ns


def test_sky_only_scene_against_numpy_and_pi_times_emission(eng):
    """Nothing to hit: every sample's colour is the sky's emission L, so sum is the numpy restatement
    on atr_probe_directions' directions alone. And the irradiance of a constant radiance is pi L for
    every normal n. The estimate's error: sh[0] is exact up to rounding (Y0 is a constant); for k >= 1,
    sh[k] = 4 pi L mean(Yk) with mean(Yk) of variance 1/(4 pi N) and the k uncorrelated (the basis is
    orthonormal), so E(n) = sum_k A_k sh[k] Yk(n) has standard deviation L sqrt(4 pi / N sum_{k>=1}
    A_k^2 Yk(n)^2) with A = pi, 2 pi / 3, pi / 4 per band. The bound is six of those plus 1e-3 L for
    f32 rounding (an N-term f32 sum errs by at most N 2^-24 of its terms' absolute sum, N x 1.1 L; times
    4 pi / N and sum_k A_k |Yk(n)| <= 8.3 that is 9e-4 L at N = 129)."""
    SKY_ONLY.upload(eng)
    n, ns, base = 255, 129, 77
    p = np.array(PC.probes("mixed"))
    got = probe(eng, p, ns, 3, 0, base)
    ok = got["invalid"] == 0
    L = np.asarray(MATS[0][0], F)
    d, _ = E.probe_directions(n, ns, 0, base, SEED)
    assert np.array_equal(got["dirs"][ok], PC.bits(d)[ok])
    rgb = np.broadcast_to(L, (n, ns, 3))
    assert (got["sample_rgb"][ok] == PC.bits(L)).all()
    sums = PR.np_sums(rgb, d)
    assert np.array_equal(got["sum"][ok], PC.bits(sums)[ok])
    assert np.array_equal(got["sh"][ok], PC.bits(PR.np_sh(sums, ns))[ok])
    assert (got["ray_casts"][ok] == 0).all() and got["traced"] == int(ok.sum()) * ns
    nrm = np.concatenate([np.eye(3, dtype=F), -np.eye(3, dtype=F), R.random_dirs(10, np.random.default_rng(63))])
    e = E.sh_irradiance(got["sh"].view(F).reshape(n, 9, 3)[ok], nrm).astype(np.float64)  # (probes, normals, 3)
    a = np.array([math.pi] + [2 * math.pi / 3] * 3 + [math.pi / 4] * 5)
    y = E.sh_basis(nrm).astype(np.float64)
    sigma = np.sqrt(4 * math.pi / ns * ((a[1:] * y[:, 1:]) ** 2).sum(axis=1))  # per normal, in units of L
    bound = (6.0 * sigma[None, :, None] + 1e-3) * L[None, None, :]
    err = np.abs(e - math.pi * L[None, None, :])
    print("largest error over its bound", float((err / bound).max()))
    assert (err <= bound).all()


# ---- 3. split invariance -------------------------------------------------------------------------------

def test_split_invariance(eng):
    MIXED.upload(eng)
    p = PC.probes("mixed")
    base = 1000
    w = PR.probe_sh(MIXED.oracle(), p, 7, 5, SEED, 0, base)
    for sb in (0, 2, 5, -1):
        same(probe(eng, p, 7, 5, 0, base, sort_bits=sb), w, ("point_base", sb), traced=w["traced"])
        a = probe(eng, p[:100], 7, 5, 0, base, sort_bits=sb)  # cut at probe 100
        b = probe(eng, p[100:], 7, 5, 0, base + 100, sort_bits=sb)
        same(a, w, ("head", sb), slice(0, 100))
        same(b, w, ("tail", sb), slice(100, None))
        assert a["traced"] + b["traced"] == w["traced"]
    for sb in (0, 5):
        for ns, cut, bl in ((7, 3, 5), (129, 64, 2)):  # samples [0, cut) then [cut, ns) through sum and ray_casts
            ww = PR.probe_sh(MIXED.oracle(), p, ns, bl, SEED, 0, base)
            a = probe(eng, p, cut, bl, 0, base, sort_bits=sb)
            wa = PR.probe_sh(MIXED.oracle(), p, cut, bl, SEED, 0, base)
            same(a, wa, ("first range", ns, sb), traced=wa["traced"])
            b = probe(eng, p, ns - cut, bl, cut, base, sort_bits=sb, start=a)
            good = ww["invalid"] == 0
            same(b, ww, ("second range", ns, sb), names=("sum", "ray_casts", "invalid"))
            assert np.array_equal(b["sh"][good], PC.bits(ww["sh"])[good])
            assert (b["sh"][~good] == 0xABABABAB).all()  # an invalid probe's sh is not written after the first range
            for k in SAMPLE:
                assert np.array_equal(np.concatenate([a[k], b[k]], axis=1), PC.bits(ww[k])), (k, ns, sb)
            assert a["traced"] + b["traced"] == ww["traced"]
    # first_sample > 0 against the reference's own continuation, from start values of no earlier call
    rng = np.random.default_rng(3)
    start = {"sum": rng.uniform(-4, 4, (len(p), 27)).astype(F), "ray_casts": rng.integers(0, 50, len(p)).astype(np.uint32)}
    wc = PR.probe_sh(MIXED.oracle(), p, 5, 3, SEED, 11, base, start)
    same(probe(eng, p, 5, 3, 11, base, start=start), wc, "first_sample 11", traced=wc["traced"],
         names=("sum", "ray_casts", "invalid") + SAMPLE)


def test_small_batches_and_streams_change_no_output(eng):
    """2^12-path batches (255 probes x 129 samples run as nine batches of whole probes) against the
    default; a stream of its own; two calls on two streams beside an atr_gather_radiance."""
    MIXED.upload(eng)
    p = PC.probes("mixed")
    ns, bl = 129, 2
    w = PC.want("mixed", ns, bl)
    whole = probe(eng, p, ns, bl)
    same(whole, w, "default tuning", traced=w["traced"])
    base = eng.tuning()
    try:
        eng.set_tuning(path_batch_log2=12)
        assert len(p) > 4096 // ns  # more than one batch
        for sb in (0, 5):
            same(probe(eng, p, ns, bl, sort_bits=sb), w, ("2^12-path batches", sb), traced=w["traced"])
    finally:
        eng.set_tuning(**base)
    s1, s2 = torch.cuda.Stream(dev()), torch.cuda.Stream(dev())
    torch.cuda.synchronize()
    a = probe(eng, p, 7, 5, stream=s1.cuda_stream, wait=False)
    gp, gn = (torch.from_numpy(np.array(x, F)).to(dev()) for x in points("mixed"))
    torch.cuda.current_stream().synchronize()
    g, gt = eng.gather_radiance(gp, gn, 7, 5, seed=SEED, want=("sum", "samples"))  # torch's current stream
    b = probe(eng, p, 64, 3, stream=s2.cuda_stream, wait=False)
    rc, done = eng.wait()
    assert (rc, done) == (0, 0) and 0 < eng.last_kernel_ms() < 10000
    torch.cuda.synchronize()
    wa, wb = PC.want("mixed", 7, 5), PC.want("mixed", 64, 3)
    same(host(a[0]), wa, "stream 1", traced=wa["traced"])
    same(host(b[0]), wb, "stream 2", traced=wb["traced"])
    from tests import test_gather_radiance_cpu as GRC
    wg = GRC.want("mixed", 7, 5)
    assert np.array_equal(g["sum"].cpu().numpy().view(np.uint32), GRC.bits(wg["sum"]))
    assert int(gt.item()) == wg["traced"]
    same(probe(eng, p, 7, 5), wa, "after them", traced=wa["traced"])


# ---- 4. buffers ------------------------------------------------------------------------------------------

def test_every_subset_of_the_outputs(eng):
    """All 127 non-empty subsets of the seven output pointers: what is asked for has the reference's
    bits, everything else and every guard byte stays as filled."""
    MIXED.upload(eng)
    npts, ns, bl = 9, 7, 3
    pn = np.array(PC.probes("mixed")[:npts])  # the non-finite probe at index 2 is among them
    w = PR.probe_sh(MIXED.oracle(), pn, ns, bl, SEED)
    p = torch.from_numpy(pn).to(dev())
    calls = 0
    for mask in itertools.product((False, True), repeat=7):
        names, traced = tuple(k for k, m in zip(ALL, mask) if m), mask[6]
        b = Bufs(npts, ns)
        rc = raw_call(eng, p, npts, ns, bl, b.out(names, traced))
        if not any(mask):
            assert rc == -1  # nothing to write
            continue
        assert rc == 0 and eng.wait() == (0, 0)
        torch.cuda.synchronize()
        calls += 1
        for k in ALL:
            got = b.get(k)
            if k in names:
                assert np.array_equal(got, PC.bits(w[k])), (names, k)
            else:
                assert (got.view(np.uint8) == FILL).all(), (names, k)
        assert int(b.traced.item()) == 5 + (w["traced"] if traced else 0), names  # one accumulator, added to
    assert calls == 127


def test_invalid_probes_sit_between_valid_ones(eng):
    MIXED.upload(eng)
    p = np.array(PC.probes("mixed")[:130])
    clean_p = p.copy()
    clean_p[PC.NAN] = [0.5, 0.25, -3.0]
    p[31] = np.inf
    p[63, 0] = -np.inf
    p[64, 2] = np.nan
    bad = [PC.NAN, 31, 63, 64]
    good = np.setdiff1d(np.arange(130), bad)
    for ns, bl in ((1, 1), (7, 5)):
        w = PR.probe_sh(MIXED.oracle(), p, ns, bl, SEED)
        assert w["invalid"][bad].all() and w["invalid"].sum() == 4
        got = probe(eng, p, ns, bl)
        same(got, w, (ns, bl), traced=w["traced"])
        assert got["invalid"].tolist() == [int(i in bad) for i in range(130)]
        for k in ALL:
            if k != "invalid":
                assert (got[k][bad] == 0).all(), k
        clean = probe(eng, clean_p, ns, bl)  # the neighbours: a run without the bad probes
        for k in ALL:
            assert np.array_equal(got[k][good], clean[k][good]), k
        assert got["traced"] < clean["traced"]
        # a later range leaves an invalid probe's sh, sum and ray_casts as they are
        rng = np.random.default_rng(5)
        start = {"sum": rng.uniform(-4, 4, (130, 27)).astype(F), "ray_casts": rng.integers(1, 50, 130).astype(np.uint32)}
        more = probe(eng, p, 2, bl, ns, start=start)
        wm = PR.probe_sh(MIXED.oracle(), p, 2, bl, SEED, ns, 0, start=start)
        same(more, wm, ("later range", ns, bl), names=("sum", "ray_casts", "invalid") + SAMPLE, traced=wm["traced"])
        for k in ("sum", "ray_casts"):
            assert np.array_equal(more[k][bad], PC.bits(start[k])[bad]), k
        assert (more["sh"][bad] == 0xABABABAB).all() and more["invalid"][bad].all()
        assert np.array_equal(more["sh"][good], PC.bits(wm["sh"])[good])
        assert (more["sample_rgb"][bad] == 0).all() and (more["dirs"][bad] == 0).all()


# ---- 5. arguments and the Engine method ------------------------------------------------------------------

def test_arguments(eng):
    MIXED.upload(eng)
    npts, ns, bl = 9, 3, 2
    pn = np.array(PC.probes("mixed")[:npts])
    p = torch.from_numpy(pn).to(dev())
    b = Bufs(npts, ns)
    out, inv = b.out(), -1
    assert raw_call(eng, p, npts, ns, bl, None) == inv
    assert raw_call(eng, None, npts, ns, bl, out) == inv
    assert raw_call(eng, p, -1, ns, bl, out) == inv
    assert raw_call(eng, p, 2 ** 31, 1, bl, out) == inv
    assert raw_call(eng, p, 2 ** 15, 65536, bl, out) == inv  # npoints x nsamples == 2^31
    for bad_ns in (0, -1, 65537):
        assert raw_call(eng, p, npts, bad_ns, bl, out) == inv
    assert raw_call(eng, p, npts, ns, bl, out, first=2 ** 24 - ns + 1) == inv
    assert raw_call(eng, p, npts, ns, bl, out, base=-1) == inv
    assert raw_call(eng, p, npts, ns, bl, out, base=2 ** 32 - npts + 1) == inv
    for bad_bl in (0, -1, 65):
        assert raw_call(eng, p, npts, ns, bad_bl, out) == inv
    for bad_sb in (-2, 1, 8):
        assert raw_call(eng, p, npts, ns, bl, out, sort_bits=bad_sb) == inv
    assert raw_call(eng, p, npts, ns, bl, b.out([k for k in ALL if k != "sum"]), first=1) == inv  # no sum
    assert raw_call(eng, p, npts, ns, bl, b.out((), False)) == inv  # nothing to write
    assert raw_call(eng, p, 0, ns, bl, out) == 0 and raw_call(eng, None, 0, ns, bl, None) == 0
    torch.cuda.synchronize()
    for k in ALL:
        assert (b.get(k).view(np.uint8) == FILL).all()
    assert int(b.traced.item()) == 5  # nothing was written
    # the ranges at their upper ends
    start = {"sum": np.zeros((npts, 27), F), "ray_casts": np.zeros(npts, np.uint32)}
    w = PR.probe_sh(MIXED.oracle(), pn, ns, 64, SEED, 2 ** 24 - ns, 2 ** 32 - npts, start)
    for sb in (0, 2, 7):
        got = probe(eng, pn, ns, 64, 2 ** 24 - ns, 2 ** 32 - npts, sort_bits=sb, start=start)
        same(got, w, ("upper ends", sb), traced=w["traced"], names=("sum", "ray_casts", "invalid") + SAMPLE)
        assert np.array_equal(got["sh"][w["invalid"] == 0], PC.bits(w["sh"])[w["invalid"] == 0])
    with pytest.raises(ValueError):
        eng.probe_sh(p.t().contiguous().t(), ns, bl)  # not contiguous
    with pytest.raises(ValueError):
        eng.probe_sh(p.double(), ns, bl)
    with pytest.raises(ValueError):
        eng.probe_sh(p, ns, bl, want=("sh", "rgb"))
    with pytest.raises(ValueError):
        eng.probe_sh(p, ns, bl, first_sample=3)  # nothing to continue
    fresh = E.Engine(0)
    try:
        assert raw_call(fresh, p, npts, ns, bl, out) == -4  # ATR_E_NOSCENE
    finally:
        fresh.close()


def test_engine_method(eng):
    """Engine.probe_sh: the default outputs, and a sample range continued through start."""
    MIXED.upload(eng)
    pn = PC.probes("mixed")
    p = torch.from_numpy(np.array(pn)).to(dev())
    w = PC.want("mixed", 7, 5)
    out, traced = eng.probe_sh(p, 7, 5, seed=SEED)
    assert eng.wait() == (0, 0)
    torch.cuda.synchronize()
    assert sorted(out) == ["invalid", "sh"] and tuple(out["sh"].shape) == (len(pn), 9, 3)
    assert np.array_equal(out["sh"].cpu().numpy().view(np.uint32).reshape(-1, 27), PC.bits(w["sh"]))
    assert np.array_equal(out["invalid"].cpu().numpy(), w["invalid"]) and int(traced.item()) == w["traced"]
    a, _ = eng.probe_sh(p, 3, 5, seed=SEED, want=("sum", "ray_casts", "sample_rgb"))
    b, _ = eng.probe_sh(p, 4, 5, seed=SEED, first_sample=3, want=("sh", "sample_rgb"),
                        start={k: a[k] for k in ("sum", "ray_casts")})
    assert eng.wait() == (0, 0)
    torch.cuda.synchronize()
    assert b["sum"] is a["sum"] and b["ray_casts"] is a["ray_casts"]
    good = w["invalid"] == 0
    for k in ("sum", "ray_casts"):
        assert np.array_equal(b[k].cpu().numpy().view(np.uint32).reshape(len(pn), -1),
                              PC.bits(w[k]).reshape(len(pn), -1)), k
    assert np.array_equal(b["sh"].cpu().numpy().view(np.uint32).reshape(-1, 27)[good], PC.bits(w["sh"])[good])
    both = torch.cat([a["sample_rgb"], b["sample_rgb"]], dim=1).cpu().numpy()
    assert np.array_equal(both.view(np.uint32), PC.bits(w["sample_rgb"]))
    grid = torch.from_numpy(E.probe_grid((-1, 0, -4), (1, 2, -2), (3, 2, 2))).to(dev())
    out, _ = eng.probe_sh(grid, 16, 2, seed=SEED)
    assert eng.wait() == (0, 0)
    torch.cuda.synchronize()
    assert tuple(out["sh"].shape) == (12, 9, 3) and not out["invalid"].cpu().numpy().any()
