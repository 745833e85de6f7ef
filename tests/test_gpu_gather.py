"""atr_gather_occlusion on the GPU: all five outputs (visible, occluded, mask, dirs, traced_rays) for
exact equality with the reference of tests/gather_ref.py (the sampler restated with the oracle's RNG,
the occlusion reference's walk per traced sample; validated without a GPU in tests/test_gather_cpu.py):
every scene, sample count, t_max set and variant; wave tails; the engine's own occlusion query and
host sampler; split invariance; invalid points and what is written; arguments; streams. Needs an
MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from tests import gather_ref as GR  # noqa: E402
from tests import ray_sets as R  # noqa: E402
from tests import test_gpu_trace_rays as TR  # noqa: E402
from tests.test_gather_cpu import SEED, bits, points  # noqa: E402
from tests.test_gpu_parity import eng  # noqa: E402,F401
from tests.test_gpu_scenes import MIXED  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
VARIANTS = (E.ATR_KERNEL_AUTO, E.ATR_KERNEL_LANE)
ALL = ("visible", "occluded", "mask", "dirs")
FIRST, BASE = 3, 1000  # the parity tests' first_sample and point_base

_want = {}


def dev():
    return torch.device("cuda", 0)


def diagonal(name):
    box = TR.boxes(name)[0]
    return np.sqrt(R.len2((box[3:] - box[:3])[None]))[0]


def tmax_set(name, which):
    """The t_max sets of the parity test (None: the NULL pointer)."""
    n = len(points(name)[0])
    if which == "null":
        return None
    if which == "radius":
        return np.full(n, F(0.25) * diagonal(name), F)
    return (np.random.default_rng(8).uniform(0.02, 0.6, n).astype(F) * diagonal(name)).astype(F)


def want(name, ns, which):
    """The reference's outputs of a scene's point set (computed once, read-only)."""
    if (name, ns, which) not in _want:
        p, n = points(name)
        w = GR.gather(TR.SCENES[name].oracle(), p, n, ns, tmax_set(name, which), FIRST, BASE, SEED)
        for a in w.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _want[name, ns, which] = w
    return _want[name, ns, which]


def gather(eng, p, n, ns, t_max=None, variant=E.ATR_KERNEL_AUTO, first=FIRST, base=BASE, seed=SEED, stream=None,
           wait=True, outputs=ALL):
    """One atr_gather_occlusion call: numpy outputs (counts and mask as uint32) and the traced count."""
    tp = torch.from_numpy(np.array(p, F)).to(dev())  # copies: the cached sets are read-only
    tn = torch.from_numpy(np.array(n, F)).to(dev())
    tm = None if t_max is None else torch.from_numpy(np.array(t_max, F)).to(dev())
    out, traced = eng.gather_occlusion(tp, tn, ns, tm, first, base, seed, variant=variant, stream=stream,
                                       outputs=outputs)
    if not wait:
        return out, traced, (tp, tn, tm)
    rc, done = eng.wait()
    assert rc == 0 and done == 0, (rc, done)
    torch.cuda.synchronize()
    return host(out, traced)


def host(out, traced):
    res = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("visible", "occluded", "mask"):
        if k in res:
            res[k] = res[k].view(np.uint32)
    res["traced"] = int(traced.item())
    return res


def same(got, w, what, rows=slice(None)):
    for k in ("visible", "occluded", "mask"):
        if k in got:
            bad = np.flatnonzero((got[k] != w[k][rows]).reshape(len(got[k]), -1).any(axis=1))
            assert len(bad) == 0, (what, k, len(bad), bad[:6].tolist(), got[k][bad[:6]].tolist(),
                                   w[k][rows][bad[:6]].tolist())
    if "dirs" in got:
        bad = np.flatnonzero((bits(got["dirs"]) != bits(w["dirs"][rows])).any(axis=(1, 2)))
        assert len(bad) == 0, (what, "dirs", len(bad), bad[:6].tolist())
    if "traced" in got and rows == slice(None):
        assert got["traced"] == w["traced"], (what, got["traced"], w["traced"])


def unpack(mask, ns):
    """(n, words) u32 mask -> (n, ns) 0/1."""
    b = (mask[:, :, None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return b.reshape(len(mask), -1)[:, :ns].astype(np.uint8)


# ---- 1. parity -------------------------------------------------------------------------------------

@pytest.mark.parametrize("ns", [1, 7, 32, 64, 100, 128])
@pytest.mark.parametrize("name", list(TR.SCENES))
def test_parity_with_reference(eng, name, ns):
    p, n = points(name)
    for which in ("null", "radius", "random"):
        w = want(name, ns, which)
        # both answers and a sample below the horizon are in the batch (every scene has occluders)
        assert w["visible"].sum() > 0 and w["occluded"].sum() > 0 and (w["flags"] == 0).any(), (name, ns, which)
        assert w["traced"] == int(w["visible"].sum() + w["occluded"].sum()) == int(w["flags"].sum())
    TR.SCENES[name].upload(eng)
    for which in ("null", "radius", "random"):
        for variant in VARIANTS:
            got = gather(eng, p, n, ns, tmax_set(name, which), variant)
            same(got, want(name, ns, which), (name, ns, which, variant))


# ---- 2. tails ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("ns,npoints", [(7, 1), (7, 9), (7, 10), (64, 1), (64, 2)])
def test_parity_at_wave_tails(eng, ns, npoints):
    MIXED.upload(eng)
    p, n = (a[:npoints] for a in points("mixed"))
    tm = tmax_set("mixed", "random")[:npoints]
    w = GR.gather(TR.SCENES["mixed"].oracle(), p, n, ns, tm, FIRST, BASE, SEED)
    for variant in VARIANTS:
        same(gather(eng, p, n, ns, tm, variant), w, (ns, npoints, variant))


# ---- 3. the engine against itself ------------------------------------------------------------------------

@pytest.mark.parametrize("name,ns", [("mixed", 100), ("soup", 64)])
def test_against_occluded_rays_and_the_host_sampler(eng, name, ns):
    TR.SCENES[name].upload(eng)
    p, n = points(name)
    tm = tmax_set(name, "random")
    d, t = E.gather_directions(n, ns, FIRST, BASE, SEED)
    flat = t.reshape(-1) == 1
    o = torch.from_numpy(np.repeat(p, ns, axis=0)[flat]).to(dev())
    dd = torch.from_numpy(d.reshape(-1, 3)[flat]).to(dev())
    tt = torch.from_numpy(np.repeat(tm, ns)[flat]).to(dev())
    for variant in VARIANTS:
        occ, traced = eng.occluded_rays(o, dd, tt, variant=variant, sort_bits=0)
        assert eng.wait() == (0, 0)
        torch.cuda.synchronize()
        vis = np.zeros(len(p) * ns, np.uint8)
        vis[flat] = occ.cpu().numpy() == E.ATR_OCCL_VISIBLE
        assert (occ.cpu().numpy() != E.ATR_OCCL_INVALID).all() and int(traced.item()) == int(flat.sum())
        got = gather(eng, p, n, ns, tm, variant)
        assert np.array_equal(unpack(got["mask"], ns), vis.reshape(-1, ns)), (name, variant)
        assert np.array_equal(bits(got["dirs"]), bits(d)), (name, variant)
        assert got["traced"] == int(flat.sum())
        assert np.array_equal(got["visible"] + got["occluded"], t.sum(axis=1).astype(np.uint32))


def test_ambient_occlusion(eng):
    MIXED.upload(eng)
    p, n = points("mixed")
    w = want("mixed", 64, "radius")
    tp, tn = torch.from_numpy(p.copy()).to(dev()), torch.from_numpy(n.copy()).to(dev())
    tm = torch.from_numpy(tmax_set("mixed", "radius")).to(dev())
    ao = eng.ambient_occlusion(tp, tn, 64, tm, FIRST, BASE, SEED)
    assert eng.wait() == (0, 0)
    torch.cuda.synchronize()
    vis, occ = w["visible"].astype(F), w["occluded"].astype(F)
    # counts up to 64 are exact in f32; the one division may be off by an ulp on a device
    assert ao.dtype == torch.float32 and ao.shape == (len(p),)
    np.testing.assert_allclose(ao.cpu().numpy(), vis / np.maximum(vis + occ, F(1)), rtol=2.0 ** -22, atol=0)


# ---- 4. split invariance ---------------------------------------------------------------------------------

def test_split_invariance(eng):
    MIXED.upload(eng)
    p, n = points("mixed")
    tm = tmax_set("mixed", "random")
    ns = 100
    w = want("mixed", ns, "random")
    for variant in VARIANTS:
        for cut in (1, 150):  # a point cut: point_base advanced by the cut
            a = gather(eng, p[:cut], n[:cut], ns, tm[:cut], variant)
            b = gather(eng, p[cut:], n[cut:], ns, tm[cut:], variant, base=BASE + cut)
            same(a, w, (variant, cut, "head"), slice(0, cut))
            same(b, w, (variant, cut, "tail"), slice(cut, None))
            assert a["traced"] + b["traced"] == w["traced"]
        a = gather(eng, p, n, 37, tm, variant)  # a sample cut: first_sample advanced by the cut
        b = gather(eng, p, n, 63, tm, variant, first=FIRST + 37)
        for k in ("visible", "occluded"):
            assert np.array_equal(a[k] + b[k], w[k]), (variant, k)
        assert np.array_equal(np.concatenate([unpack(a["mask"], 37), unpack(b["mask"], 63)], axis=1),
                              unpack(w["mask"], ns)), variant
        assert np.array_equal(bits(np.concatenate([a["dirs"], b["dirs"]], axis=1)), bits(w["dirs"]))
        assert a["traced"] + b["traced"] == w["traced"]


# ---- 5. invalid input, what is written -----------------------------------------------------------------------

G = 64  # guard words around every output buffer


def raw_call(eng, p, n, tm, npoints, ns, out, variant=E.ATR_KERNEL_AUTO, first=FIRST, base=BASE, seed=SEED,
             stream=None):
    q = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None  # noqa: E731
    return E.lib().atr_gather_occlusion(eng.h, q(p), q(n), q(tm), npoints, ns, first, base, C.c_uint64(seed),
                                        C.byref(out) if out is not None else None, variant,
                                        C.c_void_p(stream) if stream else None)


def guarded(npoints, ns):
    """The four output buffers with G guard words on both sides, filled with 0xABABABAB, and the
    atr_gather_out that points into them."""
    words = (ns + 31) // 32
    sizes = {"visible": npoints, "occluded": npoints, "mask": npoints * words, "dirs": npoints * ns * 3}
    buf = {k: torch.full((v + 2 * G,), -0x54545455, dtype=torch.int32, device=dev()) for k, v in sizes.items()}
    traced = torch.full((1,), 5, dtype=torch.int64, device=dev())
    ptr = {k: b.data_ptr() + 4 * G for k, b in buf.items()}
    return sizes, buf, traced, ptr


def payload(buf, sizes, k):
    a = buf[k].cpu().numpy().view(np.uint32)
    assert (a[:G] == 0xABABABAB).all() and (a[G + sizes[k]:] == 0xABABABAB).all(), (k, "guard words")
    return a[G:G + sizes[k]]


def test_invalid_points_sit_between_valid_ones(eng):
    MIXED.upload(eng)
    p, n = (a[:200].copy() for a in points("mixed"))
    tm = tmax_set("mixed", "random")[:200].copy()
    p[3, 1] = np.nan
    p[70] = np.inf
    n[9] *= F(1.01)
    n[64:66] = 0
    tm[17], tm[18], tm[19], tm[20], tm[21] = 0.0, -1.0, np.nan, np.inf, 1e-5
    bad = [3, 9, 17, 18, 19, 64, 65, 70]
    for ns in (7, 64):
        w = GR.gather(TR.SCENES["mixed"].oracle(), p, n, ns, tm, FIRST, BASE, SEED)
        for k in ("visible", "occluded", "mask", "flags"):
            assert (w[k][bad] == 0).all()
        assert (bits(w["dirs"][bad]) == 0).all() and w["flags"][[20, 21]].any(axis=1).all()
        assert w["occluded"][21] == 0 and w["visible"][21] > 0  # nothing is accepted below the tolerance
        for variant in VARIANTS:
            got = gather(eng, p, n, ns, tm, variant)
            same(got, w, (ns, variant))
            for k in ("visible", "occluded", "mask"):
                assert (got[k][bad] == 0).all()
            assert (bits(got["dirs"][bad]) == 0).all()


@pytest.mark.parametrize("ns", [7, 64])
def test_only_the_requested_outputs_are_written(eng, ns):
    MIXED.upload(eng)
    npts = 70
    p, n = (a[:npts] for a in points("mixed"))
    tmn = tmax_set("mixed", "random")[:npts]
    w = GR.gather(TR.SCENES["mixed"].oracle(), p, n, ns, tmn, FIRST, BASE, SEED)
    tp, tn, tm = (torch.from_numpy(a.copy()).to(dev()) for a in (p, n, tmn))
    s = torch.cuda.current_stream().cuda_stream
    sizes, buf, traced, ptr = guarded(npts, ns)
    calls = 0
    for variant in VARIANTS:
        for skip in (None,) + ALL + ("traced",):  # every output pointer NULL in turn
            for b in buf.values():
                b.fill_(-0x54545455)
            out = E.atr_gather_out(*[ptr[k] if k != skip else None for k in ALL],
                                   traced.data_ptr() if skip != "traced" else None)
            assert raw_call(eng, tp, tn, tm, npts, ns, out, variant, stream=s) == 0
            assert eng.wait() == (0, 0)
            torch.cuda.synchronize()
            calls += skip != "traced"
            for k in ALL:
                got = payload(buf, sizes, k)
                if k == skip:
                    assert (got == 0xABABABAB).all(), (variant, skip)
                else:
                    assert np.array_equal(got, w[k].view(np.uint32).reshape(-1)), (variant, skip, k)
            assert int(traced.item()) == 5 + calls * w["traced"]  # one accumulator, added to
    # a second call on other points overwrites the counts and the mask instead of adding to them
    out = E.atr_gather_out(*[ptr[k] for k in ALL], None)
    assert raw_call(eng, tp, tn, tm, npts, ns, out, base=BASE + 7, stream=s) == 0
    assert eng.wait() == (0, 0)
    torch.cuda.synchronize()
    w2 = GR.gather(TR.SCENES["mixed"].oracle(), p, n, ns, tmn, FIRST, BASE + 7, SEED)
    assert any((w2[k] != w[k]).any() for k in ("visible", "occluded", "mask"))
    for k in ALL:
        assert np.array_equal(payload(buf, sizes, k), w2[k].view(np.uint32).reshape(-1)), k


# ---- 6. arguments --------------------------------------------------------------------------------------------------

def test_arguments(eng):
    MIXED.upload(eng)
    npts, ns = 9, 7
    p, n = (torch.from_numpy(a[:npts].copy()).to(dev()) for a in points("mixed"))
    tm = torch.from_numpy(tmax_set("mixed", "random")[:npts].copy()).to(dev())
    sizes, buf, traced, ptr = guarded(npts, ns)
    out = E.atr_gather_out(*[ptr[k] for k in ALL], traced.data_ptr())
    inv = -1
    assert raw_call(eng, p, n, tm, npts, ns, None) == inv
    assert raw_call(eng, None, n, tm, npts, ns, out) == inv
    assert raw_call(eng, p, None, tm, npts, ns, out) == inv
    assert raw_call(eng, p, n, tm, -1, ns, out) == inv
    for bad_ns in (0, -1, 65537):
        assert raw_call(eng, p, n, tm, npts, bad_ns, out) == inv
    assert raw_call(eng, p, n, tm, npts, ns, out, first=2 ** 24 - ns + 1) == inv
    assert raw_call(eng, p, n, tm, npts, ns, out, base=-1) == inv
    assert raw_call(eng, p, n, tm, npts, ns, out, base=2 ** 39 - npts + 1) == inv
    assert raw_call(eng, p, n, tm, 2 ** 31 // ns + 1, ns, out) == inv  # npoints x nsamples >= 2^31
    assert raw_call(eng, p, n, tm, 2 ** 15, 65536, out) == inv
    for variant in (E.ATR_KERNEL_HYBRID, E.ATR_KERNEL_PATHS, 2, -1):
        assert raw_call(eng, p, n, tm, npts, ns, out, variant=variant) == inv
    assert raw_call(eng, p, n, tm, 0, ns, out) == 0 and raw_call(eng, None, None, None, 0, ns, None) == 0
    torch.cuda.synchronize()
    for k in ALL:
        assert (payload(buf, sizes, k) == 0xABABABAB).all()
    assert int(traced.item()) == 5  # nothing was written
    w = GR.gather(TR.SCENES["mixed"].oracle(), *(a[:npts] for a in points("mixed")), ns,
                  tmax_set("mixed", "random")[:npts], 2 ** 24 - ns, 2 ** 39 - npts, SEED)
    for variant in (E.ATR_KERNEL_AUTO, E.ATR_KERNEL_FLAT, E.ATR_KERNEL_LANE):  # both ranges at their upper ends
        assert raw_call(eng, p, n, tm, npts, ns, out, variant=variant, first=2 ** 24 - ns, base=2 ** 39 - npts,
                        stream=torch.cuda.current_stream().cuda_stream) == 0
        assert eng.wait() == (0, 0)
        torch.cuda.synchronize()
        for k in ALL:
            assert np.array_equal(payload(buf, sizes, k), w[k].view(np.uint32).reshape(-1)), (variant, k)
    assert int(traced.item()) == 5 + 3 * w["traced"]
    with pytest.raises(ValueError):
        eng.gather_occlusion(p.t().contiguous().t(), n, ns)  # not contiguous
    with pytest.raises(ValueError):
        eng.gather_occlusion(p.double(), n, ns)
    with pytest.raises(ValueError):
        eng.gather_occlusion(p, n[:-1], ns)
    with pytest.raises(ValueError):
        eng.gather_occlusion(p, n, ns, tm.double())
    with pytest.raises(ValueError):
        eng.gather_occlusion(p, n, ns, tm[:-1])
    with pytest.raises(ValueError):
        eng.gather_occlusion(p, n, ns, outputs=("visible", "hits"))
    fresh = E.Engine(0)
    try:
        assert raw_call(fresh, p, n, tm, npts, ns, out) == -4  # ATR_E_NOSCENE
    finally:
        fresh.close()


# ---- 7. streams ------------------------------------------------------------------------------------------------------

def test_two_streams_without_a_wait_between(eng):
    MIXED.upload(eng)
    p, n = points("mixed")
    tm = tmax_set("mixed", "random")
    s1, s2 = torch.cuda.Stream(dev()), torch.cuda.Stream(dev())
    torch.cuda.synchronize()
    a = gather(eng, p, n, 100, tm, stream=s1.cuda_stream, wait=False)
    b = gather(eng, p, n, 64, tm, stream=s2.cuda_stream, wait=False)  # the same head counter, handed over
    c = gather(eng, p, n, 7, tm, E.ATR_KERNEL_LANE, stream=s1.cuda_stream, wait=False)
    rc, done = eng.wait()
    assert (rc, done) == (0, 0) and eng.last_kernel_ms() > 0
    torch.cuda.synchronize()
    same(host(*a[:2]), want("mixed", 100, "random"), "stream 1")
    same(host(*b[:2]), want("mixed", 64, "random"), "stream 2")
    same(host(*c[:2]), want("mixed", 7, "random"), "stream 1 again")
