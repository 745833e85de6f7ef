"""atr_occluded_rays on the GPU, byte for byte against the reference of tests/occlusion_ref.py (the
oracle's walk with its closest distance started at t_max; validated against the oracle alone in
tests/test_occlusion_cpu.py): every scene, batch, t_max set, variant and batch order; wave tails;
the engine's own closest-hit query; model order; cluster sizes; invalid rays and bounds; what is
written; input order; streams; workspace growth; arguments; segments. Needs an MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from tests import occlusion_ref as OR  # noqa: E402
from tests import ray_sets as R  # noqa: E402
from tests import test_gpu_trace_rays as TR  # noqa: E402
from tests.test_gpu_parity import eng, run  # noqa: E402,F401
from tests.test_gpu_scenes import MIXED, ref  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
VARIANTS = (E.ATR_KERNEL_AUTO, E.ATR_KERNEL_LANE)
SORTS = (0, 2, 5, 7)
KINDS = ("aimed", "second", "axis", "inside", "away")

_want = {}


def dev():
    return torch.device("cuda", 0)


def t_ref(name, kind):
    return TR.trace(name, *TR.rays(name, kind), kind)[1]


def tmax_set(name, kind, which):
    """The t_max sets of the parity test (None: the NULL pointer)."""
    t = t_ref(name, kind)
    if which == "null":
        return None
    if which == "max":
        return np.full(len(t), R.MAX_FLOAT, F)
    if which == "t_ref":
        return np.array(t, F)
    if which == "next":
        tm = np.nextafter(np.where(t < R.MAX_FLOAT, t, F(1.0)), F(np.inf)).astype(F)
        tm[t >= R.MAX_FLOAT] = R.MAX_FLOAT
        return tm
    return OR.random_tmax(t)


def want(name, kind, which):
    """The reference's bytes of a batch and t_max set (computed once, read-only)."""
    if (name, kind, which) not in _want:
        orig, dirs = TR.rays(name, kind)
        w = OR.occluded(TR.SCENES[name].oracle(), orig, dirs, tmax_set(name, kind, which))
        w.setflags(write=False)
        _want[name, kind, which] = w
    return _want[name, kind, which]


def occl(eng, orig, dirs, t_max=None, variant=E.ATR_KERNEL_AUTO, sort_bits=-1, stream=None, wait=True):
    """One atr_occluded_rays call: the bytes and the traced-ray count."""
    o = torch.from_numpy(np.array(orig, F)).to(dev())  # copies: the cached batches are read-only
    d = torch.from_numpy(np.array(dirs, F)).to(dev())
    tm = None if t_max is None else torch.from_numpy(np.array(t_max, F)).to(dev())
    out, traced = eng.occluded_rays(o, d, tm, variant=variant, sort_bits=sort_bits, stream=stream)
    if not wait:
        return out, traced, (o, d, tm)
    rc, done = eng.wait()
    assert rc == 0 and done == 0, (rc, done)
    torch.cuda.synchronize()
    return out.cpu().numpy(), int(traced.item())


def same(got, w, what):
    bad = np.flatnonzero(got != w)
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), got[bad[:8]].tolist(), w[bad[:8]].tolist())


# ---- 1. parity -------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", list(TR.SCENES))
def test_parity_with_reference(eng, name, kind):
    TR.SCENES[name].upload(eng)
    orig, dirs = TR.rays(name, kind)
    for which in ("null", "max", "t_ref", "next", "random"):
        tm, w = tmax_set(name, kind, which), want(name, kind, which)
        assert set(np.unique(w).tolist()) <= {0, 1}
        for variant in VARIANTS:
            for sb in (SORTS if which == "random" else (0, 5)):
                got, traced = occl(eng, orig, dirs, tm, variant, sb)
                same(got, w, (name, kind, which, variant, sb))
                assert traced == len(orig), (name, kind, which, variant, sb, traced)


# ---- 2. wave tails -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_parity_at_wave_tails(eng, n):
    MIXED.upload(eng)
    orig, dirs = (a[:n] for a in TR.rays("mixed", "aimed"))
    tm, w = tmax_set("mixed", "aimed", "random")[:n], want("mixed", "aimed", "random")[:n]
    for variant in VARIANTS:
        for sb in SORTS + (-1,):
            got, traced = occl(eng, orig, dirs, tm, variant, sb)
            same(got, w, (n, variant, sb))
            assert traced == n


# ---- 3. the engine against itself -----------------------------------------------------------------------

@pytest.mark.parametrize("name,kind", [("mixed", "aimed"), ("mixed", "second"), ("ties", "aimed"), ("soup", "aimed")])
def test_against_the_closest_hit_query(eng, name, kind):
    TR.SCENES[name].upload(eng)
    orig, dirs = TR.rays(name, kind)
    t = TR.query(eng, orig, dirs, sort_bits=5, outputs=("t",))["t"]
    tm = tmax_set(name, kind, "random")
    for variant in VARIANTS:
        free, _ = occl(eng, orig, dirs, None, variant, 5)
        same(free, (t < R.MAX_FLOAT).astype(np.uint8), (name, kind, variant, "unbounded"))
        got, _ = occl(eng, orig, dirs, tm, variant, 5)
        assert (got[t < tm] == 1).all(), (name, kind, variant)  # closest t < t_max => occluded


# ---- 4. model order ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [(3, 2, 1, 0), (1, 3, 0, 2), (2, 0, 3, 1)])
def test_model_order_does_not_matter(eng, order):
    MIXED.permuted(order).upload(eng)
    for kind in ("aimed", "second"):
        orig, dirs = TR.rays("mixed", kind)
        tm, w = tmax_set("mixed", kind, "random"), want("mixed", kind, "random")  # the unpermuted scene's
        for variant in VARIANTS:
            got, _ = occl(eng, orig, dirs, tm, variant, 5)
            same(got, w, (order, kind, variant))


# ---- 5. cluster sizes ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("cluster_size", [1, 5, 16])
def test_cluster_sizes(eng, cluster_size):
    base = eng.tuning()
    try:
        eng.set_tuning(cluster_size=cluster_size)
        MIXED.upload(eng)  # cluster_size applies at upload
        for kind in ("aimed", "second", "axis"):
            orig, dirs = TR.rays("mixed", kind)
            for which in ("random", "t_ref"):
                for sb in (0, 5):
                    got, _ = occl(eng, orig, dirs, tmax_set("mixed", kind, which), E.ATR_KERNEL_AUTO, sb)
                    same(got, want("mixed", kind, which), (cluster_size, kind, which, sb))
    finally:
        eng.set_tuning(**base)


# ---- 6. invalid input ------------------------------------------------------------------------------------------

def test_invalid_rays_and_bounds(eng):
    MIXED.upload(eng)
    orig, dirs, ok_ray = TR.invalid_batch()  # 320 rays, rows 64..127 and a few more invalid
    n = len(orig)
    t = np.full(n, R.MAX_FLOAT, F)
    t[ok_ray] = TR.SCENES["mixed"].oracle().trace(orig[ok_ray], dirs[ok_ray])[1]
    tm = OR.random_tmax(t, 9)
    rows = {130: np.nan, 131: 0.0, 132: -1.0, 133: -np.inf, 134: np.inf, 135: 1e-5, 136: 1e-40, 137: -0.0}
    for r, v in rows.items():
        tm[r] = F(v)
    tm[192:256] = np.tile(np.array([np.nan, 0.0, -2.5, -np.inf], F), 16)  # a whole wavefront of bad t_max
    bad_t = np.zeros(n, bool)
    bad_t[[130, 131, 132, 133, 137]] = True
    bad_t[192:256] = True
    ok = ok_ray & ~bad_t
    assert ok_ray[list(rows)].all() and ok_ray[192:256].all() and int(ok.sum()) >= 150
    w = np.full(n, E.ATR_OCCL_INVALID, np.uint8)
    w[ok] = OR.occluded(TR.SCENES["mixed"].oracle(), orig[ok], dirs[ok], tm[ok])
    assert (w[[135, 136]] == 0).all() and set(np.unique(w[ok]).tolist()) == {0, 1}
    as_max = tm.copy()
    as_max[134] = R.MAX_FLOAT
    for variant in VARIANTS:
        for sb in SORTS:
            got, traced = occl(eng, orig, dirs, tm, variant, sb)
            same(got, w, (variant, sb))
            assert traced == int(ok.sum()), (variant, sb, traced)
            again, _ = occl(eng, orig, dirs, as_max, variant, sb)
            assert again[134] == got[134] == int(t[134] < R.MAX_FLOAT)  # +inf counts as MAX
        free, traced = occl(eng, orig, dirs, None, variant, 0)  # NULL t_max: the ray test alone
        assert (free[~ok_ray] == E.ATR_OCCL_INVALID).all() and (free[ok_ray] != E.ATR_OCCL_INVALID).all()
        assert traced == int(ok_ray.sum())


# ---- 7. what is written ----------------------------------------------------------------------------------------

def raw_call(eng, o, d, tm, n, out_ptr, traced_ptr, variant=E.ATR_KERNEL_AUTO, sort_bits=0, stream=None):
    p = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None  # noqa: E731
    return E.lib().atr_occluded_rays(eng.h, p(o), p(d), p(tm), n, C.c_void_p(out_ptr) if out_ptr else None,
                                     C.c_void_p(traced_ptr) if traced_ptr else None, variant, sort_bits,
                                     C.c_void_p(stream) if stream else None)


def test_only_the_output_bytes_are_written(eng):
    MIXED.upload(eng)
    orig, dirs = TR.rays("mixed", "aimed")
    n, G = len(orig), 64
    assert n % 4 == 1
    o, d = torch.from_numpy(orig.copy()).to(dev()), torch.from_numpy(dirs.copy()).to(dev())
    tm = torch.from_numpy(tmax_set("mixed", "aimed", "random")).to(dev())
    buf = torch.full((n + 2 * G,), 0xAB, dtype=torch.uint8, device=dev())
    traced = torch.full((1,), 5, dtype=torch.int64, device=dev())
    s = torch.cuda.current_stream().cuda_stream
    calls = 0
    for variant in VARIANTS:
        for sb in (0, 5):
            buf.fill_(0xAB)
            assert raw_call(eng, o, d, tm, n, buf.data_ptr() + G, traced.data_ptr(), variant, sb, s) == 0
            assert eng.wait() == (0, 0)
            torch.cuda.synchronize()
            calls += 1
            got = buf.cpu().numpy()
            assert (got[:G] == 0xAB).all() and (got[G + n:] == 0xAB).all(), (variant, sb)
            same(got[G:G + n], want("mixed", "aimed", "random"), (variant, sb))
            assert int(traced.item()) == 5 + calls * n  # one accumulator, added to
    buf.fill_(0xAB)
    assert raw_call(eng, o, d, tm, n, buf.data_ptr() + G, None, sort_bits=5, stream=s) == 0  # no counter
    assert eng.wait() == (0, 0)
    torch.cuda.synchronize()
    same(buf.cpu().numpy()[G:G + n], want("mixed", "aimed", "random"), "no traced_rays")


# ---- 8. input order ----------------------------------------------------------------------------------------------

def test_results_do_not_depend_on_batch_order(eng):
    MIXED.upload(eng)
    orig = np.concatenate([TR.rays("mixed", k)[0] for k in ("aimed", "second", "away")])
    dirs = np.concatenate([TR.rays("mixed", k)[1] for k in ("aimed", "second", "away")])
    tm = np.concatenate([tmax_set("mixed", k, "random") for k in ("aimed", "second", "away")])
    w = np.concatenate([want("mixed", k, "random") for k in ("aimed", "second", "away")])
    perm = np.random.default_rng(31).permutation(len(orig))
    for variant in VARIANTS:
        for sb in SORTS:
            a, _ = occl(eng, orig, dirs, tm, variant, sb)
            b, tb = occl(eng, orig[perm], dirs[perm], tm[perm], variant, sb)
            same(a, w, (variant, sb))
            same(b, w[perm], (variant, sb, "permuted"))
            assert tb == len(orig)


# ---- 9. streams ----------------------------------------------------------------------------------------------------

def test_two_streams_with_a_render_and_a_ray_query_between(eng):
    MIXED.upload(eng)
    W, H = 96, 72
    s1, s2 = torch.cuda.Stream(dev()), torch.cuda.Stream(dev())
    a, b = TR.rays("mixed", "aimed"), TR.rays("mixed", "second")
    ta, tb = tmax_set("mixed", "aimed", "random"), tmax_set("mixed", "second", "random")
    wa, wb = want("mixed", "aimed", "random"), want("mixed", "second", "random")
    torch.cuda.synchronize()
    ra = occl(eng, *a, ta, sort_bits=5, stream=s1.cuda_stream, wait=False)
    assert eng.wait()[0] == 0 and eng.last_kernel_ms() > 0
    r = run(eng, E.camera(W, H, 2, 3))
    q = TR.query(eng, *b, sort_bits=5, stream=s2.cuda_stream, wait=False)  # the same workspace
    rb = occl(eng, *b, tb, sort_bits=5, stream=s2.cuda_stream, wait=False)
    assert eng.wait()[0] == 0 and eng.last_kernel_ms() > 0
    torch.cuda.synchronize()
    same(ra[0].cpu().numpy(), wa, "stream 1")
    same(rb[0].cpu().numpy(), wb, "stream 2")
    TR.assert_parity(TR.host(*q[:2]), TR.trace("mixed", *b, "second"), "the ray query between")
    want_r = ref(MIXED, W, H, 2, 3)
    assert np.array_equal(r["fb"], want_r["fb"]) and np.array_equal(r["casts"], want_r["casts"])
    # back to back on two streams without a wait between: the shared workspace is handed over on the GPU
    ra = occl(eng, *a, ta, sort_bits=5, stream=s1.cuda_stream, wait=False)
    q = TR.query(eng, *b, sort_bits=2, stream=s2.cuda_stream, wait=False)
    rb = occl(eng, *b, tb, sort_bits=2, stream=s1.cuda_stream, wait=False)
    rc = occl(eng, *a, ta, sort_bits=7, stream=s2.cuda_stream, wait=False)
    assert eng.wait()[0] == 0
    torch.cuda.synchronize()
    same(ra[0].cpu().numpy(), wa, "stream 1 again")
    same(rb[0].cpu().numpy(), wb, "stream 1, after the ray query on stream 2")
    same(rc[0].cpu().numpy(), wa, "stream 2 again")
    TR.assert_parity(TR.host(*q[:2]), TR.trace("mixed", *b, "second"), "the ray query, back to back")
    assert int(ra[1].item()) == len(a[0]) and int(rb[1].item()) == len(b[0])


# ---- 10. workspace growth -----------------------------------------------------------------------------------------------

def test_workspace_growth():
    orig, dirs = TR.rays("mixed", "aimed")
    tm, w = tmax_set("mixed", "aimed", "random"), want("mixed", "aimed", "random")
    a = E.Engine(0)
    try:
        MIXED.upload(a)
        ws0 = a.workspace_info()
        small, _ = occl(a, orig[:64], dirs[:64], tm[:64], sort_bits=2)
        same(small, w[:64], "64 rays")
        grown, traced = occl(a, orig, dirs, tm, sort_bits=5)  # more rays and more bins than the workspace holds
        same(grown, w, "4097 rays after 64")
        assert traced == len(orig)
        again, _ = occl(a, orig[:64], dirs[:64], tm[:64], sort_bits=2)  # a small batch in the grown workspace
        same(again, w[:64], "64 rays again")
        assert a.workspace_info() == ws0  # the path workspaces' report is what it was
    finally:
        a.close()


# ---- 11. arguments --------------------------------------------------------------------------------------------------------

def test_arguments(eng):
    MIXED.upload(eng)
    n = 65
    orig, dirs = (a[:n] for a in TR.rays("mixed", "aimed"))
    o, d = torch.from_numpy(np.array(orig, F)).to(dev()), torch.from_numpy(np.array(dirs, F)).to(dev())
    tm = torch.from_numpy(tmax_set("mixed", "aimed", "random")[:n].copy()).to(dev())
    out = torch.full((n,), 0xAB, dtype=torch.uint8, device=dev())
    traced = torch.full((1,), 5, dtype=torch.int64, device=dev())
    op, tp, inv = out.data_ptr(), traced.data_ptr(), -1
    assert raw_call(eng, o, d, tm, n, None, tp) == inv
    assert raw_call(eng, None, d, tm, n, op, tp) == inv
    assert raw_call(eng, o, None, tm, n, op, tp) == inv
    assert raw_call(eng, o, d, tm, -1, op, tp) == inv
    assert raw_call(eng, o, d, tm, 2 ** 31, op, tp) == inv
    for variant in (E.ATR_KERNEL_HYBRID, E.ATR_KERNEL_PATHS, 2, -1):
        assert raw_call(eng, o, d, tm, n, op, tp, variant=variant) == inv
    for sb in (1, 8, -2, 64):
        assert raw_call(eng, o, d, tm, n, op, tp, sort_bits=sb) == inv
    assert raw_call(eng, o, d, tm, 0, op, tp) == 0 and raw_call(eng, None, None, None, 0, None, None) == 0
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xAB).all() and int(traced.item()) == 5  # nothing was written
    for variant in (E.ATR_KERNEL_AUTO, E.ATR_KERNEL_FLAT, E.ATR_KERNEL_LANE):
        for sb in (-1, 0, 2, 7):
            assert raw_call(eng, o, d, tm, n, op, tp, variant=variant, sort_bits=sb,
                            stream=torch.cuda.current_stream().cuda_stream) == 0
    assert eng.wait() == (0, 0)
    torch.cuda.synchronize()
    assert int(traced.item()) == 5 + 12 * n
    same(out.cpu().numpy(), want("mixed", "aimed", "random")[:n], "after the valid calls")
    with pytest.raises(ValueError):
        eng.occluded_rays(o.t().contiguous().t(), d)  # not contiguous
    with pytest.raises(ValueError):
        eng.occluded_rays(o.double(), d)
    with pytest.raises(ValueError):
        eng.occluded_rays(o, d, tm.double())
    with pytest.raises(ValueError):
        eng.occluded_rays(o, d, tm[:-1])
    with pytest.raises(ValueError):
        eng.occluded_rays(o, d, torch.stack([tm, tm], 1)[:, 0])  # not contiguous
    fresh = E.Engine(0)
    try:
        assert raw_call(fresh, o, d, tm, n, op, tp) == -4  # ATR_E_NOSCENE
    finally:
        fresh.close()


# ---- 12. segments ------------------------------------------------------------------------------------------------------------

def test_segments_to_two_lights_in_both_directions(eng):
    MIXED.upload(eng)
    orig, dirs = TR.rays("mixed", "aimed")
    t = t_ref("mixed", "aimed")
    hit = t < R.MAX_FLOAT
    pts = (orig[hit] + dirs[hit] * t[hit][:, None]).astype(F)  # points on the scene's surfaces
    box = TR.boxes("mixed")[0]
    ctr, ext = (box[:3] + box[3:]) * F(0.5), box[3:] - box[:3]
    sc = TR.SCENES["mixed"].oracle()
    seen = []
    for light in (ctr + ext * np.array([0.0, 0.9, 0.0], F), ctr + ext * np.array([0.7, 0.6, 0.8], F)):
        lights = np.broadcast_to(light.astype(F), pts.shape).copy()
        lights[5] = pts[5]  # a degenerate segment
        for p, q in ((pts, lights), (lights, pts)):
            tp, tq = torch.from_numpy(p).to(dev()), torch.from_numpy(q).to(dev())
            o, d, tm = (a.cpu().numpy() for a in E.segment_rays(tp, tq))
            ok = R.passes(o, d)
            assert not ok[5] and ok.sum() == len(p) - 1
            w = np.full(len(p), E.ATR_OCCL_INVALID, np.uint8)
            w[ok] = OR.occluded(sc, o[ok], d[ok], tm[ok])
            for variant in VARIANTS:
                got, traced = eng.occluded_segments(tp, tq, variant=variant, sort_bits=5)
                assert eng.wait() == (0, 0)
                torch.cuda.synchronize()
                same(got.cpu().numpy(), w, (light.tolist(), variant))
                assert int(traced.item()) == int(ok.sum())
            seen.append(float((w[ok] == 1).mean()))
    print("occluded shares", seen)
    assert min(seen) < 1.0 and max(seen) > 0.0  # some segments are blocked, some reach
