"""atr_denoise_variance on the GPU: `out`, `variance_out` and `framebuffer` for exact equality with the
plain C reference of tests/denoise_variance_ref.py (pinned without a GPU in
tests/test_denoise_variance_cpu.py), at the edges of the kernels' 64 x 4 blocks, for every guide subset,
pass count and term, with the spatial estimate on and off, inert pixels and bad variances of every kind,
in place, on two streams and beside an atr_denoise, through a growing workspace, and end to end on
rendered frames with TemporalAccumulator.filtered; the arguments. Every raw output buffer is filled with a
sentinel first and guarded on both sides. Needs an MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from tests import accumulate_ref as AR  # noqa: E402
from tests import denoise_ref as DR  # noqa: E402
from tests import denoise_variance_ref as VR  # noqa: E402
from tests.test_accumulate_cpu import orbit  # noqa: E402
from tests.test_denoise_cpu import scene  # noqa: E402
from tests.test_denoise_variance_cpu import extras  # noqa: E402
from tests.test_gpu_parity import eng, run, upload  # noqa: E402,F401

pytestmark = pytest.mark.gpu
F = np.float32
G = 256  # guard bytes around every raw output buffer
FILL = 0xAB
EMPTY = np.uint32(0xFFFFFFFF)
ON = dict(sigma_luminance=2.0, luminance_floor=1e-3, sigma_position=0.4, normal_power_log2=3)
OUTS = (("out", 12, F), ("vout", 4, F), ("fb", 4, np.uint32))


def dev():
    return torch.device("cuda", 0)


def up(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev())


def raw(eng, color, var, normal=None, position=None, ident=None, moments=None, length=None,  # noqa: F811
        want=("out", "vout", "fb"), guides=True, stream=None, params=None, size=None, **kw):
    """atr_denoise_variance through ctypes on guarded, sentinel-filled buffers: (rc, out, variance_out,
    framebuffer), None for an output that was not asked for or after an error."""
    h, w = color.shape[:2] if size is None else size
    t = [up(a) for a in (color, var, normal, position, ident, moments, length)]
    n = color.shape[0] * color.shape[1]
    buf = {k: torch.full((n * per + 2 * G,), FILL, dtype=torch.uint8, device=dev()) for k, per, _ in OUTS}
    g = E.atr_denoise_guides(*[a.data_ptr() if a is not None else None for a in t[2:5]])
    p = params
    if p is None:
        d = dict(VR.DEFAULTS, **kw)
        p = E.atr_denoise_variance_params(d["passes"], d["sigma_luminance"], d["luminance_floor"], d["sigma_position"],
                                          d["normal_power_log2"], d["spatial_below"])
    vp = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None  # noqa: E731
    at = lambda k: C.c_void_p(buf[k].data_ptr() + G) if k in want else None  # noqa: E731
    torch.cuda.synchronize()
    rc = E.lib().atr_denoise_variance(eng.h, vp(t[0]), vp(t[1]), C.byref(g) if guides else None, vp(t[5]), vp(t[6]), w, h,
                                      C.byref(p) if p else None, at("out"), at("vout"), at("fb"),
                                      C.c_void_p(stream) if stream else None)
    wrc, done = eng.wait()
    assert wrc == 0 and done == 0
    torch.cuda.synchronize()
    res = []
    for k, per, dt in OUTS:
        a = buf[k].cpu().numpy()
        assert (a[:G] == FILL).all() and (a[G + n * per:] == FILL).all(), (k, "guard bytes")
        body = a[G:G + n * per]
        if rc != 0 or k not in want:
            assert (body == FILL).all(), (k, "written")
            res.append(None)
        else:
            res.append(body.view(dt).reshape(color.shape if k == "out" else color.shape[:2]).copy())
    return (rc,) + tuple(res)


def check(eng, color, var, *rest, **kw):  # noqa: F811
    rc, out, vout, fb = raw(eng, color, var, *rest, **kw)
    assert rc == 0
    want, wv, wfb = VR.denoise_variance(color, var, *rest, **kw)
    assert DR.same_bits(out, want)
    assert DR.same_bits(vout, wv)
    assert np.array_equal(fb, wfb)
    return out, vout


def everything(h, w, seed, nan=True):
    return scene(h, w, seed=seed, nan=nan) + extras(h, w, seed, nan=nan)


# 63/64/65 and 3/4/5: one below, at and one above the kernels' block of 64 x 4 pixels; from 7 pixels on
# a side some pixels lie outside the estimate's 3-pixel border and some inside
@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (7, 1), (5, 5), (63, 3), (64, 4), (65, 5), (64, 3), (65, 4), (129, 9),
                                 (130, 67)])
def test_sizes(eng, w, h):  # noqa: F811
    color, normal, position, ident, var, moments, length = everything(h, w, w * 131 + h)
    out, vout = check(eng, color, var, normal, position, ident, moments, length, passes=3, **ON)
    if w * h > 1:
        assert not DR.same_bits(out, color) and not DR.same_bits(vout, var)
    check(eng, color, var, passes=2)


def test_eight_passes_on_a_larger_image(eng):  # noqa: F811
    color, normal, position, ident, var, moments, length = everything(131, 257, 9)
    check(eng, color, var, normal, position, ident, moments, length, passes=8, **ON)


@pytest.mark.parametrize("passes", range(1, 9))
def test_pass_counts(eng, passes):  # noqa: F811
    color, normal, position, ident, var, moments, length = everything(33, 65, 12)
    check(eng, color, var, normal, position, ident, moments, length, passes=passes, **ON)


@pytest.mark.parametrize("subset", range(8))
def test_every_guide_subset_with_the_luminance_term_on_and_off(eng, subset):  # noqa: F811
    color, normal, position, ident, var, moments, length = everything(33, 65, 11)
    g = (normal if subset & 1 else None, position if subset & 2 else None, ident if subset & 4 else None)
    kw = dict(passes=3, sigma_position=0.4, normal_power_log2=3)
    outs = [check(eng, color, var, *g, moments, length, sigma_luminance=sl, **kw)[0] for sl in (0.0, 2.0)]
    assert not DR.same_bits(outs[0], outs[1])
    # and without the estimate (the estimate kernel is not launched)
    check(eng, color, var, *g, sigma_luminance=2.0, **kw)


def test_the_estimate_on_off_and_on_mixed_lengths(eng):  # noqa: F811
    color, normal, position, ident, var, moments, length = everything(37, 70, 13)
    assert (length < 4).any() and (length >= 4).any() and (length == 0).any()
    kw = dict(passes=2, **ON)
    on, von = check(eng, color, var, normal, position, ident, moments, length, **kw)
    off, voff = check(eng, color, var, normal, position, ident, moments, length, spatial_below=0, **kw)
    none, vnone = check(eng, color, var, normal, position, ident, **kw)
    assert DR.same_bits(off, none) and DR.same_bits(voff, vnone) and not DR.same_bits(von, voff)
    # every history long enough: the estimate runs and changes nothing
    long_, vlong = check(eng, color, var, normal, position, ident, moments, np.full_like(length, 4), **kw)
    assert DR.same_bits(long_, none) and DR.same_bits(vlong, vnone)
    # length 1 everywhere with a zero variance, as a history's first frame has; a larger threshold
    check(eng, color, np.zeros_like(var), normal, position, ident, moments, np.ones_like(length), **kw)
    check(eng, color, var, normal, position, ident, moments, length, spatial_below=1 << 24, **kw)
    # without normals (the Euclidean position term) and without guides
    check(eng, color, var, None, position, ident, moments, length, **kw)
    check(eng, color, var, None, None, None, moments, length, **kw)


@pytest.mark.parametrize("power", [0, 7])
def test_normal_powers(eng, power):  # noqa: F811
    color, normal, position, ident, var, moments, length = everything(33, 65, 14)
    check(eng, color, var, normal, position, ident, moments, length, passes=3, sigma_luminance=2.0, sigma_position=0.4,
          normal_power_log2=power)


def test_inert_images(eng):  # noqa: F811
    color, normal, position, ident, var, moments, length = everything(19, 70, 15, nan=False)
    # all inert: the input comes back, the variance is 0
    out, vout = check(eng, color, var, normal, position, np.full_like(ident, EMPTY), moments, length, passes=4, **ON)
    assert DR.same_bits(out, color) and (vout == 0).all()
    # one live pixel: it is its own only tap
    one = np.full_like(ident, EMPTY)
    one[7, 33] = 5
    check(eng, color, var, normal, position, one, moments, length, passes=4, **ON)
    # a checkerboard of two ids: at spacing 1 only every other tap counts
    yy, xx = np.mgrid[0:19, 0:70]
    board = ((xx + yy) & 1).astype(np.uint32) + 7
    check(eng, color, var, normal, position, board, moments, length, passes=3, **ON)


@pytest.mark.parametrize("where", ["color", "normal", "position"])
def test_nan_and_inf_in_each_input(eng, where):  # noqa: F811
    color, normal, position, ident, var, moments, length = everything(19, 70, 16, nan=False)
    g = {"color": color, "normal": normal, "position": position}
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        g[where][3 + 5 * k, 10 + 20 * k, k] = bad
    out, vout = check(eng, color, var, normal, position, ident, moments, length, passes=4, **ON)
    for k in range(3):
        assert DR.same_bits(out[3 + 5 * k, 10 + 20 * k], color[3 + 5 * k, 10 + 20 * k]) and vout[3 + 5 * k, 10 + 20 * k] == 0
    live = np.isfinite(color).all(2) & np.isfinite(normal).all(2) & np.isfinite(position).all(2)
    assert np.isfinite(out[live]).all() and np.isfinite(vout).all()


def test_bad_variances_and_moments(eng):  # noqa: F811
    color, normal, position, ident, var, moments, length = everything(19, 70, 17, nan=False)
    for k, bad in enumerate((0.0, np.nan, np.inf, -np.inf, -0.25)):
        var[2 + 3 * k, 5 + 12 * k] = bad
    moments[4, 4, 0], moments[9, 40, 1], moments[15, 66, 0] = np.nan, np.inf, -np.inf
    out, vout = check(eng, color, var, normal, position, ident, moments, length, passes=3, **ON)
    assert np.isfinite(out).all() and np.isfinite(vout).all() and (vout >= 0).all()
    check(eng, color, np.full_like(var, np.nan), normal, position, ident, passes=2, **ON)
    check(eng, color, np.zeros_like(var), normal, position, ident, passes=2, **ON)


def test_in_place_and_optional_outputs(eng):  # noqa: F811
    color, normal, position, ident, var, moments, length = everything(37, 101, 18)
    kw = dict(passes=4, **ON)
    want, wv, wfb = VR.denoise_variance(color, var, normal, position, ident, moments, length, **kw)
    tc, tv, tn, tp, ti, tm, tl = (up(a) for a in (color, var, normal, position, ident, moments, length))
    sep, vsep, fb = eng.denoise_variance(tc, tv, tn, tp, ti, tm, tl, variance_out=True, framebuffer=True, **kw)
    same, vsame = eng.denoise_variance(tc, tv, tn, tp, ti, tm, tl, out=tc, variance_out=tv, **kw)  # both in place
    rc, _ = eng.wait()
    assert rc == 0
    torch.cuda.synchronize()
    assert same.data_ptr() == tc.data_ptr() and vsame.data_ptr() == tv.data_ptr()
    assert DR.same_bits(sep.cpu().numpy(), want) and DR.same_bits(tc.cpu().numpy(), want)
    assert DR.same_bits(vsep.cpu().numpy(), wv) and DR.same_bits(tv.cpu().numpy(), wv)
    assert np.array_equal(fb.cpu().numpy().view(np.uint32), wfb)
    # variance_out NULL; the framebuffer alone; guides NULL equals a guides record of three NULLs
    rc, out, vout, fb = raw(eng, color, var, normal, position, ident, moments, length, want=("out", "fb"), **kw)
    assert rc == 0 and vout is None and DR.same_bits(out, want) and np.array_equal(fb, wfb)
    rc, out, vout, fb = raw(eng, color, var, normal, position, ident, moments, length, want=("fb",), **kw)
    assert rc == 0 and out is None and vout is None and np.array_equal(fb, wfb)
    rc, out, vout, fb = raw(eng, color, var, normal, position, ident, moments, length, want=("out",), **kw)
    assert rc == 0 and fb is None and DR.same_bits(out, want)
    w3 = VR.denoise_variance(color, var, passes=3)
    rc, out, vout, fb = raw(eng, color, var, guides=False, passes=3)
    assert rc == 0 and DR.same_bits(out, w3[0]) and DR.same_bits(vout, w3[1]) and np.array_equal(fb, w3[2])
    one = eng.denoise_variance(up(color), up(var), passes=3)  # the plain return value
    eng.wait()
    torch.cuda.synchronize()
    assert DR.same_bits(one.cpu().numpy(), w3[0])


def test_two_streams_a_growing_workspace_and_an_atr_denoise_beside_it(eng):  # noqa: F811
    """On a fresh context: the second, larger call grows the workspace behind the first; the third (small
    again, on the first stream) waits for the second on the GPU; an atr_denoise on the other stream
    between them has a workspace of its own."""
    e2 = E.Engine(0)
    try:
        a, b = everything(21, 50, 19), everything(90, 333, 20)
        kw = dict(passes=5, **ON)
        dk = dict(passes=5, sigma_color=0.8, sigma_position=0.4, normal_power_log2=3)
        s1, s2 = torch.cuda.Stream(device=dev()), torch.cuda.Stream(device=dev())
        order = lambda x: (x[0], x[4], x[1], x[2], x[3], x[5], x[6])  # noqa: E731  color, variance, guides, history
        ta, tb = [up(x) for x in order(a)], [up(x) for x in order(b)]
        torch.cuda.synchronize()
        o1 = e2.denoise_variance(*ta, variance_out=True, stream=s1.cuda_stream, **kw)
        d1 = e2.denoise(tb[0], tb[2], tb[3], tb[4], stream=s2.cuda_stream, **dk)
        o2 = e2.denoise_variance(*tb, variance_out=True, stream=s2.cuda_stream, **kw)
        d2 = e2.denoise(ta[0], ta[2], ta[3], ta[4], stream=s1.cuda_stream, **dk)
        o3 = e2.denoise_variance(*ta, variance_out=True, stream=s1.cuda_stream, **kw)
        rc, done = e2.wait()
        assert rc == 0 and done == 0
        assert 0 < e2.last_kernel_ms() < 1000
        torch.cuda.synchronize()
        wa, wb = VR.denoise_variance(*order(a), **kw), VR.denoise_variance(*order(b), **kw)
        for got, want in ((o1, wa), (o2, wb), (o3, wa)):
            assert DR.same_bits(got[0].cpu().numpy(), want[0]) and DR.same_bits(got[1].cpu().numpy(), want[1])
        assert DR.same_bits(d1.cpu().numpy(), DR.denoise(*b[:4], **dk)[0])
        assert DR.same_bits(d2.cpu().numpy(), DR.denoise(*a[:4], **dk)[0])
    finally:
        e2.close()


def test_invalid_arguments_leave_the_outputs_untouched(eng):  # noqa: F811
    color, normal, position, ident, var, moments, length = everything(9, 12, 21)
    P = E.atr_denoise_variance_params

    def bad(**kw):
        args = dict(normal=normal, position=position, ident=ident, moments=moments, length=length)
        args.update(kw)
        return raw(eng, color, var, **args)[0]  # raw() asserts the sentinels

    inv = -1  # ATR_E_INVALID
    assert bad(passes=3) == 0
    for p in (0, 9, -1):
        assert bad(passes=p) == inv
    for k in (-1, 8):
        assert bad(normal_power_log2=k) == inv
    for k in (-1, (1 << 24) + 1):
        assert bad(spatial_below=k) == inv
    for s in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert bad(sigma_luminance=s) == inv
        assert bad(sigma_position=s) == inv
        assert bad(luminance_floor=s) == inv
    assert bad(luminance_floor=0.0) == inv
    assert bad(sigma_position=1e-30) == inv and bad(sigma_position=1e30) == inv  # kp infinite, zero
    assert bad(passes=1, sigma_position=1e18) == 0 and bad(passes=8, sigma_position=1e18) == inv
    assert bad(sigma_position=1e-30, position=None) == 0  # the term is off without the guide
    assert bad(sigma_position=-1.0, position=None) == inv
    for k in range(2):
        r = (C.c_int32 * 2)()
        r[k] = 1
        assert bad(params=P(3, 2.0, 1e-3, 0.0, 5, 4, r)) == inv
    assert bad(want=()) == inv and bad(want=("vout",)) == inv  # out and framebuffer both NULL
    assert bad(moments=None) == inv and bad(length=None) == inv and bad(moments=None, length=None) == 0
    for size in [(0, 12), (9, 0), (-1, 12), (16385, 12), (9, 16385)]:
        assert bad(size=size) == inv
    # NULL ctx, params, color, variance
    t, v = up(color), up(var)
    o = torch.full((9 * 12 * 3,), 7.0, dtype=torch.float32, device=dev())
    p = P(3, 2.0, 1e-3, 0.0, 5, 4)
    f = E.lib().atr_denoise_variance
    vp = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731
    assert f(None, vp(t), vp(v), None, None, None, 12, 9, C.byref(p), vp(o), None, None, None) == inv
    assert f(eng.h, None, vp(v), None, None, None, 12, 9, C.byref(p), vp(o), None, None, None) == inv
    assert f(eng.h, vp(t), None, None, None, None, 12, 9, C.byref(p), vp(o), None, None, None) == inv
    assert f(eng.h, vp(t), vp(v), None, None, None, 12, 9, None, vp(o), None, None, None) == inv
    torch.cuda.synchronize()
    assert (o == 7.0).all()
    with pytest.raises(ValueError):
        eng.denoise_variance(t.reshape(9, 12 * 3), v)
    with pytest.raises(ValueError):
        eng.denoise_variance(t, v.reshape(12, 9))
    with pytest.raises(ValueError):
        eng.denoise_variance(t, v, normal=t[:, :6].contiguous())
    with pytest.raises(ValueError):
        eng.denoise_variance(t, v, ident=torch.zeros((9, 12), dtype=torch.int64, device=dev()))
    with pytest.raises(ValueError):
        eng.denoise_variance(t, v, moments=up(moments))
    with pytest.raises(ValueError):
        eng.denoise_variance(t.cpu(), v)
    with pytest.raises(ValueError):
        E.TemporalAccumulator(eng).filtered()
    with pytest.raises(ValueError):
        E.TemporalAccumulator(eng).filtered(radius=3)


def test_rendered_frames_accumulated_and_filtered_end_to_end(eng):  # noqa: F811
    """The Monkey at 72 x 40 from three consecutive cameras of the 0.02-rad orbit, 1 spp and 3 bounces,
    through TemporalAccumulator.push and then filtered(): the image equals the composed references
    (accumulate_ref three times, then denoise_variance_ref on its colour, variance, moments, length and
    the last guides), and the history is as the pushes left it."""
    upload(eng, "Monkey")
    w, h = 72, 40
    acc = E.TemporalAccumulator(eng)
    prev = None
    for f in range(3):
        eye, facing = orbit(f, 0.02)
        cam = E.camera(w, h, 1, 3, eye=eye, facing=facing)
        frame = run(eng, cam)
        g = eng.render_guides(cam)
        acc.push(cam, torch.from_numpy(frame["rgb"]).to(dev()), g)
        rc, _ = eng.wait()
        assert rc == 0
        torch.cuda.synchronize()
        gn = (g[0].cpu().numpy(), g[1].cpu().numpy(), g[2].cpu().numpy().view(np.uint32))
        want = AR.accumulate(frame["rgb"], gn, prev)
        prev = AR.history(want, cam, gn)
    got, fb = acc.filtered(framebuffer=True)
    plain = acc.filtered(sigma_luminance=2.0, passes=2, spatial_below=0)
    rc, _ = eng.wait()
    assert rc == 0
    torch.cuda.synchronize()
    args = (want["color"], want["variance"], *gn, want["moments"], want["length"])
    ref = VR.denoise_variance(*args)
    assert DR.same_bits(got.cpu().numpy(), ref[0]) and np.array_equal(fb.cpu().numpy().view(np.uint32), ref[2])
    assert DR.same_bits(plain.cpu().numpy(), VR.denoise_variance(*args, sigma_luminance=2.0, passes=2, spatial_below=0)[0])
    hit = frame["face"] != E.MISS
    assert 100 < hit.sum() < hit.size
    assert set(np.unique(want["length"][hit])) >= {1, 3}  # short and long histories side by side
    assert DR.same_bits(ref[0][~hit], want["color"][~hit]) and not DR.same_bits(ref[0][hit], want["color"][hit])
    # the history is untouched
    assert AR.same_bits(acc.prev["color"].cpu().numpy(), want["color"])
    assert AR.same_bits(acc.prev["moments"].cpu().numpy(), want["moments"])
    assert AR.same_bits(acc.variance.cpu().numpy(), want["variance"])
