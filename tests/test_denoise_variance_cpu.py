"""The variance-guided denoiser's plain C reference (tests/denoise_variance_ref.py) pinned without a GPU,
so that it is not its own only witness: a vectorised numpy-f32 restatement of include/atray.h's formulas
tap by tap, values worked by hand with exact binary numbers, the variance's sanitisation, the inert
rules, the spatial estimate, the argument rules through the host-only atr_denoise_variance_check, the
defaults, and the two conditions that set the defaults."""
import ctypes as C

import numpy as np
import pytest

from tests import denoise_ref as DR
from tests import denoise_variance_ref as VR
from tests.test_denoise_cpu import np_framebuffer, scene

F = np.float32
H5 = [F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625)]
G3 = [F(0.25), F(0.5), F(0.25)]
EMPTY = np.uint32(0xFFFFFFFF)
ONE = F(1.0)


def np_lum(c):
    return (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]


def np_denoise_variance(color, variance, normal=None, position=None, ident=None, moments=None, length=None, **params):
    """atray.h's formulas on whole images, one tap at a time in the stated order; every numpy f32
    operation is separately rounded. Returns (out, variance_out)."""
    kw = dict(VR.DEFAULTS, **params)
    cur = np.array(color, F)
    h, w = cur.shape[:2]
    fin = lambda a: np.isfinite(a).all(axis=2)  # noqa: E731
    inert = ~fin(cur)
    if ident is not None:
        ident = np.asarray(ident).view(np.uint32)
        inert |= ident == EMPTY
    if normal is not None:
        inert |= ~fin(normal)
    if position is not None:
        inert |= ~fin(position)
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]  # noqa: E731
    Y, X = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    pos_on = position is not None and kw["sigma_position"] > 0
    lum_on = kw["sigma_luminance"] > 0

    def tap(dx, dy):
        qx, qy = X + dx, Y + dy
        ok = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
        qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
        ok &= ~inert[qy, qx]
        if ident is not None:
            ok &= ident[qy, qx] == ident
        return ok, qy, qx

    def guide_terms(wt, qy, qx, kp):
        if normal is not None:
            c = dot(normal, normal[qy, qx])
            c = np.where(c > 0, c, F(0.0))
            for _ in range(kw["normal_power_log2"]):
                c = c * c
            wt = wt * c
        if pos_on:
            dv = position[qy, qx] - position
            if normal is not None:
                e = dot(normal, dv)
                e2 = e * e
            else:
                e2 = dot(dv, dv)
            wt = wt * (ONE / (ONE + e2 * kp))
        return wt

    def kp_of(p):
        sp = F(kw["sigma_position"]) * F(1 << p)
        return ONE / (sp * sp)

    with np.errstate(all="ignore"):
        v = np.array(variance, F)
        v = np.where(~inert & (v > 0) & (v < np.inf), v, F(0.0)).astype(F)
        if moments is not None and kw["spatial_below"] > 0:
            length = np.asarray(length).view(np.uint32)
            a, b, ws = np.zeros((h, w), F), np.zeros((h, w), F), np.zeros((h, w), F)
            for dy in range(-3, 4):
                for dx in range(-3, 4):
                    ok, qy, qx = tap(dx, dy)
                    m = moments[qy, qx]
                    ok &= np.isfinite(m).all(axis=2)
                    wt = guide_terms(np.ones((h, w), F), qy, qx, kp_of(0))
                    use = ok & (wt > 0)
                    a = np.where(use, a + m[..., 0] * wt, a)
                    b = np.where(use, b + m[..., 1] * wt, b)
                    ws = np.where(use, ws + wt, ws)
            m1, m2 = a / ws, b / ws
            e = m2 - m1 * m1
            e = np.where(e > 0, e, F(0.0))
            lp = np.where(length > 0, length, 1).astype(F)
            est = e * (F(kw["spatial_below"]) / lp)
            v = np.where(~inert & (length < np.uint32(kw["spatial_below"])) & (ws > 0), est, v).astype(F)
        for p in range(kw["passes"]):
            s = 1 << p
            rl = None
            if lum_on:
                gs, ks = np.zeros((h, w), F), np.zeros((h, w), F)
                for dy in range(-1, 2):
                    for dx in range(-1, 2):
                        ok, qy, qx = tap(dx, dy)
                        k = G3[dy + 1] * G3[dx + 1]
                        gs = np.where(ok, gs + v[qy, qx] * k, gs)
                        ks = np.where(ok, ks + k, ks)
                gv = gs / ks
                rl = ONE / (F(kw["sigma_luminance"]) * np.sqrt(gv) + F(kw["luminance_floor"]))
            lum = np_lum(cur)
            total, vs, wsum = np.zeros((h, w, 3), F), np.zeros((h, w), F), np.zeros((h, w), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    ok, qy, qx = tap(dx * s, dy * s)
                    cq = cur[qy, qx]
                    wt = guide_terms(np.full((h, w), H5[dy + 2] * H5[dx + 2], F), qy, qx, kp_of(p))
                    if lum_on:
                        x = np.abs(lum[qy, qx] - lum) * rl
                        wt = wt * (ONE / (ONE + x))
                    use = ok & (wt > 0)
                    total = np.where(use[..., None], total + cq * wt[..., None], total)
                    vs = np.where(use, vs + v[qy, qx] * (wt * wt), vs)
                    wsum = np.where(use, wsum + wt, wsum)
            new = ~inert & (wsum > 0)
            cur = np.where(new[..., None], total / wsum[..., None], cur).astype(F)
            v = np.where(new, vs / (wsum * wsum), v).astype(F)
    return cur, v


def extras(h, w, seed, nan=True):
    """A variance image with zero, NaN, infinite and negative entries, moments (some NaN or infinite) and
    lengths 0..7 (on both sides of spatial_below = 4)."""
    r = np.random.default_rng(seed + 1000)
    var = (r.random((h, w), dtype=F) * F(0.05)).astype(F)
    m1 = r.random((h, w), dtype=F)
    moments = np.stack([m1, m1 * m1 + r.random((h, w), dtype=F) * F(0.02)], -1).astype(F)
    length = r.integers(0, 8, (h, w)).astype(np.uint32)
    if nan and h * w > 12:
        for bad in (0.0, np.nan, np.inf, -np.inf, -0.5):
            var[r.integers(h), r.integers(w)] = bad
        moments[r.integers(h), r.integers(w), 0] = np.nan
        moments[r.integers(h), r.integers(w), 1] = np.inf
    return var, moments, length


def same(a, b):
    return all(DR.same_bits(x, y) for x, y in zip(a, b))


# ---- the numpy restatement -----------------------------------------------------------------------------

def test_numpy_restatement_equals_the_reference_in_bits():
    color, normal, position, ident = scene(23, 37)
    var, moments, length = extras(23, 37, 1)
    kw = dict(passes=3, sigma_luminance=2.0, luminance_floor=1e-3, sigma_position=0.3, normal_power_log2=3)
    out, vout, fb = VR.denoise_variance(color, var, normal, position, ident, moments, length, **kw)
    want = np_denoise_variance(color, var, normal, position, ident, moments, length, **kw)
    assert same((out, vout), want)
    assert np.array_equal(fb, np_framebuffer(want[0]))
    assert not DR.same_bits(out, color) and not DR.same_bits(vout, var)
    # the other branches: no normal (the Euclidean distance), no guides at all, no estimate, term off
    for args, kw in [((None, position, None, moments, length), dict(passes=2, sigma_position=0.7)),
                     ((None, None, None, moments, length), dict(passes=4)),
                     ((normal, None, ident), dict(passes=2, sigma_luminance=4.0)),
                     ((normal, position, ident, moments, length), dict(passes=2, sigma_luminance=0.0, sigma_position=0.5)),
                     ((None, None, None), dict(passes=8, luminance_floor=1e-2))]:
        got = VR.denoise_variance(color, var, *args, **kw)
        assert same(got[:2], np_denoise_variance(color, var, *args, **kw)), kw


@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (7, 1), (5, 5), (3, 3)])
def test_small_sizes_against_the_restatement(w, h):
    color, normal, position, ident = scene(h, w, seed=w + 10 * h)
    var, moments, length = extras(h, w, w + 10 * h)
    for passes in (1, 3, 8):
        kw = dict(passes=passes, sigma_luminance=2.0, sigma_position=0.4, normal_power_log2=2)
        got = VR.denoise_variance(color, var, normal, position, ident, moments, length, **kw)
        assert same(got[:2], np_denoise_variance(color, var, normal, position, ident, moments, length, **kw))


# ---- values worked by hand -----------------------------------------------------------------------------

def test_uniform_image_by_hand():
    """A uniform 9 x 9 image with the uniform variance v = 2^-6, no guides, one pass: every luminance
    difference is 0, so a tap weighs h*h. An interior pixel sees all 25: wsum = 1 and the sum of w^2 is
    (70/256)^2 = 4900/65536, every partial sum exact. The corner (0, 0) sees dy, dx in {0, 1, 2}: wsum =
    (11/16)^2 = 121/256, the sum of w^2 is (53/256)^2 = 2809/65536."""
    v = F(2.0 ** -6)
    color = np.tile(np.array([0.25, 0.5, 0.75], F), (9, 9, 1))
    var = np.full((9, 9), v, F)
    for sl in (0.0, 2.0):
        out, vout, _ = VR.denoise_variance(color, var, passes=1, sigma_luminance=sl)
        assert vout[4, 4] == v * F(4900.0) / F(65536.0) == F(2.0 ** -6 * 4900 / 65536)
        assert (vout[2:7, 2:7] == vout[4, 4]).all()
        wsum = F(121.0 / 256.0)
        corner = (v * F(2809.0 / 65536.0)) / (wsum * wsum)
        for y, x in ((0, 0), (0, 8), (8, 0), (8, 8)):
            assert vout[y, x] == corner
        # an edge pixel away from the corners: three rows of five taps, (11/16)(1) and (53/256)(70/256)
        wsum = F(11.0 / 16.0)
        assert vout[0, 4] == (v * F(53.0 * 70.0 / 65536.0)) / (wsum * wsum)
        assert DR.same_bits(out[2:7, 2:7], color[2:7, 2:7])  # sum = c * 1 exactly in the interior


def test_one_pixel_by_hand():
    c = np.array([[[0.25, 3.5, -1.0]]], F)
    v = np.array([[0.3]], F)
    w = H5[2] * H5[2]
    for passes in range(1, 9):
        out, vout, fb = VR.denoise_variance(c, v, passes=passes, sigma_luminance=2.0)
        want, wv = c[0, 0], v[0, 0]
        for _ in range(passes):
            want, wv = (want * w) / w, (wv * (w * w)) / (w * w)  # the centre is an ordinary tap
        assert DR.same_bits(out[0, 0], want) and vout[0, 0] == wv
        assert fb[0, 0] == (0 | (255 << 8) | (63 << 16))
    # the estimate of a 1 x 1 image: e = m2 - m1^2 from its own moments, boosted by 4 / length
    m = np.array([[[0.5, 0.3125]]], F)  # e = 0.0625
    for ln, boost in ((1, 4.0), (2, 2.0), (0, 4.0), (4, None), (9, None)):
        _, vout, _ = VR.denoise_variance(c, v, moments=m, length=np.array([[ln]], np.uint32), passes=1, spatial_below=4)
        start = v[0, 0] if boost is None else F(0.0625) * F(boost)
        assert vout[0, 0] == (start * (w * w)) / (w * w), ln


GREEN = float.fromhex("0x1.65f11cp-1")  # 0.7152f * GREEN rounds to 0.5 exactly


def test_two_pixels_with_a_luminance_step_by_hand():
    """P = (0, 0, 0) and Q = (0, GREEN, 0) side by side, lum 0 and 0.5; v = 2^-4 on both, so the
    prefiltered variance is v (0.375 v / 0.375) and sd = 0.25; sigma_luminance 1 and floor 0.25 give rl = 2,
    x = 1 and a luminance weight of exactly 1/2 on the other pixel."""
    color = np.array([[[0, 0, 0], [0, GREEN, 0]]], F)
    assert np_lum(color)[0, 1] == F(0.5) and np_lum(color)[0, 0] == 0
    v = F(2.0 ** -4)
    var = np.full((1, 2), v, F)
    out, vout, _ = VR.denoise_variance(color, var, passes=1, sigma_luminance=1.0, luminance_floor=0.25)
    w0 = H5[2] * H5[2]                 # the centre: 9/64, luminance weight 1
    w1 = (H5[2] * H5[3]) * F(0.5)      # the neighbour: 3/32 halved
    assert (w0, w1) == (F(0.140625), F(0.046875))
    wsum = w0 + w1
    g = F(GREEN)
    # P: centre first (dx = 0), then Q (dx = 1); Q: P first (dx = -1), then the centre
    assert out[0, 0, 1] == (F(0.0) * w0 + g * w1) / wsum
    assert out[0, 1, 1] == (F(0.0) * w1 + g * w0) / wsum
    assert (out[0, :, 0] == 0).all() and (out[0, :, 2] == 0).all()
    want = (v * (w0 * w0) + v * (w1 * w1)) / (wsum * wsum)
    assert vout[0, 0] == want and vout[0, 1] == (v * (w1 * w1) + v * (w0 * w0)) / (wsum * wsum)
    # with the term off both weigh h*h: 9/64 and 3/32
    out, vout, _ = VR.denoise_variance(color, var, passes=1, sigma_luminance=0.0, luminance_floor=0.25)
    w1 = H5[2] * H5[3]
    assert out[0, 0, 1] == (F(0.0) * w0 + g * w1) / (w0 + w1)
    assert vout[0, 0] == (v * (w0 * w0) + v * (w1 * w1)) / ((w0 + w1) * (w0 + w1))


# ---- the variance's sanitisation, inert pixels -----------------------------------------------------------

def test_bad_variances_count_as_zero_and_make_no_pixel_inert():
    color, normal, position, ident = scene(11, 13, seed=3, nan=False)
    var = np.full((11, 13), 0.01, F)
    clean = var.copy()
    for k, bad in enumerate((np.nan, np.inf, -np.inf, -0.25, -0.0)):
        var[2 + k, 3 + 2 * k] = bad
        clean[2 + k, 3 + 2 * k] = 0.0
    kw = dict(passes=3, sigma_luminance=2.0, sigma_position=0.5)
    a = VR.denoise_variance(color, var, normal, position, ident, **kw)
    b = VR.denoise_variance(color, clean, normal, position, ident, **kw)
    assert same(a, b)
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all() and (a[1] >= 0).all()
    assert not DR.same_bits(a[0][2, 3], color[2, 3])  # the pixel is filtered like any other


@pytest.mark.parametrize("where,bad", [(a, b) for a in ("color", "normal", "position") for b in (np.nan, np.inf, -np.inf)]
                         + [("ident", None)])
def test_an_inert_pixel_keeps_its_bits_has_no_variance_and_is_no_tap(where, bad):
    color, normal, position, _ = scene(11, 13, seed=3, nan=False)
    var, moments, length = extras(11, 13, 3, nan=False)
    ident = np.zeros((11, 13), np.uint32)
    g = {"color": color, "normal": normal, "position": position}
    if where == "ident":
        ident[5, 6] = EMPTY
    else:
        g[where][5, 6, 1] = bad
    kw = dict(passes=3, sigma_luminance=2.0, sigma_position=0.5)
    out, vout, fb = VR.denoise_variance(color, var, normal, position, ident, moments, length, **kw)
    assert DR.same_bits(out[5, 6], color[5, 6]) and vout[5, 6] == 0
    assert fb[5, 6] == np_framebuffer(color)[5, 6]
    # marking it EMPTY and giving it any finite values, variance and moments gives the same neighbours
    marked = ident.copy()
    marked[5, 6] = EMPTY
    clean = {k: a.copy() for k, a in g.items()}
    if where != "ident":
        clean[where][5, 6, 1] = F(0.5)
    var2, mom2 = var.copy(), moments.copy()
    var2[5, 6], mom2[5, 6] = 9.0, (3.0, 100.0)
    ref = VR.denoise_variance(clean["color"], var2, clean["normal"], clean["position"], marked, mom2, length, **kw)
    keep = np.ones((11, 13), bool)
    keep[5, 6] = False
    assert DR.same_bits(out[keep], ref[0][keep]) and DR.same_bits(vout[keep], ref[1][keep])
    assert np.isfinite(out[keep]).all() and np.isfinite(vout[keep]).all()


def test_nothing_leaks_across_ids():
    color, normal, position, ident = scene(23, 37, seed=2, nan=False)
    var, moments, length = extras(23, 37, 2, nan=False)
    a = ident == 0
    other, ovar, omom = color.copy(), var.copy(), moments.copy()
    r = np.random.default_rng(5)
    other[~a] = r.random((int((~a).sum()), 3), dtype=F) * F(9.0)
    ovar[~a] = 7.0
    omom[~a] = (2.0, 50.0)
    kw = dict(passes=4, sigma_luminance=2.0, sigma_position=0.5)
    x = VR.denoise_variance(color, var, normal, position, ident, moments, length, **kw)
    y = VR.denoise_variance(other, ovar, normal, position, ident, omom, length, **kw)
    assert DR.same_bits(x[0][a], y[0][a]) and DR.same_bits(x[1][a], y[1][a])
    assert not DR.same_bits(x[0][~a], y[0][~a])


# ---- the spatial estimate ------------------------------------------------------------------------------

def test_long_histories_take_no_estimate():
    color, normal, position, ident = scene(17, 21, seed=6)
    var, moments, _ = extras(17, 21, 6)
    kw = dict(passes=2, sigma_luminance=2.0, sigma_position=0.5)
    plain = VR.denoise_variance(color, var, normal, position, ident, **kw)
    for ln in (4, 5, 64, 0xFFFFFFFF):
        length = np.full((17, 21), ln, np.uint32)
        assert same(VR.denoise_variance(color, var, normal, position, ident, moments, length, **kw), plain)
    short = np.full((17, 21), 3, np.uint32)
    assert not same(VR.denoise_variance(color, var, normal, position, ident, moments, short, **kw), plain)
    # spatial_below = 0 switches it off whatever the lengths
    assert same(VR.denoise_variance(color, var, normal, position, ident, moments, short, spatial_below=0, **kw), plain)


def test_length_one_everywhere_ignores_the_supplied_variance():
    """atr_accumulate gives a pixel of length 1 the variance 0; every live pixel takes the estimate
    instead, which is 4 times the window's variance, and the supplied variance plays no part."""
    color, normal, position, ident = scene(17, 21, seed=7, nan=False)
    var, moments, _ = extras(17, 21, 7, nan=False)
    length = np.ones((17, 21), np.uint32)
    kw = dict(passes=1, sigma_luminance=2.0)
    a = VR.denoise_variance(color, np.zeros_like(var), normal, position, ident, moments, length, **kw)
    b = VR.denoise_variance(color, var, normal, position, ident, moments, length, **kw)
    assert same(a, b) and (a[1] > 0).all()
    zero = VR.denoise_variance(color, np.zeros_like(var), normal, position, ident, **kw)
    assert (zero[1] == 0).all() and not DR.same_bits(a[0], zero[0])
    # the estimate on its own: uniform moments (m1 = 0.5, m2 = 0.3125) give e = 0.0625 for every window,
    # whatever the weights, up to the rounding of a / ws; without guides the weights are 1 and it is exact
    flat = np.tile(np.array([0.5, 0.3125], F), (17, 21, 1))
    _, vout, _ = VR.denoise_variance(color, var, moments=flat, length=length, passes=1, sigma_luminance=0.0)
    _, want, _ = VR.denoise_variance(color, np.full_like(var, 0.25), passes=1, sigma_luminance=0.0)
    assert DR.same_bits(vout, want)


def test_a_tap_with_a_nan_moment_is_skipped():
    color = np.full((1, 3, 3), 0.5, F)
    var = np.zeros((1, 3), F)
    length = np.ones((1, 3), np.uint32)
    moments = np.array([[[0.5, 0.3125], [0.25, 0.125], [0.75, 0.625]]], F)
    w = H5[2] * H5[2]

    def start(m, ln=length):
        # one pass on an image whose only live pixel is 0, so that its variance_out is its start value
        ident = np.array([[0, 1, 2]], np.uint32)
        return VR.denoise_variance(color, var, ident=ident, moments=m, length=ln, passes=1)[1][0]

    # with three ids every pixel sees only itself: e = m2 - m1^2, times 4
    own = start(moments)
    assert list(own) == [(F(e) * F(4.0) * (w * w)) / (w * w) for e in (0.0625, 0.0625, 0.0625)]
    # one id: pixel 0 sees all three with weight 1: a = 1.5, b = 1.0625, ws = 3
    full = VR.denoise_variance(color, var, moments=moments, length=np.array([[1, 9, 9]], np.uint32), passes=1,
                               sigma_luminance=0.0)[1]
    m1, m2 = F(1.5) / F(3.0), F(1.0625) / F(3.0)
    v0 = (m2 - m1 * m1) * F(4.0)
    w1, w2 = H5[2] * H5[3], H5[2] * H5[4]
    assert full[0, 0] == ((v0 * (w * w) + F(0.0) * (w1 * w1)) + F(0.0) * (w2 * w2)) / (((w + w1) + w2) * ((w + w1) + w2))
    # a NaN (or infinite) moment in pixel 1 leaves pixels 0 and 2: a = 1.25, b = 0.9375, ws = 2
    for bad, k in ((np.nan, 0), (np.inf, 1), (-np.inf, 0)):
        m = moments.copy()
        m[0, 1, k] = bad
        got = VR.denoise_variance(color, var, moments=m, length=np.array([[1, 9, 9]], np.uint32), passes=1,
                                  sigma_luminance=0.0)[1]
        m1, m2 = F(1.25) / F(2.0), F(0.9375) / F(2.0)
        v0 = (m2 - m1 * m1) * F(4.0)
        assert got[0, 0] == ((v0 * (w * w) + F(0.0) * (w1 * w1)) + F(0.0) * (w2 * w2)) / (((w + w1) + w2) * ((w + w1) + w2))
    # a pixel whose own moments are NaN and that sees nobody else keeps its variance
    m = moments.copy()
    m[0, 0, 0] = np.nan
    assert start(m)[0] == 0


def test_length_zero_on_a_live_pixel_counts_as_one():
    color, normal, position, ident = scene(9, 12, seed=8, nan=False)
    var, moments, _ = extras(9, 12, 8, nan=False)
    kw = dict(passes=2, sigma_luminance=2.0)
    zero = VR.denoise_variance(color, var, normal, position, ident, moments, np.zeros((9, 12), np.uint32), **kw)
    one = VR.denoise_variance(color, var, normal, position, ident, moments, np.ones((9, 12), np.uint32), **kw)
    two = VR.denoise_variance(color, var, normal, position, ident, moments, np.full((9, 12), 2, np.uint32), **kw)
    assert same(zero, one) and not same(one, two)


def test_sigma_luminance_zero_turns_the_term_off():
    color, normal, position, ident = scene(15, 18, seed=9)
    var, _, _ = extras(15, 18, 9)
    kw = dict(passes=3, sigma_position=0.5)
    off = VR.denoise_variance(color, var, normal, position, ident, sigma_luminance=0.0, **kw)
    # off: neither the variance nor the floor reaches the colour
    for v2, fl in ((var * F(100.0), 1e-4), (var, 10.0)):
        other = VR.denoise_variance(color, v2, normal, position, ident, sigma_luminance=0.0, luminance_floor=fl, **kw)
        assert DR.same_bits(off[0], other[0])
    on = VR.denoise_variance(color, var, normal, position, ident, sigma_luminance=1.0, **kw)
    assert not DR.same_bits(off[0], on[0])
    # off equals atr_denoise's arithmetic with its colour term off
    want, _ = DR.denoise(color, normal, position, ident, passes=3, sigma_color=0.0, sigma_position=0.5)
    assert DR.same_bits(off[0], want)


def test_constants_rule():
    rc, kp = VR.constants(8, 0.5)
    assert rc == 0 and np.array_equal(kp, np.array([4.0 / 4.0 ** p for p in range(8)], F))
    assert VR.constants(1, 1e-30)[0] == -1 and VR.constants(1, 1e30)[0] == -1
    assert VR.constants(1, 1e18)[0] == 0 and VR.constants(8, 1e18)[0] == -1
    assert VR.constants(1, 1e-30, position_given=False)[0] == 0
    c, v = np.zeros((2, 2, 3), F), np.zeros((2, 2), F)
    assert VR.denoise_variance(c, v, sigma_position=1e-30) is not None
    assert VR.denoise_variance(c, v, position=c, sigma_position=1e-30) is None


# ---- the entry points (these need the engine library) ----------------------------------------------------

def test_binding_and_defaults():
    from atray_amd import engine as E
    sig = E.signatures()
    names = {"atr_denoise_variance", "atr_denoise_variance_check", "atr_default_denoise_variance_params"}
    assert names <= set(sig) and names <= set(E.EXPORTS)
    args, res = sig["atr_denoise_variance"]
    assert len(args) == 13 and res is C.c_int
    assert len(sig["atr_denoise_variance_check"][0]) == 11
    assert C.sizeof(E.atr_denoise_variance_params) == 32
    p = E.atr_denoise_variance_params(9, 9.0, 9.0, 9.0, 9, 9, (C.c_int32 * 2)(1, 2))
    E.lib().atr_default_denoise_variance_params(C.byref(p))
    got = dict(passes=p.passes, sigma_luminance=p.sigma_luminance, luminance_floor=p.luminance_floor,
               sigma_position=p.sigma_position, normal_power_log2=p.normal_power_log2, spatial_below=p.spatial_below)
    assert list(p.reserved) == [0, 0]
    assert got == {k: (float(F(v)) if isinstance(v, float) else v) for k, v in VR.DEFAULTS.items()}
    import inspect
    d = {k: v.default for k, v in inspect.signature(E.Engine.denoise_variance).parameters.items()}
    assert {k: d[k] for k in VR.DEFAULTS} == VR.DEFAULTS
    assert (d["out"], d["variance_out"], d["framebuffer"], d["stream"]) == (None, False, False, None)
    assert callable(E.TemporalAccumulator.filtered)


def test_argument_rules():
    """atr_denoise_variance_check is atr_denoise_variance's validation on the host; the addresses are
    never followed."""
    from atray_amd import engine as E
    ok, inv = 0, -1
    P = E.atr_denoise_variance_params
    good = dict(passes=3, sigma_luminance=2.0, luminance_floor=1e-3, sigma_position=0.0, normal_power_log2=5,
                spatial_below=4)
    mk = lambda **kw: P(*[dict(good, **kw)[k] for k in good])  # noqa: E731

    def call(w=8, h=4, color=0x1000, variance=0x2000, guides=True, gn=0x3000, gp=0x4000, gi=0x5000, moments=0x6000,
             length=0x7000, params=None, out=0x8000, vout=0x9000, fb=0xA000, **kw):
        g = E.atr_denoise_guides(gn, gp, gi)
        p = mk(**kw) if params is None else params
        return E.lib().atr_denoise_variance_check(color, variance, C.byref(g) if guides else None, moments, length, w, h,
                                                  C.byref(p) if p else None, out, vout, fb)

    assert call() == ok
    assert call(color=None) == inv and call(variance=None) == inv and call(params=False) == inv
    assert call(out=None) == ok and call(fb=None) == ok and call(out=None, fb=None) == inv
    assert call(vout=None) == ok and call(vout=None, out=None, fb=None) == inv
    assert call(out=0x1000, vout=0x2000) == ok  # in place
    assert call(moments=None) == inv and call(length=None) == inv and call(moments=None, length=None) == ok
    assert call(guides=False) == ok and call(gn=None, gp=None, gi=None) == ok
    for size in [(0, 4), (8, 0), (-1, 4), (16385, 4), (8, 16385)]:
        assert call(w=size[0], h=size[1]) == inv
    assert call(w=16384, h=16384) == ok and call(w=1, h=1) == ok
    nan, inf = float("nan"), float("inf")
    for kw in [dict(passes=1), dict(passes=8), dict(sigma_luminance=0.0), dict(sigma_luminance=1e30),
               dict(luminance_floor=1e-30), dict(luminance_floor=1e30), dict(normal_power_log2=0),
               dict(normal_power_log2=7), dict(spatial_below=0), dict(spatial_below=1 << 24), dict(sigma_position=0.5)]:
        assert call(**kw) == ok, kw
    for kw in [dict(passes=0), dict(passes=9), dict(passes=-1), dict(sigma_luminance=-0.5), dict(sigma_luminance=nan),
               dict(sigma_luminance=inf), dict(luminance_floor=0.0), dict(luminance_floor=-1.0), dict(luminance_floor=nan),
               dict(luminance_floor=inf), dict(sigma_position=-0.5), dict(sigma_position=nan), dict(sigma_position=inf),
               dict(sigma_position=-inf), dict(normal_power_log2=-1), dict(normal_power_log2=8), dict(spatial_below=-1),
               dict(spatial_below=(1 << 24) + 1)]:
        assert call(**kw) == inv, kw
    for k in range(2):
        r = (C.c_int32 * 2)()
        r[k] = 1
        assert call(params=P(3, 2.0, 1e-3, 0.0, 5, 4, r)) == inv
    # the kp rule: only with the position term on, in every pass
    assert call(sigma_position=1e-30) == inv and call(sigma_position=1e30) == inv
    assert call(sigma_position=1e-30, gp=None) == ok and call(sigma_position=1e-30, guides=False) == ok
    assert call(sigma_position=-1.0, gp=None) == inv  # the sigma itself is still checked
    assert call(passes=1, sigma_position=1e18) == ok and call(passes=8, sigma_position=1e18) == inv
    for passes, sp in [(1, 1e18), (8, 1e18), (8, 1e17), (8, 3e-20), (2, 3e-20), (1, 1e-30), (5, 1.0)]:
        assert call(passes=passes, sigma_position=sp) == (inv if VR.constants(passes, sp)[0] else ok)
    # the entry point itself: a NULL context is refused before anything else
    p = mk()
    assert E.lib().atr_denoise_variance(None, 0x1000, 0x2000, None, None, None, 8, 4, C.byref(p), 0x8000, None, None,
                                        None) == inv


# ---- the conditions on the defaults ----------------------------------------------------------------------

PW, PH = 56, 40


def two_plane_image(seed):
    """§4s's kind of synthetic image, 56 x 40: two planes side by side, each with a colour gradient, an
    ident and a normal of its own; grey Gaussian noise of sd 0.02 on the left plane and 0.2 on the right.
    Returns (clean, noisy, variance, (normal, position, ident), right), variance the true sd^2."""
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:PH, 0:PW]
    right = xx >= PW // 2
    u, v = (xx / F(PW)).astype(F), (yy / F(PH)).astype(F)
    left_c = np.stack([F(0.2) + F(0.6) * u, F(0.7) - F(0.4) * v, F(0.3) + F(0.3) * u * v], -1)
    right_c = np.stack([F(0.8) - F(0.5) * v, F(0.25) + F(0.5) * u, F(0.6) - F(0.3) * u], -1)
    clean = np.where(right[..., None], right_c, left_c).astype(F)
    sd = np.where(right, F(0.2), F(0.02)).astype(F)
    noise = r.standard_normal((PH, PW)).astype(F) * sd
    noisy = (clean + noise[..., None]).astype(F)
    normal = np.where(right[..., None], np.array([0.6, 0.0, 0.8], F), np.array([0.0, 0.0, 1.0], F)).astype(F)
    position = np.stack([xx * F(0.1), yy * F(0.1), np.where(right, (xx - PW // 2) * F(-0.075), F(0.0))], -1).astype(F)
    ident = np.where(right, 2, 1).astype(np.uint32)
    return clean, noisy, (sd * sd).astype(F), (normal, position, ident), right


def mse(a, b, mask=None):
    d = (a.astype(np.float64) - b.astype(np.float64)) ** 2
    return float(d.mean() if mask is None else d[mask].mean())


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_defaults_beat_every_single_tolerance_on_two_noise_levels(seed):
    """Conditions on the defaults, not measurements (DESIGN.md §4u has the grid): on the two-plane image,
    with the true variance supplied, (a) the error on each plane separately is below the unfiltered
    image's and (b) the whole-image error is below atr_denoise's with the same guides, sigma_position
    and normal power at every sigma_color in {0.01, 0.05, 0.2, 1} and both of its pass counts {3, 5}."""
    clean, noisy, var, (normal, position, ident), right = two_plane_image(seed)
    d = VR.DEFAULTS
    out, _, _ = VR.denoise_variance(noisy, var, normal, position, ident)
    for plane in (~right, right):
        print(f"seed {seed}: plane mse {mse(out, clean, plane):.3e}, unfiltered {mse(noisy, clean, plane):.3e}")
    whole = mse(out, clean)
    others = {(p, sc): mse(DR.denoise(noisy, normal, position, ident, passes=p, sigma_color=sc,
                                      sigma_position=d["sigma_position"], normal_power_log2=d["normal_power_log2"])[0], clean)
              for p in (3, 5) for sc in (0.01, 0.05, 0.2, 1.0)}
    print(f"seed {seed}: whole image {whole:.3e}; atr_denoise's best {min(others.values()):.3e}")
    for plane in (~right, right):
        assert mse(out, clean, plane) < mse(noisy, clean, plane)
    for key, e in others.items():
        assert whole < e, key
