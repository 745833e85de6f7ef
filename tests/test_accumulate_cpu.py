"""The temporal accumulator's plain C reference (tests/accumulate_ref.py) pinned without a GPU, so that it
is not its own only witness: a vectorised numpy-f32 restatement of include/atray.h's formulas, pixels
worked by hand from a camera at the origin facing -z (so that sx and sy are exact binary fractions), each
tap test rejecting alone, the inert rule, a camera at rest, the argument rules through the host-only
atr_accumulate_check, and one condition on the defaults: on a diffuse Monkey they lower the error of the
last 1-spp frame of an orbit against its 256-spp render."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import oracle as O
from tests import accumulate_ref as AR

F = np.float32
EMPTY = np.uint32(0xFFFFFFFF)
ORIGIN = np.array([0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 1], F)  # eye, x, y, z axes, k = 1: the film is [-1, 1]^2


def np_accumulate(color, guides=(None, None, None), prev=None, moments=True, **params):
    """atray.h's formulas on whole images, one tap at a time in the stated order; every numpy f32
    operation is separately rounded."""
    kw = dict(AR.DEFAULTS, **params)
    c = np.array(color, F)
    h, w = c.shape[:2]
    nrm, pos, idt = guides
    fin = lambda a: np.isfinite(a).all(axis=2)  # noqa: E731
    inert = ~fin(c)
    if idt is not None:
        idt = np.asarray(idt).view(np.uint32)
        inert |= idt == EMPTY
    if nrm is not None:
        inert |= ~fin(nrm)
    if pos is not None:
        inert |= ~fin(pos)
    dot = lambda a, b: (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]  # noqa: E731
    total, msum, wsum = np.zeros((h, w, 3), F), np.zeros((h, w, 2), F), np.zeros((h, w), F)
    nmin = np.full((h, w), 0xFFFFFFFF, np.uint32)
    one = F(1.0)
    with np.errstate(all="ignore"):
        if prev is not None:
            cam = prev["cam"] if isinstance(prev["cam"], np.ndarray) else AR.cam_floats(prev["cam"])
            pn, pp, pi = prev["guides"]
            pi = None if pi is None else np.asarray(pi).view(np.uint32)
            pc, pm, pl = prev["color"], prev.get("moments"), np.asarray(prev["length"]).view(np.uint32)
            v = pos - cam[0:3]
            depth = -dot(v, cam[9:12])
            a, b = dot(v, cam[3:6]) / depth, dot(v, cam[6:9]) / depth
            sx = (a / cam[12] + one) * (F(0.5) * F(w))
            sy = (b + one) * (F(0.5) * F(h))
            ok0 = ~inert & (depth > 0) & (sx >= -one) & (sx < F(w)) & (sy >= -one) & (sy < F(h))
            sx, sy = np.where(ok0, sx, F(0.0)), np.where(ok0, sy, F(0.0))
            fx0, fy0 = np.floor(sx), np.floor(sy)
            x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
            tx, ty = sx - fx0, sy - fy0
            tol = F(kw["plane_tolerance"]) * depth
            tol2 = tol * tol
            for dy in (0, 1):
                for dx in (0, 1):
                    qx, qy = x0 + dx, y0 + dy
                    ok = ok0 & (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                    ok &= pl[qy, qx] != 0
                    if idt is not None:
                        ok &= (pi[qy, qx] == idt) & (pi[qy, qx] != EMPTY)
                    if nrm is not None:
                        ok &= dot(nrm, pn[qy, qx]) >= F(kw["min_normal_dot"])
                    dv = pp[qy, qx] - pos
                    if nrm is not None:
                        e = dot(nrm, dv)
                        e2 = e * e
                    else:
                        e2 = dot(dv, dv)
                    ok &= e2 <= tol2
                    hc = pc[qy, qx]
                    ok &= fin(hc)
                    if moments:
                        hm = pm[qy, qx]
                        ok &= fin(hm)
                    wt = (tx if dx else one - tx) * (ty if dy else one - ty)
                    ok &= wt > 0
                    total = np.where(ok[..., None], total + hc * wt[..., None], total)
                    if moments:
                        msum = np.where(ok[..., None], msum + hm * wt[..., None], msum)
                    wsum = np.where(ok, wsum + wt, wsum)
                    nmin = np.where(ok, np.minimum(nmin, pl[qy, qx]), nmin)
        lum = (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]
        has = ~inert & (wsum > 0)
        hcol, hmom = total / wsum[..., None], msum / wsum[..., None]
        ln = np.minimum(nmin, np.uint32(kw["max_length"] - 1)) + np.uint32(1)
        aw = one / ln.astype(F)
        ac = np.where(F(kw["alpha"]) > aw, F(kw["alpha"]), aw)
        am = np.where(F(kw["alpha_moments"]) > aw, F(kw["alpha_moments"]), aw)
        oc = np.where(has[..., None], hcol + (c - hcol) * ac[..., None], c)
        m1 = np.where(has, hmom[..., 0] + (lum - hmom[..., 0]) * am, lum)
        m2 = np.where(has, hmom[..., 1] + (lum * lum - hmom[..., 1]) * am, lum * lum)
        m1, m2 = np.where(inert, F(0.0), m1), np.where(inert, F(0.0), m2)
        var = m2 - m1 * m1
        var = np.where(var > 0, var, F(0.0))
        length = np.where(inert, 0, np.where(has, ln, 1)).astype(np.uint32)
    return {"color": oc.astype(F), "moments": np.stack([m1, m2], -1).astype(F) if moments else None, "length": length,
            "variance": var.astype(F) if moments else None, "framebuffer": np_framebuffer(oc)}


def np_framebuffer(img):
    """The renderer's clamp and quantisation (a NaN gives 0)."""
    with np.errstate(all="ignore"):
        k = np.where(img > 1, F(1.0), img)
        k = np.where(F(0.0) > k, F(0.0), k)
        q = np.where(np.isnan(k), 0, (np.nan_to_num(k) * F(255.0)).astype(np.uint32) & 0xFF).astype(np.uint32)
    return q[..., 2] | (q[..., 1] << 8) | (q[..., 0] << 16)


def same(a, b):
    """Two results agree in every output, bit for bit."""
    for k in ("color", "moments", "length", "variance", "framebuffer"):
        if (a[k] is None) != (b[k] is None) or (a[k] is not None and not AR.same_bits(a[k], b[k])):
            return False
    return True


def two_planes(cam, nan=True, seed=0):
    """A synthetic world seen from `cam` (an atr_camera): a far wall z = -40 for |x| < 1000 with a window
    (sky) at 10 < x < 16 and, in front of it, a tilted panel through (0, -15, -30) for |x| < 8, |y + 15| < 6; sky elsewhere. Positions are
    the camera's rays times an analytic t. Returns (normal, position, ident), ident 1, 2 or EMPTY; with
    nan=True a few normals and positions are NaN or infinite."""
    from atray_amd import engine as E
    h, w = int(cam.height), int(cam.width)
    o, d = E.camera_rays(cam)
    nb = np.array([0.3, 0.2, 1.0], F)
    nb = (nb / np.sqrt((nb * nb).sum())).astype(F)
    planes = [(np.array([0, 0, 1], F), F(-40.0)), (nb, F((nb * np.array([0, -15, -30], F)).sum()))]
    with np.errstate(all="ignore"):
        t = [((dist - (o * n).sum(1)) / (d * n).sum(1)).astype(F) for n, dist in planes]
        p = [(o + d * ti[:, None]).astype(F) for ti in t]
    on_a = (t[0] > 0) & (np.abs(p[0][:, 0]) < 1000) & ~((p[0][:, 0] > 10) & (p[0][:, 0] < 16))
    on_b = (t[1] > 0) & (np.abs(p[1][:, 0]) < 8) & (np.abs(p[1][:, 1] + 15) < 6)
    ident = np.where(on_b, 2, np.where(on_a, 1, EMPTY)).astype(np.uint32)
    position = np.where(on_b[:, None], p[1], np.where(on_a[:, None], p[0], F(0.0))).astype(F)
    normal = np.where(on_b[:, None], nb, np.where(on_a[:, None], planes[0][0], F(0.0))).astype(F)
    normal = np.where(((normal * -d).sum(1) < 0)[:, None], -normal, normal).astype(F)
    normal, position, ident = normal.reshape(h, w, 3), position.reshape(h, w, 3), ident.reshape(h, w)
    if nan and h * w > 12:
        r = np.random.default_rng(seed + 77)
        normal[r.integers(h), r.integers(w), 0] = np.nan
        position[r.integers(h), r.integers(w), 2] = -np.inf
    return normal, position, ident


def noisy(h, w, seed, nan=True):
    r = np.random.default_rng(seed)
    c = r.random((h, w, 3), dtype=F) * F(1.5)
    if nan and h * w > 12:
        c[r.integers(h), r.integers(w), 1] = np.nan
        c[r.integers(h), r.integers(w), 2] = np.inf
    return c


def orbit(k, step=0.02, center=None, spp=1, bounces=1):
    """(eye, facing) of frame k: the app's camera turned by k * step rad about the vertical axis through
    `center` (the Monkey's by default)."""
    from atray_amd.assets import CENTERS
    c = np.array(CENTERS["Monkey"] if center is None else center, np.float64)
    a = k * step
    rot = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    eye = c + rot @ (np.array(O.APP_EYE, np.float64) - c)
    return tuple(float(x) for x in eye), tuple(float(x) for x in rot @ np.array(O.APP_FACING, np.float64))


def chain(cams, size, subset=7, nan=True, use=AR.accumulate, **params):
    """The results of accumulating one noisy frame per camera through ping-ponged histories."""
    h, w = size
    prev, outs = None, []
    for f, cam in enumerate(cams):
        g = two_planes(cam, nan=nan, seed=f)
        g = (g[0] if subset & 1 else None, g[1], g[2] if subset & 2 else None)
        out = use(noisy(h, w, 100 + f, nan=nan), g, prev, moments=bool(subset & 4), **params)
        prev = AR.history(out, cam, g)
        outs.append(out)
    return outs


def test_numpy_restatement_equals_the_reference_in_bits():
    from atray_amd import engine as E
    w, h = 37, 23
    cams = [E.camera(w, h, eye=e, facing=f) for e, f in (orbit(k, 0.01, (0, -15, -35)) for k in (0, 1, 16, 60))]
    for subset in range(8):
        a = chain(cams, (h, w), subset, max_length=2, alpha=0.1, alpha_moments=0.3)
        b = chain(cams, (h, w), subset, use=np_accumulate, max_length=2, alpha=0.1, alpha_moments=0.3)
        assert all(same(x, y) for x, y in zip(a, b)), subset
        # without normals the plane test is the distance itself, which few neighbours pass at this pixel size
        assert (a[2]["length"] == 2).sum() > (100 if subset & 1 else 10)
        assert set(np.unique(a[3]["length"])) == {0, 1, 2}, subset  # the last step turns part of the wall off the film
    assert not AR.same_bits(a[1]["color"], noisy(h, w, 101))


W8, H4 = 8, 4


def flat(p, n=(0, 0, 1)):
    """Guides of an 8 x 4 frame whose every pixel shows the point p with normal n and ident 3."""
    return (np.tile(np.array(n, F), (H4, W8, 1)), np.tile(np.array(p, F), (H4, W8, 1)), np.full((H4, W8), 3, np.uint32))


def hist(seed=5):
    r = np.random.default_rng(seed)
    return {"color": r.random((H4, W8, 3), dtype=F), "moments": r.random((H4, W8, 2), dtype=F),
            "length": r.integers(1, 9, (H4, W8)).astype(np.uint32)}


def by_hand(c, taps, prev, max_length=64, alpha=0.0, alpha_moments=0.0):
    """The blend of colour c with the kept taps [(x, y, w)], scalar by scalar in f32."""
    total, ms, wsum, nmin = np.zeros(3, F), np.zeros(2, F), F(0.0), 0xFFFFFFFF
    for x, y, w in taps:
        total = total + prev["color"][y, x] * F(w)
        ms = ms + prev["moments"][y, x] * F(w)
        wsum = wsum + F(w)
        nmin = min(nmin, int(prev["length"][y, x]))
    lum = (F(0.2126) * c[0] + F(0.7152) * c[1]) + F(0.0722) * c[2]
    if not taps:
        return c, np.array([lum, lum * lum], F), 1
    hc, hm = total / wsum, ms / wsum
    n = min(nmin, max_length - 1) + 1
    aw = F(1.0) / F(n)
    ac, am = max(F(alpha), aw), max(F(alpha_moments), aw)
    return hc + (c - hc) * ac, np.array([hm[0] + (lum - hm[0]) * am, hm[1] + (lum * lum - hm[1]) * am], F), n


def expect(out, c, taps, prev, **kw):
    col, mom, n = by_hand(c, taps, prev, **kw)
    assert AR.same_bits(out["color"], np.tile(col.astype(F), (H4, W8, 1)))
    assert AR.same_bits(out["moments"], np.tile(mom.astype(F), (H4, W8, 1)))
    assert (out["length"] == n).all()
    var = mom[1] - mom[0] * mom[0]
    assert AR.same_bits(out["variance"], np.full((H4, W8), var if var > 0 else 0, F))


FOUR = [(2, 1, 0.375), (3, 1, 0.125), (2, 2, 0.375), (3, 2, 0.125)]  # tx, ty = 0.25, 0.5 at x0, y0 = 2, 1
P4 = (-0.875, -0.5, -2.0)  # depth 2, a = -0.4375, b = -0.25: sx = (a + 1) * 4 = 2.25, sy = (b + 1) * 2 = 1.5


def run(p, prev, c=(0.25, 0.5, 0.75), pg=None, **kw):
    g = flat(p)
    color = np.tile(np.array(c, F), (H4, W8, 1))
    full = dict(prev, cam=ORIGIN, guides=flat(p) if pg is None else pg)
    return AR.accumulate(color, g, full, **kw), np.array(c, F)


def test_four_taps_by_hand():
    prev = hist()
    out, c = run(P4, prev)
    expect(out, c, FOUR, prev)
    # the weights' sum is 1 and nmin the least of the four lengths, by their numbers
    n = min(int(prev["length"][y, x]) for x, y, _ in FOUR) + 1
    assert (out["length"] == n).all()
    out, c = run(P4, prev, alpha=0.5, alpha_moments=0.75, max_length=2)
    expect(out, c, FOUR, prev, alpha=0.5, alpha_moments=0.75, max_length=2)


def test_film_edges_by_hand():
    prev = hist(6)
    # sx = -0.5: a = -1.125; only the column x = 0 exists, with weight tx = 0.5
    out, c = run((-2.25, -0.5, -2.0), prev)
    expect(out, c, [(0, 1, 0.25), (0, 2, 0.25)], prev)
    # sx = 7.5: a = 0.875; only the column x = 7, with weight 1 - tx = 0.5
    out, c = run((1.75, -0.5, -2.0), prev)
    expect(out, c, [(7, 1, 0.25), (7, 2, 0.25)], prev)
    # sy = 3.5: b = 0.75; only the row y = 3
    out, c = run((-0.875, 1.5, -2.0), prev)
    expect(out, c, [(2, 3, 0.375), (3, 3, 0.125)], prev)
    # sx = 8 = W exactly (a = 1), sy = 4 = H exactly (b = 1), sx = -1.5: no history
    for p in [(2.0, -0.5, -2.0), (-0.875, 2.0, -2.0), (-2.75, -0.5, -2.0)]:
        out, c = run(p, prev)
        expect(out, c, [], prev)
    # sx = -1 exactly (a = -1.25): inside the test, and the one column's weight is tx = 0, so no tap is kept
    out, c = run((-2.5, -0.5, -2.0), prev)
    expect(out, c, [], prev)
    # depth <= 0: behind the eye, and in the eye's plane
    for p in [(-0.875, -0.5, 2.0), (1.0, 1.0, 0.0)]:
        out, c = run(p, prev)
        expect(out, c, [], prev)


@pytest.mark.parametrize("kind", ["ident", "empty", "normal", "plane", "length", "colour", "moment"])
def test_each_tap_test_rejects_alone(kind):
    prev = hist(7)
    pg = [a.copy() for a in flat(P4)]
    x, y = 3, 1  # the second tap
    if kind == "ident":
        pg[2][y, x] = 4
    elif kind == "empty":
        pg[2][y, x] = EMPTY
    elif kind == "normal":
        pg[0][y, x] = (0.6, 0.0, 0.8)  # dot 0.8 < 0.9
    elif kind == "plane":
        pg[1][y, x, 2] += F(0.0625)    # e = 0.0625 > tol = 0.02 * 2
    elif kind == "length":
        prev["length"][y, x] = 0
    elif kind == "colour":
        prev["color"][y, x, 2] = np.inf
    else:
        prev["moments"][y, x, 1] = np.nan
    out, c = run(P4, prev, pg=pg)
    expect(out, c, [t for t in FOUR if t[:2] != (x, y)], prev)
    if kind == "empty":  # an EMPTY tap is rejected even by a pixel whose own ident were EMPTY's bits: it is inert
        return
    # just inside each bound the tap is kept
    pg = [a.copy() for a in flat(P4)]
    pg[0][y, x] = (0.0, 0.4375, 0.90625)  # dot 0.90625 >= 0.9
    pg[1][y, x, 2] += F(0.03125)          # e = 0.03125 * 1 <= 0.04
    out, c = run(P4, hist(7), pg=pg)
    expect(out, c, FOUR, hist(7))


def test_without_normals_the_plane_test_is_the_distance():
    prev = hist(8)
    g = (None,) + flat(P4)[1:]
    color = np.tile(np.array((0.25, 0.5, 0.75), F), (H4, W8, 1))
    for off, kept in ((0.03125, True), (0.0625, False)):
        pg = [None, flat(P4)[1].copy(), flat(P4)[2]]
        pg[1][1, 3, 0] += F(off)  # along the plane: the tangent-plane test would keep both
        out = AR.accumulate(color, g, dict(prev, cam=ORIGIN, guides=pg))
        expect(out, color[0, 0], FOUR if kept else [t for t in FOUR if t[:2] != (3, 1)], prev)


@pytest.mark.parametrize("where,bad", [(a, b) for a in ("color", "normal", "position") for b in (np.nan, np.inf, -np.inf)]
                         + [("ident", None)])
def test_an_inert_pixel_keeps_its_bits_and_is_no_tap(where, bad):
    from atray_amd import engine as E
    w, h = 13, 11
    cam = E.camera(w, h)
    g = [a.copy() for a in two_planes(cam, nan=False)]
    c = noisy(h, w, 1, nan=False)
    live = g[2] != EMPTY
    ys, xs = np.nonzero(live)
    y, x = int(ys[len(ys) // 2]), int(xs[len(ys) // 2])
    if where == "ident":
        g[2][y, x] = EMPTY
    else:
        {"color": c, "normal": g[0], "position": g[1]}[where][y, x, 1] = bad
    first = AR.accumulate(c, g, None)
    assert AR.same_bits(first["color"][y, x], c[y, x]) and first["length"][y, x] == 0
    assert first["variance"][y, x] == 0 and (first["moments"][y, x] == 0).all()
    assert first["framebuffer"][y, x] == np_framebuffer(c)[y, x]
    live[y, x] = False
    assert live.sum() > 20 and (first["length"][live] == 1).all() and AR.same_bits(first["color"][live], c[live])
    # the next frame from the same camera, that pixel live again: nothing of its inert history is read
    g2 = two_planes(cam, nan=False)
    c2 = noisy(h, w, 2, nan=False)
    second = AR.accumulate(c2, g2, AR.history(first, cam, g))
    other = AR.history(first, cam, g)
    other["color"] = first["color"].copy()
    other["color"][y, x] = (7.0, 8.0, 9.0)
    other["moments"] = first["moments"].copy()
    other["moments"][y, x] = (3.0, 4.0)
    assert same(second, AR.accumulate(c2, g2, other))
    assert second["length"][y, x] in (1, 2) and (second["length"][live] == 2).all()
    assert np.isfinite(second["color"]).all()


def test_starting_a_history():
    c = noisy(9, 14, 3)
    for g in [(None, None, None), (None, None, np.where(c[..., 0] > 1, EMPTY, 2).astype(np.uint32))]:
        out = AR.accumulate(c, g, None)
        assert same(out, np_accumulate(c, g, None))
        live = out["length"] == 1
        assert live.any() and (~live).any() and (out["length"][~live] == 0).all()
        assert AR.same_bits(out["color"], c)
        lum = (F(0.2126) * c[..., 0] + F(0.7152) * c[..., 1]) + F(0.0722) * c[..., 2]
        assert AR.same_bits(out["moments"][live], np.stack([lum, lum * lum], -1)[live])
        assert (out["variance"] == 0).all()
    bare = AR.accumulate(c, moments=False)
    assert bare["moments"] is None and bare["variance"] is None and AR.same_bits(bare["color"], c)


def test_a_camera_at_rest_counts_frames_and_saturates():
    from atray_amd import engine as E
    w, h = 40, 24
    cam = E.camera(w, h)
    outs = chain([cam] * 5, (h, w), nan=False)
    live = two_planes(cam, nan=False)[2] != EMPTY
    assert 100 < live.sum() < h * w
    for f, out in enumerate(outs):
        assert (out["length"][live] == f + 1).all() and (out["length"][~live] == 0).all()
    # the running mean of the five frames, to rounding, and a variance of the noise's order
    mean = np.mean([noisy(h, w, 100 + f, nan=False) for f in range(5)], axis=0)
    assert np.allclose(outs[4]["color"][live], mean[live], atol=1e-3)
    assert outs[4]["variance"][live].mean() > 0.01
    capped = chain([cam] * 5, (h, w), nan=False, max_length=3)
    assert [int(o["length"][live].max()) for o in capped] == [1, 2, 3, 3, 3]
    assert same(capped[2], outs[2]) and not same(capped[3], outs[3])
    # alpha = 1 returns the frame itself; max_length = 1 likewise
    for kw in (dict(alpha=1.0, alpha_moments=1.0), dict(max_length=1)):
        out = chain([cam] * 3, (h, w), nan=False, **kw)[2]
        # h + (c - h) * 1: two roundings of values below 1.5, 2 * 1.5 * 2^-24 each at the most
        assert np.allclose(out["color"], noisy(h, w, 102, nan=False), rtol=0, atol=4 * 1.5 * 2.0 ** -24)
        assert not (out["length"][live] == 1).any() or kw == dict(max_length=1)
        assert out["variance"][live].max() < 1e-6


def test_binding_and_defaults():
    from atray_amd import engine as E
    sig = E.signatures()
    assert {"atr_accumulate", "atr_accumulate_check", "atr_default_accumulate_params"} <= set(sig)
    args, res = sig["atr_accumulate"]
    assert len(args) == 13 and res is C.c_int
    assert C.sizeof(E.atr_accumulate_params) == 32 and C.sizeof(E.atr_history) == 3 * C.sizeof(C.c_void_p)
    p = E.atr_accumulate_params(9.0, 9.0, 9, 9.0, 9.0, (C.c_int32 * 3)(1, 2, 3))
    E.lib().atr_default_accumulate_params(C.byref(p))
    got = (p.alpha, p.alpha_moments, p.max_length, p.plane_tolerance, p.min_normal_dot, list(p.reserved))
    assert got == (0.0, 0.0, 64, float(F(0.02)), float(F(0.9)), [0] * 3)
    assert got[:5] == tuple(float(F(AR.DEFAULTS[k])) if k != "max_length" else AR.DEFAULTS[k] for k in
                            ("alpha", "alpha_moments", "max_length", "plane_tolerance", "min_normal_dot"))
    import inspect
    d = {k: v.default for k, v in inspect.signature(E.Engine.accumulate).parameters.items()}
    assert {k: d[k] for k in AR.DEFAULTS} == AR.DEFAULTS
    assert hasattr(E, "TemporalAccumulator")


def test_argument_rules():
    """atr_accumulate_check is atr_accumulate's validation on the host; the addresses are never followed."""
    from atray_amd import engine as E
    ok, inv = 0, -1

    def call(w=8, h=4, prev=True, color=0x1000, variance=0x9000, cam=None, params=None, **over):
        a = dict(gn=0x2000, gp=0x3000, gi=0x4000, pn=0x2100, pp=0x3100, pi=0x4100, hc=0x5000, hm=0x6000, hl=0x7000,
                 oc=0x5100, om=0x6100, ol=0x7100)
        a.update(over)
        g, pg = E.atr_denoise_guides(a["gn"], a["gp"], a["gi"]), E.atr_denoise_guides(a["pn"], a["pp"], a["pi"])
        hp, ho = E.atr_history(a["hc"], a["hm"], a["hl"]), E.atr_history(a["oc"], a["om"], a["ol"])
        cam = E.camera(8, 4) if cam is None else cam
        p = E.atr_accumulate_params(0.0, 0.0, 64, 0.02, 0.9) if params is None else params
        return E.lib().atr_accumulate_check(color, C.byref(g) if over.get("guides", 1) else None,
                                            C.byref(cam) if over.get("has_cam", 1) else None,
                                            C.byref(pg) if over.get("prev_guides", 1) else None,
                                            C.byref(hp) if prev else None, w, h, C.byref(p) if p else None,
                                            C.byref(ho) if over.get("out", 1) else None, variance)

    assert call() == ok
    assert call(color=None) == inv and call(params=False) == inv and call(out=0) == inv
    assert call(oc=None) == inv and call(ol=None) == inv
    for size in [(0, 4), (8, 0), (-1, 4), (16385, 4), (8, 16385)]:
        assert call(w=size[0], h=size[1], prev=False) == inv
    assert call(w=16384, h=16384, prev=False) == ok
    # without prev: no camera, no guides, no position needed
    assert call(prev=False, guides=0, has_cam=0, prev_guides=0) == ok
    assert call(prev=False, gp=None, gn=None) == ok
    # with prev
    assert call(has_cam=0) == inv and call(prev_guides=0) == inv and call(guides=0) == inv
    assert call(gp=None) == inv and call(pp=None) == inv and call(hc=None) == inv and call(hl=None) == inv
    assert call(gn=None) == inv and call(pn=None) == inv and call(gn=None, pn=None) == ok
    assert call(gi=None) == inv and call(pi=None) == inv and call(gi=None, pi=None) == ok
    assert call(hm=None) == inv and call(om=None) == inv and call(hm=None, om=None, variance=None) == ok
    assert call(hm=None, om=None) == inv and call(prev=False, om=None) == inv  # variance needs out->moments
    assert call(prev=False, om=None, variance=None) == ok
    assert call(oc=0x5000) == inv and call(om=0x6000) == inv and call(ol=0x7000) == inv
    assert call(oc=0x1000) == ok  # out->color == color
    assert call(cam=E.camera(9, 4)) == inv and call(cam=E.camera(8, 5)) == inv
    assert call(w=9, cam=E.camera(9, 4)) == ok
    for k in (0.0, -1.0, float("nan"), float("inf")):
        cam = E.camera(8, 4)
        cam.h_fov = k
        assert call(cam=cam) == inv
        assert call(cam=cam, prev=False) == ok
    P = E.atr_accumulate_params
    good = dict(alpha=0.0, alpha_moments=0.0, max_length=64, plane_tolerance=0.02, min_normal_dot=0.9)
    mk = lambda **kw: P(*[dict(good, **kw)[k] for k in good])  # noqa: E731
    nan, inf = float("nan"), float("inf")
    for prev in (True, False):
        for kw in [dict(alpha=1.0), dict(alpha_moments=1.0), dict(max_length=1), dict(max_length=1 << 24),
                   dict(min_normal_dot=-1.0), dict(min_normal_dot=1.0), dict(plane_tolerance=1e30)]:
            assert call(prev=prev, params=mk(**kw)) == ok, kw
        for kw in [dict(alpha=-0.1), dict(alpha=1.5), dict(alpha=nan), dict(alpha_moments=-0.1), dict(alpha_moments=1.5),
                   dict(alpha_moments=nan), dict(max_length=0), dict(max_length=-3), dict(max_length=(1 << 24) + 1),
                   dict(plane_tolerance=0.0), dict(plane_tolerance=-1.0), dict(plane_tolerance=nan),
                   dict(plane_tolerance=inf), dict(min_normal_dot=-1.5), dict(min_normal_dot=1.5),
                   dict(min_normal_dot=nan)]:
            assert call(prev=prev, params=mk(**kw)) == inv, kw
        for k in range(3):
            r = (C.c_int32 * 3)()
            r[k] = 1
            assert call(prev=prev, params=P(0.0, 0.0, 64, 0.02, 0.9, r)) == inv
    # the entry point itself: a NULL context is refused before anything else
    p = mk()
    ho = E.atr_history(0x5100, 0x6100, 0x7100)
    assert E.lib().atr_accumulate(None, 0x1000, None, None, None, None, 8, 4, C.byref(p), C.byref(ho), None, None,
                                  None) == inv


def monkey_guides(s, fn, w, h, eye, facing):
    """Guides from the oracle's primary hits: position = eye + d * t, flat face normals turned towards
    the eye, ident 0 / EMPTY."""
    from atray_amd import engine as E
    face, t, _ = s.primary_hits(O.Camera(w, h, eye=eye, facing=facing))
    hit = face != 0xFFFFFFFF
    cam = E.camera(w, h, eye=eye, facing=facing)
    orig, dirs = E.camera_rays(cam)
    with np.errstate(all="ignore"):  # a miss has t = the largest float
        position = (orig + dirs * t.reshape(-1, 1)).astype(F).reshape(h, w, 3)
    normal = fn[np.where(hit, face, 0).reshape(-1)].reshape(h, w, 3)
    toward = (normal * -dirs.reshape(h, w, 3)).sum(2) < 0
    normal = np.where(toward[..., None], -normal, normal).astype(F)
    position[~hit] = 0
    return cam, (normal, position, np.where(hit, 0, 0xFFFFFFFF).astype(np.uint32)), hit


def monkey_orbit(w, h, frames, step, mat, spp=1, seed=0x853C49E6748FEA9B, **params):
    """Accumulates `frames` 1-spp frames of the orbit; returns (mse of the last frame, mse of the
    accumulated last frame, hit pixels), both against that camera's 256-spp render over its hit pixels."""
    from atray_amd import engine as E
    from atray_amd.assets import CENTERS, asset_path
    s = O.Scene(asset_path("Monkey"), center=CENTERS["Monkey"], materials=(O.SKY, mat))
    m = E.Mesh.load_obj(asset_path("Monkey"))
    m.translate_to(m.aabb(), CENTERS["Monkey"])
    arr = m.arrays()
    V, FV = arr[0], arr[3]
    v0, v1, v2 = (V[FV[:, k]] for k in range(3))
    fn = np.cross(v0 - v1, v0 - v2).astype(F)
    fn = fn / np.sqrt((fn * fn).sum(1, keepdims=True)).astype(F)
    prev = None
    for f in range(frames):
        eye, facing = orbit(f, step)
        cam, g, hit = monkey_guides(s, fn, w, h, eye, facing)
        frame = s.render(O.Camera(w, h, spp=spp, bounces=3, eye=eye, facing=facing), seed + f)[0]
        out = AR.accumulate(frame, g, prev, **params)
        prev = AR.history(out, cam, g)
    clean = s.render(O.Camera(w, h, spp=256, bounces=3, eye=eye, facing=facing), seed)[0]
    assert AR.same_bits(out["color"][~hit], frame[~hit])
    mse = lambda a: float(((a[hit].astype(np.float64) - clean[hit]) ** 2).mean())  # noqa: E731
    return mse(frame), mse(out["color"]), int(hit.sum()), out


def test_the_defaults_lower_the_error_of_an_orbit_of_noisy_frames():
    """A condition on the defaults, not a measurement: the oracle's Monkey with the model material's
    scatter set to 0 (diffuse), 72 x 40, 1 spp, 3 bounces, seed 0x853C49E6748FEA9B + f, 8 frames of an
    orbit about the model's centre at 0.02 rad per frame, guides from the oracle's primary hits; the
    accumulated last frame is strictly closer (mean squared error over its hit pixels) to that camera's
    256-spp render than the 1-spp frame is. DESIGN.md §4t has the values."""
    e, r, _ = O.MODEL_MAT
    before, after, nhit, out = monkey_orbit(72, 40, 8, 0.02, (e, r, 0.0))
    print(f"mse over {nhit} hit pixels: 1 spp {before:.3e}, accumulated {after:.3e}; "
          f"lengths {np.bincount(out['length'].ravel())}")
    assert 100 < nhit < 72 * 40
    assert after < before
