"""The denoiser's plain C reference (tests/denoise_ref.py) pinned without a GPU, so that it is not its own
only witness: values worked by hand, a vectorised numpy-f32 restatement of include/atray.h's formulas
tap by tap, the inert and ident rules, the kc/kp rejection rule, the binding, and one condition on the
defaults: they lower the error of a 4-spp render of the oracle against its 256-spp render."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests import denoise_ref as DR

F = np.float32
H5 = [F(0.0625), F(0.25), F(0.375), F(0.25), F(0.0625)]
EMPTY = np.uint32(0xFFFFFFFF)


def np_denoise(color, normal=None, position=None, ident=None, passes=5, sigma_color=0.01, sigma_position=0.0,
               normal_power_log2=5):
    """atray.h's formulas on whole images, one tap at a time in the stated order; every numpy f32
    operation is separately rounded."""
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
    with np.errstate(all="ignore"):
        for p in range(passes):
            s = 1 << p
            sc = F(sigma_color) / F(s)
            kc = F(1.0) / (sc * sc)
            sp = F(sigma_position) * F(s)
            kp = F(1.0) / (sp * sp)
            total, wsum = np.zeros((h, w, 3), F), np.zeros((h, w), F)
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qx, qy = X + dx * s, Y + dy * s
                    ok = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                    qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
                    ok &= ~inert[qy, qx]
                    if ident is not None:
                        ok &= ident[qy, qx] == ident
                    cq = cur[qy, qx]
                    wt = np.full((h, w), H5[dy + 2] * H5[dx + 2], F)
                    if normal is not None:
                        c = dot(normal, normal[qy, qx])
                        c = np.where(c > 0, c, F(0.0))
                        for _ in range(normal_power_log2):
                            c = c * c
                        wt = wt * c
                    if position is not None and sigma_position > 0:
                        dv = position[qy, qx] - position
                        if normal is not None:
                            e = dot(normal, dv)
                            e2 = e * e
                        else:
                            e2 = dot(dv, dv)
                        wt = wt * (F(1.0) / (F(1.0) + e2 * kp))
                    if sigma_color > 0:
                        dc = cq - cur
                        wt = wt * (F(1.0) / (F(1.0) + dot(dc, dc) * kc))
                    use = ok & (wt > 0)
                    total = np.where(use[..., None], total + cq * wt[..., None], total)
                    wsum = np.where(use, wsum + wt, wsum)
            new = total / wsum[..., None]
            cur = np.where((~inert & (wsum > 0))[..., None], new, cur).astype(F)
    return cur


def np_framebuffer(img):
    """The renderer's clamp and quantisation (a NaN gives 0)."""
    with np.errstate(all="ignore"):
        k = np.where(img > 1, F(1.0), img)     # pl_min(c, 1) = c > 1 ? 1 : c
        k = np.where(F(0.0) > k, F(0.0), k)    # pl_max(0, k) = 0 > k ? 0 : k
        q = np.where(np.isnan(k), 0, (np.nan_to_num(k) * F(255.0)).astype(np.uint32) & 0xFF).astype(np.uint32)
    return q[..., 2] | (q[..., 1] << 8) | (q[..., 0] << 16)


def scene(h, w, seed=1, nan=True):
    """A random image with all guides: colours, roughly unit normals of two directions, positions, three
    ids in blocks; some EMPTY, NaN and inf pixels."""
    r = np.random.default_rng(seed)
    color = r.random((h, w, 3), dtype=F) * F(2.0)
    ident = ((np.arange(w)[None, :] // 7 + np.arange(h)[:, None] // 5) % 3).astype(np.uint32)
    base = np.array([[0, 0, 1], [0.6, 0, 0.8], [0, 1, 0]], F)
    normal = (base[ident] + (r.random((h, w, 3), dtype=F) - F(0.5)) * F(0.2)).astype(F)
    position = (np.stack(np.meshgrid(np.arange(w), np.arange(h)), -1).astype(F) * F(0.1))
    position = np.concatenate([position, r.random((h, w, 1), dtype=F)], -1).astype(F)
    if nan and h * w > 12:
        ident[r.integers(h), r.integers(w)] = EMPTY
        color[r.integers(h), r.integers(w), 1] = np.nan
        color[r.integers(h), r.integers(w), 2] = np.inf
        normal[r.integers(h), r.integers(w), 0] = -np.inf
        position[r.integers(h), r.integers(w), 2] = np.nan
    return color, normal, position, ident


def test_one_pixel_is_returned_at_every_pass_count():
    c = np.array([[[0.25, 3.5, -1.0]]], F)
    for passes in range(1, 9):
        for sc in (0.0, 1.0):
            out, fb = DR.denoise(c, passes=passes, sigma_color=sc)
            assert DR.same_bits(out, c)
            assert fb[0, 0] == (0 | (255 << 8) | (63 << 16))  # b = 0 (clamped), g = 255, r = uint(63.75)


def by_hand_row(c):
    """One pass on a 5-pixel row without guides and with the colour term off, pixel by pixel: the taps
    inside the row in the order dx = -2..2, w = h[2] * h[dx + 2]."""
    taps = {0: [(0, 2), (1, 3), (2, 4)], 1: [(0, 1), (1, 2), (2, 3), (3, 4)], 2: [(0, 0), (1, 1), (2, 2), (3, 3), (4, 4)],
            3: [(1, 0), (2, 1), (3, 2), (4, 3)], 4: [(2, 0), (3, 1), (4, 2)]}
    out = np.zeros((5, 3), F)
    for x, lst in taps.items():
        total, wsum = np.zeros(3, F), F(0.0)
        for q, k in lst:
            wt = H5[2] * H5[k]
            total = total + c[q] * wt
            wsum = wsum + wt
        out[x] = total / wsum
    return out


def test_rows_by_hand():
    c = np.array([[1.0, 0.5, 0.1], [0.3, 0.7, 0.2], [0.9, 0.1, 0.6], [0.2, 0.4, 0.8], [0.55, 0.35, 0.15]], F)
    want = by_hand_row(c)
    # the edge pixels' truncated sets by their numbers: pixel 0 sees the weights 9/64, 3/32, 3/128
    w0 = [F(0.140625), F(0.09375), F(0.0234375)]
    e = ((c[0] * w0[0] + c[1] * w0[1]) + c[2] * w0[2]) / ((w0[0] + w0[1]) + w0[2])
    assert DR.same_bits(want[0], e.astype(F))
    row, _ = DR.denoise(c.reshape(1, 5, 3), passes=1, sigma_color=0.0)
    col, _ = DR.denoise(c.reshape(5, 1, 3), passes=1, sigma_color=0.0)
    assert DR.same_bits(row.reshape(5, 3), want)
    assert DR.same_bits(col.reshape(5, 3), want)
    # pass 2 has spacing 2: pixel 0 sees itself, pixel 2 and pixel 4
    two, _ = DR.denoise(c.reshape(1, 5, 3), passes=2, sigma_color=0.0)
    w = [H5[2] * H5[2], H5[2] * H5[3], H5[2] * H5[4]]
    p0 = ((want[0] * w[0] + want[2] * w[1]) + want[4] * w[2]) / ((w[0] + w[1]) + w[2])
    assert DR.same_bits(two[0, 0], p0.astype(F))


def test_numpy_restatement_equals_the_reference_in_bits():
    color, normal, position, ident = scene(23, 37)
    kw = dict(passes=3, sigma_color=0.8, sigma_position=0.3, normal_power_log2=3)
    out, fb = DR.denoise(color, normal, position, ident, **kw)
    want = np_denoise(color, normal, position, ident, **kw)
    assert DR.same_bits(out, want)
    assert np.array_equal(fb, np_framebuffer(want))
    # and the other branches: no normal (the Euclidean distance), no guides at all
    kw = dict(passes=2, sigma_color=0.5, sigma_position=0.7)
    assert DR.same_bits(DR.denoise(color, None, position, None, **kw)[0], np_denoise(color, None, position, None, **kw))
    assert DR.same_bits(DR.denoise(color, passes=4)[0], np_denoise(color, passes=4))
    assert not DR.same_bits(out, color)


def test_nothing_leaks_across_ids():
    color, normal, position, ident = scene(23, 37, seed=2, nan=False)
    a = ident == 0
    other = color.copy()
    other[~a] = np.random.default_rng(5).random((int((~a).sum()), 3), dtype=F) * F(9.0)
    kw = dict(passes=4, sigma_color=1.0, sigma_position=0.5)
    x, _ = DR.denoise(color, normal, position, ident, **kw)
    y, _ = DR.denoise(other, normal, position, ident, **kw)
    assert DR.same_bits(x[a], y[a]) and not DR.same_bits(x[~a], y[~a])


@pytest.mark.parametrize("where", ["color", "normal", "position"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_an_inert_pixel_keeps_its_bits_and_is_no_tap(where, bad):
    color, normal, position, _ = scene(11, 13, seed=3, nan=False)
    g = {"color": color, "normal": normal, "position": position}
    g[where][5, 6, 1] = bad
    ident = np.zeros((11, 13), np.uint32)
    kw = dict(passes=3, sigma_color=1.0, sigma_position=0.5)
    out, _ = DR.denoise(color, normal, position, ident, **kw)
    assert DR.same_bits(out[5, 6], color[5, 6])
    marked = ident.copy()
    marked[5, 6] = EMPTY
    clean = {k: v.copy() for k, v in g.items()}
    clean[where][5, 6, 1] = F(0.5)
    ref, _ = DR.denoise(clean["color"], clean["normal"], clean["position"], marked, **kw)
    keep = np.ones((11, 13), bool)
    keep[5, 6] = False
    assert DR.same_bits(out[keep], ref[keep])
    assert np.isfinite(out[keep]).all()


def test_three_by_three_with_eight_passes():
    color, normal, position, ident = scene(3, 3, seed=4, nan=False)
    ident[:] = 0
    kw = dict(sigma_color=1.0, sigma_position=0.5)
    two, _ = DR.denoise(color, normal, position, ident, passes=2, **kw)
    # from pass 2 on (spacing 4) every tap but the centre lies outside: sum / wsum of the one tap
    for passes in (3, 8):
        out, _ = DR.denoise(color, normal, position, ident, passes=passes, **kw)
        assert DR.same_bits(out, np_denoise(color, normal, position, ident, passes=passes, **kw))
        # (c * w) / w: two roundings per pass and channel, six passes at the most
        assert np.allclose(out, two, rtol=12 * 2.0 ** -23, atol=0)


def test_constants_rule():
    """kc = 1 / (sigma_color / s)^2 and kp = 1 / (sigma_position * s)^2 in f32; a term that is on needs
    every pass's constant finite and > 0."""
    rc, kc, kp = DR.constants(8, 1.0, 0.5)
    assert rc == 0
    assert np.array_equal(kc, np.array([4.0 ** p for p in range(8)], F))
    assert np.array_equal(kp, np.array([4.0 / 4.0 ** p for p in range(8)], F))

    def rule(passes, sc, sp, given=True):
        with np.errstate(all="ignore"):
            for p in range(passes):
                s = F(1 << p)
                a, b = F(sc) / s, F(sp) * s
                kc, kp = F(1.0) / (a * a), F(1.0) / (b * b)
                if sc > 0 and not (np.isfinite(kc) and kc > 0):
                    return -1
                if given and sp > 0 and not (np.isfinite(kp) and kp > 0):
                    return -1
        return 0

    cases = [(1, 1e-30, 0.0), (1, 1e30, 0.0), (8, 1e17, 0.0), (1, 1e17, 0.0), (1, 0.0, 1e-30), (1, 0.0, 1e30),
             (8, 0.0, 1e17), (1, 0.0, 1e17), (8, 1e-17, 0.0), (8, 0.0, 1e-17), (8, 0.0, 0.0), (5, 1.0, 0.0),
             (8, 3e-20, 0.0), (2, 0.0, 3e-20)]
    got = [DR.constants(p, sc, sp)[0] for p, sc, sp in cases]
    assert got == [rule(p, sc, sp) for p, sc, sp in cases]
    assert -1 in got and 0 in got
    assert got[:2] == [-1, -1] and got[4:6] == [-1, -1]
    # the position term is off without the guide, whatever its sigma
    assert DR.constants(1, 0.0, 1e-30, position_given=False)[0] == 0
    c = np.zeros((2, 2, 3), F)
    assert DR.denoise(c, sigma_color=1e-30) is None
    assert DR.denoise(c, sigma_position=1e-30) is not None
    assert DR.denoise(c, position=c, sigma_position=1e-30) is None


def test_binding_and_defaults():
    from atray_amd import engine as E
    sig = E.signatures()
    assert "atr_denoise" in sig and "atr_default_denoise_params" in sig
    args, res = sig["atr_denoise"]
    assert len(args) == 9 and res is C.c_int
    assert C.sizeof(E.atr_denoise_params) == 32 and C.sizeof(E.atr_denoise_guides) == 3 * C.sizeof(C.c_void_p)
    p = E.atr_denoise_params(9, 9.0, 9.0, 9, (C.c_int32 * 4)(1, 2, 3, 4))
    E.lib().atr_default_denoise_params(C.byref(p))
    assert (p.passes, p.sigma_color, p.sigma_position, p.normal_power_log2, list(p.reserved)) == (5, float(F(0.01)), 0.0, 5, [0] * 4)
    assert E.ATR_DENOISE_EMPTY == 0xFFFFFFFF
    import inspect
    d = {k: v.default for k, v in inspect.signature(E.Engine.denoise).parameters.items()}
    assert (d["passes"], d["sigma_color"], d["sigma_position"], d["normal_power_log2"]) == (5, 0.01, 0.0, 5)


def test_the_defaults_lower_the_error_of_a_noisy_render():
    """A condition on the defaults, not a measurement: on the oracle's Monkey at 72 x 40, 3 bounces, no
    anti-aliasing, with guides from the oracle's primary hits (position = eye + d * t, flat face normals,
    ident 0 / EMPTY), the filtered 4-spp render is strictly closer (mean squared error over the hit
    pixels) to the 256-spp render than the 4-spp render is.

    The defaults are set by this condition. The Monkey covers 19 x 18 pixels of this frame, so nearly
    every pixel shows a face of its own (signal sd 0.166), and the 4-spp noise is small beside it (rms
    0.008): the mean squared error over the 200 hit pixels is 6.65e-5 unfiltered, 6.44e-5 with the
    defaults (sigma_color 0.01), and 2.53e-4 with a colour tolerance on the scale of the signal
    (sigma_color 1). DESIGN.md §4s has the table."""
    from atray_amd import engine as E
    from atray_amd.assets import CENTERS, asset_path
    W, Hh, seed = 72, 40, 0x853C49E6748FEA9B
    s = O.Scene(asset_path("Monkey"), center=CENTERS["Monkey"])
    noisy = s.render(O.Camera(W, Hh, spp=4, bounces=3), seed)[0]
    clean = s.render(O.Camera(W, Hh, spp=256, bounces=3), seed)[0]
    face, t, _ = s.primary_hits(O.Camera(W, Hh))
    hit = face != 0xFFFFFFFF
    assert 100 < hit.sum() < W * Hh
    orig, dirs = E.camera_rays(E.camera(W, Hh))
    with np.errstate(all="ignore"):  # a miss has t = the largest float
        position = (orig + dirs * t.reshape(-1, 1)).astype(F).reshape(Hh, W, 3)
    m = E.Mesh.load_obj(asset_path("Monkey"))
    m.translate_to(m.aabb(), CENTERS["Monkey"])
    arr = m.arrays()
    V, FV = arr[0], arr[3]
    v0, v1, v2 = (V[FV[:, k]] for k in range(3))
    fn = np.cross(v0 - v1, v0 - v2).astype(F)
    fn = fn / np.sqrt((fn * fn).sum(1, keepdims=True)).astype(F)
    normal = fn[np.where(hit, face, 0).reshape(-1)].reshape(Hh, W, 3)
    toward = (normal * -dirs.reshape(Hh, W, 3)).sum(2) < 0
    normal = np.where(toward[..., None], -normal, normal).astype(F)
    ident = np.where(hit, 0, 0xFFFFFFFF).astype(np.uint32)
    position[~hit] = 0
    out, _ = DR.denoise(noisy, normal, position, ident)  # the defaults
    assert DR.same_bits(out[~hit], noisy[~hit])
    mse = lambda a: float(((a[hit].astype(np.float64) - clean[hit]) ** 2).mean())  # noqa: E731
    before, after = mse(noisy), mse(out)
    print(f"mse over {int(hit.sum())} hit pixels: 4 spp {before:.6f}, denoised {after:.6f}")
    assert after < before
