"""atr_denoise on the GPU: `out` and `framebuffer` for exact equality with the plain C reference of
tests/denoise_ref.py (pinned without a GPU in tests/test_denoise_cpu.py), at the edges of the pass
kernel's 64 x 4 blocks, for every guide subset, pass count and term, with inert pixels of every kind, in
place, on two streams, on a rendered frame with render_guides, and in bake_lightmap; the arguments. Every
raw output buffer is filled with a sentinel first and guarded on both sides. Needs an MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from atray_amd.assets import CENTERS, asset_path  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import denoise_ref as DR  # noqa: E402
from tests.test_denoise_cpu import scene  # noqa: E402
from tests.test_gpu_parity import eng, run, upload  # noqa: E402,F401

pytestmark = pytest.mark.gpu
F = np.float32
G = 256  # guard bytes around every raw output buffer
FILL = 0xAB
EMPTY = np.uint32(0xFFFFFFFF)
ON = dict(sigma_color=0.8, sigma_position=0.4, normal_power_log2=3)


def dev():
    return torch.device("cuda", 0)


def up(a):
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(dev())


def raw(eng, color, normal=None, position=None, ident=None, want=("out", "fb"), guides=True, stream=None,  # noqa: F811
        params=None, size=None, **kw):
    """atr_denoise through ctypes on guarded, sentinel-filled buffers: (rc, out or None, fb or None)."""
    h, w = color.shape[:2] if size is None else size
    t = [up(a) for a in (color, normal, position, ident)]
    n = color.shape[0] * color.shape[1]
    buf = {"out": torch.full((n * 12 + 2 * G,), FILL, dtype=torch.uint8, device=dev()),
           "fb": torch.full((n * 4 + 2 * G,), FILL, dtype=torch.uint8, device=dev())}
    g = E.atr_denoise_guides(*[a.data_ptr() if a is not None else None for a in t[1:]])
    p = params
    if p is None:
        p = E.atr_denoise_params(kw.get("passes", 5), kw.get("sigma_color", 0.01), kw.get("sigma_position", 0.0),
                                 kw.get("normal_power_log2", 5))
    torch.cuda.synchronize()
    rc = E.lib().atr_denoise(eng.h, C.c_void_p(t[0].data_ptr()), C.byref(g) if guides else None, w, h,
                             C.byref(p) if p else None,
                             C.c_void_p(buf["out"].data_ptr() + G) if "out" in want else None,
                             C.c_void_p(buf["fb"].data_ptr() + G) if "fb" in want else None,
                             C.c_void_p(stream) if stream else None)
    wrc, done = eng.wait()
    assert wrc == 0 and done == 0
    torch.cuda.synchronize()
    res = []
    for k, per, dt in (("out", 12, F), ("fb", 4, np.uint32)):
        a = buf[k].cpu().numpy()
        assert (a[:G] == FILL).all() and (a[G + n * per:] == FILL).all(), (k, "guard bytes")
        body = a[G:G + n * per]
        if rc != 0 or k not in want:
            assert (body == FILL).all(), (k, "written")
            res.append(None)
        else:
            res.append(body.view(dt).reshape((color.shape[0], color.shape[1], 3) if k == "out" else color.shape[:2]).copy())
    return rc, res[0], res[1]


def check(eng, color, normal=None, position=None, ident=None, **kw):  # noqa: F811
    rc, out, fb = raw(eng, color, normal, position, ident, **kw)
    assert rc == 0
    want, wfb = DR.denoise(color, normal, position, ident, **kw)
    assert DR.same_bits(out, want)
    assert np.array_equal(fb, wfb)
    return out


# 63/64/65 and 3/4/5: one below, at and one above the pass kernel's block of 64 x 4 pixels
@pytest.mark.parametrize("w,h", [(1, 1), (1, 7), (7, 1), (5, 5), (63, 3), (64, 4), (65, 5), (130, 67), (64, 3), (63, 5),
                                 (65, 4), (128, 8), (129, 9)])
def test_sizes(eng, w, h):  # noqa: F811
    color, normal, position, ident = scene(h, w, seed=w * 131 + h)
    out = check(eng, color, normal, position, ident, passes=3, **ON)
    if w * h > 1:
        assert not DR.same_bits(out, color)
    check(eng, color, passes=2)


def test_eight_passes_on_a_larger_image(eng):  # noqa: F811
    color, normal, position, ident = scene(131, 257, seed=9)
    check(eng, color, normal, position, ident, passes=8, **ON)


@pytest.mark.parametrize("subset", range(8))
def test_every_guide_subset_with_the_colour_term_on_and_off(eng, subset):  # noqa: F811
    color, normal, position, ident = scene(33, 65, seed=11)
    g = dict(normal=normal if subset & 1 else None, position=position if subset & 2 else None,
             ident=ident if subset & 4 else None)
    outs = [check(eng, color, passes=3, sigma_color=sc, sigma_position=0.4, normal_power_log2=3, **g)
            for sc in (0.0, 0.8)]
    assert not DR.same_bits(outs[0], outs[1])


@pytest.mark.parametrize("passes", range(1, 9))
def test_pass_counts(eng, passes):  # noqa: F811
    color, normal, position, ident = scene(33, 65, seed=12)
    check(eng, color, normal, position, ident, passes=passes, **ON)


@pytest.mark.parametrize("power", [0, 3, 7])
def test_normal_powers(eng, power):  # noqa: F811
    color, normal, position, ident = scene(33, 65, seed=13)
    check(eng, color, normal, position, ident, passes=3, sigma_color=0.8, sigma_position=0.4, normal_power_log2=power)
    check(eng, color, normal, passes=2, sigma_color=0.0, normal_power_log2=power)


def test_position_term_without_normals_and_switched_off(eng):  # noqa: F811
    color, _, position, ident = scene(33, 65, seed=14)
    a = check(eng, color, None, position, ident, passes=3, sigma_color=0.5, sigma_position=0.3)  # Euclidean
    b = check(eng, color, None, position, ident, passes=3, sigma_color=0.5, sigma_position=0.0)  # inertness only
    c = check(eng, color, None, None, ident, passes=3, sigma_color=0.5)
    assert not DR.same_bits(a, b) and not DR.same_bits(b, c)  # a NaN position makes its pixel inert in b only


def test_inert_images(eng):  # noqa: F811
    color, normal, position, ident = scene(19, 70, seed=15, nan=False)
    # all inert: the input comes back
    out = check(eng, color, normal, position, np.full_like(ident, EMPTY), passes=4, **ON)
    assert DR.same_bits(out, color)
    # one live pixel: it is its own only tap
    one = np.full_like(ident, EMPTY)
    one[7, 33] = 5
    check(eng, color, normal, position, one, passes=4, **ON)
    # a checkerboard of two ids: at spacing 1 only every other tap counts, from spacing 2 on all of them
    yy, xx = np.mgrid[0:19, 0:70]
    board = ((xx + yy) & 1).astype(np.uint32) + 7
    check(eng, color, normal, position, board, passes=3, **ON)
    check(eng, color, None, None, board, passes=2, sigma_color=0.0)


@pytest.mark.parametrize("where", ["color", "normal", "position"])
def test_nan_and_inf_in_each_input(eng, where):  # noqa: F811
    color, normal, position, ident = scene(19, 70, seed=16, nan=False)
    g = {"color": color, "normal": normal, "position": position}
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        g[where][3 + 5 * k, 10 + 20 * k, k] = bad
    out = check(eng, color, normal, position, ident, passes=4, **ON)
    for k in range(3):
        assert DR.same_bits(out[3 + 5 * k, 10 + 20 * k], color[3 + 5 * k, 10 + 20 * k])
    live = np.isfinite(color).all(2) & np.isfinite(normal).all(2) & np.isfinite(position).all(2)
    assert np.isfinite(out[live]).all()


def test_in_place_framebuffer_alone_and_no_guides(eng):  # noqa: F811
    color, normal, position, ident = scene(37, 101, seed=17)
    kw = dict(passes=4, **ON)
    want, wfb = DR.denoise(color, normal, position, ident, **kw)
    tc, tn, tp, ti = (up(a) for a in (color, normal, position, ident))
    sep, fb = eng.denoise(tc, tn, tp, ti, framebuffer=True, **kw)
    same = eng.denoise(tc, tn, tp, ti, out=tc, **kw)  # out == color
    rc, _ = eng.wait()
    assert rc == 0
    torch.cuda.synchronize()
    assert same.data_ptr() == tc.data_ptr()
    assert DR.same_bits(sep.cpu().numpy(), want) and DR.same_bits(tc.cpu().numpy(), want)
    assert np.array_equal(fb.cpu().numpy().view(np.uint32), wfb)
    # the framebuffer alone (out NULL); guides NULL equals a guides record of three NULLs
    rc, out, fb = raw(eng, color, normal, position, ident, want=("fb",), **kw)
    assert rc == 0 and out is None and np.array_equal(fb, wfb)
    rc, out, fb = raw(eng, color, guides=False, passes=3)
    w3, f3 = DR.denoise(color, passes=3)
    assert rc == 0 and DR.same_bits(out, w3) and np.array_equal(fb, f3)
    rc, out, _ = raw(eng, color, want=("out",), passes=3)
    assert rc == 0 and DR.same_bits(out, w3)


def test_a_rendered_frame_with_its_guides(eng):  # noqa: F811
    upload(eng, "Monkey")
    cam = E.camera(96, 54, 4, 3)
    frame = run(eng, cam)
    normal, position, ident = eng.render_guides(cam)
    color = torch.from_numpy(frame["rgb"]).to(dev())
    out, fb = eng.denoise(color, normal, position, ident, sigma_position=0.2, framebuffer=True)
    rc, _ = eng.wait()
    assert rc == 0
    torch.cuda.synchronize()
    n, p, i = normal.cpu().numpy(), position.cpu().numpy(), ident.cpu().numpy().view(np.uint32)
    hit = frame["face"] != E.MISS
    assert 100 < hit.sum() < hit.size
    assert np.array_equal(i == EMPTY, ~hit)
    assert set(np.unique(i[hit])) == {(E.ATR_RAY_TRI << 28) | 1}
    assert np.allclose((n[hit] * n[hit]).sum(1), 1, atol=1e-5) and np.isfinite(p[hit]).all()
    want, wfb = DR.denoise(frame["rgb"], n, p, i, sigma_position=0.2)
    assert DR.same_bits(out.cpu().numpy(), want)
    assert np.array_equal(fb.cpu().numpy().view(np.uint32), wfb)
    assert DR.same_bits(want[~hit], frame["rgb"][~hit]) and not DR.same_bits(want[hit], frame["rgb"][hit])
    assert np.array_equal(wfb[~hit], frame["fb"][~hit])  # an inert pixel's framebuffer is the render's own


def test_two_sizes_back_to_back_on_two_streams(eng):  # noqa: F811
    """On a fresh context: the second, larger call grows the workspace behind the first, the third (small
    again, on the first stream) waits for the second on the GPU."""
    e2 = E.Engine(0)
    try:
        a, b = scene(21, 50, seed=18), scene(90, 333, seed=19)
        kw = dict(passes=5, **ON)
        s1, s2 = torch.cuda.Stream(device=dev()), torch.cuda.Stream(device=dev())
        ta, tb = [up(x) for x in a], [up(x) for x in b]
        torch.cuda.synchronize()
        o1 = e2.denoise(*ta, stream=s1.cuda_stream, **kw)
        o2 = e2.denoise(*tb, stream=s2.cuda_stream, **kw)
        o3 = e2.denoise(*ta, stream=s1.cuda_stream, **kw)
        rc, done = e2.wait()
        assert rc == 0 and done == 0
        ms = e2.last_kernel_ms()
        assert 0 < ms < 1000
        torch.cuda.synchronize()
        wa, wb = DR.denoise(*a, **kw)[0], DR.denoise(*b, **kw)[0]
        assert DR.same_bits(o1.cpu().numpy(), wa) and DR.same_bits(o3.cpu().numpy(), wa)
        assert DR.same_bits(o2.cpu().numpy(), wb)
    finally:
        e2.close()


def test_kernel_time_is_valid_after_wait(eng):  # noqa: F811
    color, normal, position, ident = scene(67, 130, seed=20)
    check(eng, color, normal, position, ident, passes=5, **ON)
    assert 0 < eng.last_kernel_ms() < 1000


def test_invalid_arguments_leave_the_outputs_untouched(eng):  # noqa: F811
    color, normal, position, ident = scene(9, 12, seed=21)
    P = E.atr_denoise_params

    def bad(**kw):
        rc, out, fb = raw(eng, color, normal, position, ident, **kw)  # raw() asserts the sentinels
        return rc

    inv = -1  # ATR_E_INVALID
    assert bad(passes=3) == 0
    for p in (0, 9, -1):
        assert bad(passes=p) == inv
    for k in (-1, 8):
        assert bad(normal_power_log2=k) == inv
    for s in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert bad(sigma_color=s) == inv
        assert bad(sigma_position=s) == inv
    assert bad(sigma_color=1e-30) == inv and bad(sigma_position=1e-30) == inv  # kc, kp infinite
    assert bad(sigma_color=1e30) == inv and bad(sigma_position=1e30) == inv    # kc, kp zero
    # a later pass alone breaks the rule: (1e18 * 128)^2 overflows, (1e-18 / 128)^2 is below 1 / FLT_MAX
    assert bad(passes=1, sigma_position=1e18) == 0 and bad(passes=8, sigma_position=1e18) == inv
    assert bad(passes=1, sigma_color=1e-18) == 0 and bad(passes=8, sigma_color=1e-18) == inv
    assert bad(passes=8, sigma_color=1e17) == 0
    for k in range(4):
        r = (C.c_int32 * 4)()
        r[k] = 1
        assert bad(params=P(3, 1.0, 0.0, 5, r)) == inv
    assert bad(want=()) == inv  # out and framebuffer both NULL
    for size in [(0, 12), (9, 0), (-1, 12), (16385, 12), (9, 16385)]:
        assert bad(size=size) == inv
    # the position term is off without the guide: its sigma is still checked, its kp is not
    rc, _, _ = raw(eng, color, normal, None, ident, sigma_position=1e-30)
    assert rc == 0
    rc, _, _ = raw(eng, color, normal, None, ident, sigma_position=-1.0)
    assert rc == inv
    # NULL ctx, params, color
    t = up(color)
    o = torch.full((9 * 12 * 3,), 7.0, dtype=torch.float32, device=dev())
    p = P(3, 1.0, 0.0, 5)
    f = E.lib().atr_denoise
    vp = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731
    assert f(None, vp(t), None, 12, 9, C.byref(p), vp(o), None, None) == inv
    assert f(eng.h, None, None, 12, 9, C.byref(p), vp(o), None, None) == inv
    assert f(eng.h, vp(t), None, 12, 9, None, vp(o), None, None) == inv
    torch.cuda.synchronize()
    assert (o == 7.0).all()
    with pytest.raises(ValueError):
        eng.denoise(t.reshape(9, 12 * 3))
    with pytest.raises(ValueError):
        eng.denoise(t, normal=t[:, :6].contiguous())
    with pytest.raises(ValueError):
        eng.denoise(t, ident=torch.zeros((9, 12), dtype=torch.int64, device=dev()))
    with pytest.raises(ValueError):
        eng.denoise(t.cpu())


def test_bake_with_and_without_denoising(eng):  # noqa: F811
    """The Cube at 64 x 64, 16 visibility samples: with denoise={...} the bake equals the composition of
    its documented steps (the references' texels, the device's gathered values, the reference filter,
    the reference dilation); without the keyword it equals the bake as it was."""
    from tests import texel_ref as TX
    w = h = 64
    m = E.Mesh.load_obj(asset_path("Cube"))
    box = m.translate_to(m.aabb(), CENTERS["Cube"])
    cx, cy, cz = CENTERS["Cube"]
    spheres = [((cx + 0.3, cy + 1.6, cz), 0.9, 2)]
    mats = [O.SKY, O.MODEL_MAT, ((0.9, 0.7, 0.3), (0.6, 0.6, 0.6), 0.8)]
    eng.upload(mats, [(m, E.Octree.build(m, 300), box, 1)], spheres)
    seed = 0x853C49E6748FEA9B
    plain, tex = eng.bake_lightmap(m, w, h, 16, seed=seed)
    ref = TX.mesh_texels(m.arrays(), w, h)
    texel = tex["texel"].cpu().numpy()
    assert np.array_equal(texel, ref["texel"]) and len(texel) == 2709
    plain = plain.cpu().numpy()
    values = plain.reshape(-1, 3)[texel]  # the gathered values: the dilation leaves covered texels alone
    assert TX.same_bits(plain, TX.texels_to_image(values, texel, w, h, 2))
    kw = dict(passes=3, sigma_color=0.7, sigma_position=0.3, normal_power_log2=4)
    img, tex2 = eng.bake_lightmap(m, w, h, 16, seed=seed, denoise=kw)
    for key in TX.KEYS:
        assert TX.same_bits(tex2[key].cpu().numpy(), ref[key]), key
    zero = (0, 0, 0)
    col = TX.texels_to_image(values, texel, w, h, 0, zero)
    nim = TX.texels_to_image(ref["normal"], texel, w, h, 0, zero)
    pim = TX.texels_to_image(ref["point"], texel, w, h, 0, zero)
    ident = np.where(ref["slot"] >= 0, 0, 0xFFFFFFFF).astype(np.uint32).reshape(h, w)
    den, _ = DR.denoise(col, nim, pim, ident, **kw)
    want = TX.texels_to_image(den.reshape(-1, 3)[texel], texel, w, h, 2)
    assert TX.same_bits(img.cpu().numpy(), want)
    assert not TX.same_bits(img.cpu().numpy(), plain)
    again, _ = eng.bake_lightmap(m, w, h, 16, seed=seed, denoise=None)
    assert TX.same_bits(again.cpu().numpy(), plain)
    with pytest.raises(ValueError):
        eng.bake_lightmap(m, w, h, 16, seed=seed, denoise={"radius": 3})
