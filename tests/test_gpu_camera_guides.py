"""atr_camera_guides and atr_camera_rays on the GPU. normal, position and ident for equality in every
bit with Engine.render_guides(cam) -- the composition the call replaces: numpy camera_rays, atr_trace_rays,
torch arithmetic -- and depth and material with atr_trace_rays' t and material for the same rays (a NaN
equals a NaN; a valid camera gives none): on the Cube (flat normals), the Monkey (smooth normals: u and v),
a brute-force model, several models with a sphere and a plane and with coincident models, scenes without
models, an eye inside a mesh (whose back faces no ray hits), inside the sphere and under the plane (the
normal flip); at 1 x 1, 8 x 8, 13 x 7, 65 x 9 and 72 x 40, the
smallest frames with a partial 8 x 8 cell in x, in y and in both, and with more cells than one workgroup's
four waves. Tile lists, output subsets, streams, degenerate and rejected cameras, TemporalAccumulator. Every
output buffer is filled with a sentinel first and guarded on both sides. Needs an MI355X (-m gpu)."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from atray_amd.assets import CENTERS  # noqa: E402
from tests.test_accumulate_cpu import orbit  # noqa: E402
from tests.test_gpu_parity import eng, run, upload  # noqa: E402,F401
from tests.test_gpu_scenes import MATS, SPHERES, TIES, Sc  # noqa: E402

pytestmark = pytest.mark.gpu
SIZES = [(1, 1), (8, 8), (13, 7), (65, 9), (72, 40)]
NAMES = ("normal", "position", "ident", "depth", "material")
PER = {"normal": 3, "position": 3, "ident": 1, "depth": 1, "material": 1}
G = 64       # guard elements around every output buffer
FILL = -77   # the sentinel: -77.0f in the float outputs, -77 in the integer ones
# the Cube, the Monkey and a brute-force Cube that overlaps them, a sphere, and a floor close enough to be seen
MIXED = Sc(["cube", "monkey", "cube_bf"], [1, 2, 4], MATS, SPHERES, [((0.0, 1.0, 0.0), -2.5, 6)])
NO_MODELS = Sc([], [], MATS, SPHERES, [((0.0, 1.0, 0.0), -2.5, 6)])
EMPTY_SCENE = Sc([], [], MATS)
# off the centre, which lies in the planes of the faces' diagonals
INSIDE_CUBE = dict(eye=tuple(c + o for c, o in zip(CENTERS["Cube"], (0.31, -0.17, 0.23))), facing=(0.3, -0.2, -1.0))
SCENES = {
    "cube": (lambda e: upload(e, "Cube"), {}),
    "monkey": (lambda e: upload(e, "Monkey"), {}),
    "monkey_brute_force": (lambda e: upload(e, "Monkey", tree=False), {}),
    "mixed": (MIXED.upload, {}),
    "coincident": (TIES[0].upload, {}),
    "no_models": (NO_MODELS.upload, {}),
    "empty": (EMPTY_SCENE.upload, {}),
    "inside_cube": (lambda e: upload(e, "Cube"), INSIDE_CUBE),
    "inside_sphere": (MIXED.upload, dict(eye=(-1.55, 1.65, -3.3), facing=(0.3, -0.2, -1.0))),
    "under_plane": (MIXED.upload, dict(eye=(0.0, -4.0, 0.0), facing=(0.0, 0.6, -1.0))),
}


def dev():
    return torch.device("cuda", 0)


def dtype(name):
    return torch.float32 if name in ("normal", "position", "depth") else torch.int32


class Out:
    """Sentinel-filled, guarded output tensors for one call."""

    def __init__(self, w, h, names=NAMES):
        self.w, self.h, self.names, self.buf, self.out = w, h, tuple(names), {}, {}
        for k in self.names:
            n = w * h * PER[k]
            self.buf[k] = torch.full((n + 2 * G,), FILL, dtype=dtype(k), device=dev())
            self.out[k] = self.buf[k][G:G + n].view((h, w, 3) if PER[k] == 3 else (h, w))

    def host(self):
        """The outputs as numpy arrays, after checking the guards."""
        res = {}
        for k in self.names:
            b = self.buf[k].cpu().numpy()
            assert (b[:G] == FILL).all() and (b[-G:] == FILL).all(), (k, "guard")
            res[k] = b[G:-G].reshape(self.out[k].shape)
        return res


def guides(eng, cam, names=NAMES, tiles=None, stream=None):  # noqa: F811
    """Engine.camera_guides into fresh guarded buffers (not yet synchronised)."""
    o = Out(cam.width, cam.height, names)
    torch.cuda.synchronize()
    got = eng.camera_guides(cam, tiles=tiles, outputs=names, out=o.out, stream=stream)
    assert all(a is o.out[k] for a, k in zip(got, names))
    return o


def reference(eng, cam):  # noqa: F811
    """The composition: render_guides(cam), and trace_rays on camera_rays(cam) for depth and material."""
    h, w = cam.height, cam.width
    with np.errstate(all="ignore"):
        rays = E.camera_rays(cam)
        n, p, i = eng.render_guides(cam)
    o, d = (torch.from_numpy(a).to(dev()) for a in rays)
    hit, _ = eng.trace_rays(o, d, outputs=("t", "material", "normal", "kind"))
    rc, _ = eng.wait()
    assert rc == 0
    torch.cuda.synchronize()
    return {"normal": n.cpu().numpy(), "position": p.cpu().numpy(), "ident": i.cpu().numpy(),
            "depth": hit["t"].cpu().numpy().reshape(h, w), "material": hit["material"].cpu().numpy().reshape(h, w),
            "raw_normal": hit["normal"].cpu().numpy().reshape(h, w, 3), "kind": hit["kind"].cpu().numpy().reshape(h, w)}


def same(got, want, what=None, where=None):
    """Equal bits (a NaN equals a NaN), on the pixels of the boolean image `where` if given."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    eq = got.view(np.uint32) == want.view(np.uint32)
    if got.dtype == np.float32:
        eq |= np.isnan(got) & np.isnan(want)
    if where is not None:
        eq = eq[where]
    bad = np.argwhere(~eq)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist())


def finish(eng):  # noqa: F811
    rc, done = eng.wait()
    assert rc == 0 and done == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("scene", list(SCENES))
def test_guides_equal_the_composition(eng, scene):  # noqa: F811
    up, view = SCENES[scene]
    up(eng)
    for w, h in SIZES:
        cam = E.camera(w, h, **view)
        want = reference(eng, cam)
        o = guides(eng, cam)
        finish(eng)
        got = o.host()
        for k in NAMES:
            same(got[k], want[k], (scene, w, h, k))
        assert not np.isnan(got["position"]).any() and not np.isnan(got["normal"]).any()
    # the largest frame shows what the scene is there for
    kinds, sky = set(np.unique(want["kind"]).tolist()), got["ident"] == -1
    assert np.array_equal(sky, want["kind"] == E.ATR_RAY_SKY)
    assert (got["normal"][sky].view(np.uint32) == 0).all() and (got["material"][sky] == 0).all()
    assert (got["depth"][sky] == E.MAX_FLOAT).all()
    flipped = (got["normal"] != want["raw_normal"]).any(axis=2)
    if scene == "mixed":
        assert kinds == {E.ATR_RAY_SKY, E.ATR_RAY_TRI, E.ATR_RAY_SPHERE, E.ATR_RAY_PLANE}
        ids = set(np.unique(got["ident"]).tolist())
        assert ids >= {-1, (1 << 28) | 1, (1 << 28) | 2, (1 << 28) | 3, 2 << 28, 3 << 28}, ids
    elif scene == "no_models":
        assert kinds == {E.ATR_RAY_SKY, E.ATR_RAY_SPHERE, E.ATR_RAY_PLANE}
    elif scene == "empty":
        assert sky.all()
    elif scene == "inside_cube":
        assert sky.all()  # tri_hit takes front faces only: from inside a mesh there is nothing to hit
    elif scene == "inside_sphere":
        assert kinds == {E.ATR_RAY_SPHERE} and flipped.all()  # the sphere's normal points away from the eye
    elif scene == "under_plane":
        plane = want["kind"] == E.ATR_RAY_PLANE
        assert plane.any() and flipped[plane].all()  # so does the floor's, seen from below
    else:
        assert E.ATR_RAY_TRI in kinds and sky.any()
    if scene == "cube":
        assert not flipped.any()  # and every hit from outside a front face


def test_tile_lists(eng):  # noqa: F811
    MIXED.upload(eng)
    w, h = 72, 40
    cam = E.camera(w, h)
    want = reference(eng, cam)
    # the reference's overlapping grid: every pixel, once
    tiles = E.make_tiles(w, h, 8)
    assert len(tiles) > 1
    o = guides(eng, cam, tiles=tiles)
    finish(eng)
    got = o.host()
    for k in NAMES:
        same(got[k], want[k], ("grid", k))
    # a tile not aligned to the cells, and two disjoint tiles: pixels outside keep the sentinel
    for rects in ([[5, 3, 20, 17]], [[0, 0, 8, 0], [63, 33, 71, 39]], [[9, 9, 9, 9]]):
        inside = np.zeros((h, w), bool)
        for x0, y0, x1, y1 in rects:
            inside[y0:y1 + 1, x0:x1 + 1] = True
        o = guides(eng, cam, tiles=rects)
        finish(eng)
        got = o.host()
        for k in NAMES:
            same(got[k], want[k], (rects, k), where=inside)
            assert (got[k][~inside] == FILL).all(), (rects, k)


@pytest.mark.parametrize("name", NAMES)
def test_single_outputs(eng, name):  # noqa: F811
    upload(eng, "Monkey")
    cam = E.camera(65, 9)
    want = reference(eng, cam)
    o = guides(eng, cam, names=(name,))
    finish(eng)
    same(o.host()[name], want[name], name)


def test_new_tensors_have_render_guides_shapes(eng):  # noqa: F811
    upload(eng, "Monkey")
    cam = E.camera(13, 7)
    got = eng.camera_guides(cam)
    want = eng.render_guides(cam)
    finish(eng)
    assert len(got) == 3
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype and a.is_contiguous()
        same(a.cpu().numpy(), b.cpu().numpy())
    depth, material = eng.camera_guides(cam, outputs=("depth", "material"))
    assert depth.dtype == torch.float32 and material.dtype == torch.int32 and depth.shape == material.shape == (7, 13)
    finish(eng)
    with pytest.raises(ValueError):
        eng.camera_guides(cam, outputs=("colour",))
    with pytest.raises(ValueError):
        eng.camera_guides(cam, outputs=())
    with pytest.raises(ValueError):
        eng.camera_guides(cam, out={"normal": torch.zeros((7, 13), device=dev())})
    with pytest.raises(ValueError):
        eng.camera_guides(cam, out={"depth": depth})


def test_device_rays_equal_the_host_function(eng):  # noqa: F811
    for (w, h), view in zip(SIZES[2:], ({}, INSIDE_CUBE, dict(h_fov=2.5))):
        cam = E.camera(w, h, **view)
        n = w * h
        for first, count in [(0, None), (w - 3, w + 7), (n - 1, 1), (n, 0)]:
            o, d = eng.camera_rays(cam, first, count)
            finish(eng)
            ho, hd = E.camera_rays_host(cam, first, count)
            same(o.cpu().numpy(), ho, (w, h, first, "origins"))
            same(d.cpu().numpy(), hd, (w, h, first, "directions"))
    with pytest.raises(E.AtrError):
        eng.camera_rays(cam, 1, n)
    assert E.lib().atr_camera_rays(None, C.byref(cam), 0, 0, None, None, None) == -1


def test_two_streams_two_cameras(eng):  # noqa: F811
    upload(eng, "Monkey")
    cams = [E.camera(72, 40), E.camera(72, 40, eye=(0.6, 1.5, 0.3), facing=(-0.3, -0.3, -1.0))]
    wants = [reference(eng, c) for c in cams]
    streams = [torch.cuda.Stream(dev()) for _ in cams]
    outs = [guides(eng, c, stream=s.cuda_stream) for c, s in zip(cams, streams)]
    for s in streams:
        s.synchronize()
    finish(eng)
    for o, want in zip(outs, wants):
        got = o.host()
        for k in NAMES:
            same(got[k], want[k], k)
    assert not np.array_equal(wants[0]["ident"], wants[1]["ident"])


def test_beside_a_denoise_on_another_stream(eng):  # noqa: F811
    upload(eng, "Monkey")
    cam = E.camera(72, 40)
    want = reference(eng, cam)
    n, p, i = eng.render_guides(cam)
    color = torch.rand((40, 72, 3), dtype=torch.float32, device=dev())
    alone = eng.denoise(color, n, p, i)
    finish(eng)
    s1, s2 = torch.cuda.Stream(dev()), torch.cuda.Stream(dev())
    beside = eng.denoise(color, n, p, i, stream=s1.cuda_stream)
    o = guides(eng, cam, stream=s2.cuda_stream)
    s1.synchronize()
    s2.synchronize()
    finish(eng)
    got = o.host()
    for k in NAMES:
        same(got[k], want[k], k)
    same(beside.cpu().numpy(), alone.cpu().numpy(), "denoise")


def test_anti_aliasing_is_not_read(eng):  # noqa: F811
    upload(eng, "Monkey")
    a = guides(eng, E.camera(65, 9))
    b = guides(eng, E.camera(65, 9, spp=4, bounces=0, aa=True))
    finish(eng)
    ga, gb = a.host(), b.host()
    for k in NAMES:
        same(gb[k], ga[k], k)


def test_degenerate_cameras(eng):  # noqa: F811
    """frame_center == eye: the centre pixel's direction is 0 / 0, an invalid ray among valid ones. With
    camera_x = camera_y = 0 as well every pixel is invalid: ray_ok keeps all of them out of the scan (the
    kernel does not enter it for a wave without a valid ray), so the frame is EMPTY, with normal +0, depth
    3.4e38, material 0 and a NaN position."""
    upload(eng, "Monkey")
    w, h = 72, 40
    cam = E.camera(w, h)
    cam.frame_center = E.atr_camera.from_buffer_copy(cam).eye
    want = reference(eng, cam)
    assert want["kind"][20, 36] == E.ATR_RAY_INVALID and (want["kind"] == E.ATR_RAY_INVALID).sum() == 1
    o = guides(eng, cam)
    finish(eng)
    got = o.host()
    for k in NAMES:
        same(got[k], want[k], k)
    assert got["ident"][20, 36] == -1 and np.isnan(got["position"][20, 36]).all()
    cam.camera_x = E.atr_vec3(0.0, 0.0, 0.0)
    cam.camera_y = E.atr_vec3(0.0, 0.0, 0.0)
    want = reference(eng, cam)
    assert (want["kind"] == E.ATR_RAY_INVALID).all()
    o = guides(eng, cam)
    finish(eng)
    got = o.host()
    for k in NAMES:
        same(got[k], want[k], k)
    assert (got["ident"] == -1).all() and (got["normal"].view(np.uint32) == 0).all()
    assert (got["depth"] == E.MAX_FLOAT).all() and (got["material"] == 0).all() and np.isnan(got["position"]).all()


def test_arguments(eng):  # noqa: F811
    upload(eng, "Cube")
    L = E.lib()
    w, h = 13, 7
    cam = E.camera(w, h)
    o = Out(w, h)
    full = E.atr_guides_out(*[o.out[k].data_ptr() for k in NAMES])
    tiles, nt = E.tiles_array([[0, 0, w - 1, h - 1]])
    tp = C.cast(tiles, C.c_void_p)
    torch.cuda.synchronize()
    call = lambda ctx, c, t, n, g: L.atr_camera_guides(ctx, C.byref(c) if c is not None else None, t, n,  # noqa: E731
                                                       C.byref(g) if g is not None else None, None)
    assert call(None, cam, tp, nt, full) == -1
    assert call(eng.h, None, tp, nt, full) == -1
    assert call(eng.h, cam, tp, nt, None) == -1
    assert call(eng.h, cam, tp, nt, E.atr_guides_out()) == -1
    assert call(eng.h, cam, tp, 0, full) == -1 and call(eng.h, cam, tp, -1, full) == -1
    assert call(eng.h, cam, None, 1, full) == -1
    for rect in ([0, 0, w, h - 1], [0, 0, w - 1, h], [-1, 0, 3, 3], [0, -1, 3, 3], [4, 0, 3, 3], [0, 5, 3, 4]):
        t, n = E.tiles_array([[0, 0, 3, 3], rect])
        assert call(eng.h, cam, C.cast(t, C.c_void_p), n, full) == -1, rect
    for field, value in [("width", 0), ("height", 0), ("h_fov", float("nan")), ("aspect_ratio", float("inf")),
                         ("half_pixel_width", float("nan")), ("half_pixel_height", float("inf"))]:
        bad = E.atr_camera.from_buffer_copy(cam)
        setattr(bad, field, value)
        assert call(eng.h, bad, tp, nt, full) == -1, field
    for vec in ("eye", "frame_center", "camera_x", "camera_y", "camera_z"):
        bad = E.atr_camera.from_buffer_copy(cam)
        getattr(bad, vec).y = float("nan")
        assert call(eng.h, bad, tp, nt, full) == -1, vec
        with pytest.raises(E.AtrError):
            eng.camera_guides(bad, out=o.out, outputs=NAMES)
    # nothing was enqueued by any of them
    finish(eng)
    for k, a in o.host().items():
        assert (a == FILL).all(), k
    fresh = E.Engine(0)
    try:
        assert call(fresh.h, cam, tp, nt, full) == -4  # ATR_E_NOSCENE
    finally:
        fresh.close()
    # and the call that is right
    assert call(eng.h, cam, tp, nt, full) == 0
    rc, done = eng.wait()
    assert rc == 0 and done == 0
    assert eng.last_kernel_ms() > 0
    want = reference(eng, cam)
    got = o.host()
    for k in NAMES:
        same(got[k], want[k], k)


def test_accumulator_orbit_equals_render_guides(eng):  # noqa: F811
    """Four frames of the 0.02-rad orbit about the Monkey through TemporalAccumulator.push, with the
    guides it obtains itself and with render_guides' handed in: the same history, in every bit."""
    upload(eng, "Monkey")
    w, h = 72, 40
    mine, theirs = E.TemporalAccumulator(eng), E.TemporalAccumulator(eng)
    for f in range(4):
        eye, facing = orbit(f, 0.02)
        cam = E.camera(w, h, 1, 3, eye=eye, facing=facing)
        color = torch.from_numpy(run(eng, cam)["rgb"]).to(dev())
        a, va = mine.push(cam, color)
        b, vb = theirs.push(cam, color, guides=eng.render_guides(cam))
        finish(eng)
        same(a.cpu().numpy(), b.cpu().numpy(), (f, "color"))
        same(va.cpu().numpy(), vb.cpu().numpy(), (f, "variance"))
        same(mine.prev["moments"].cpu().numpy(), theirs.prev["moments"].cpu().numpy(), (f, "moments"))
        same(mine.prev["length"].cpu().numpy(), theirs.prev["length"].cpu().numpy(), (f, "length"))
        for x, y in zip(mine.prev["guides"], theirs.prev["guides"]):
            same(x.cpu().numpy(), y.cpu().numpy(), (f, "guides"))
    assert int(mine.prev["length"].max()) == 4
