"""The primary kernels' sky path (ATR_SKY_PATH): a wavefront none of whose rays passes
the first box test of any model writes the sky's outputs from the kernel arguments and reads nothing
of the scene. The test it skips is the one it just ran, so nothing may change: a default context, a
context created with ATR_SKY_PATH=0 and the oracle must agree bit for bit on the framebuffer, ray_casts,
hit_face, hit_t, rgb and the traced-ray count, through HYBRID at 6 / 7 / 8 waves, AUTO and FLAT's primary
route, in both layouts, with one camera and with three per launch. The instrumented render never takes
the path (its n_box is the reference's) and counts the waves that would (sky_cells): all of them where
a float64 projection of the models' boxes leaves a cell two pixels clear, never more than the cells
without an oracle hit, none in a switched-off context, with a sphere, a plane or five models.
Needs an MI355X (-m gpu)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from atray_amd.assets import CENTERS  # noqa: E402
from tests import test_gpu_scenes as TS  # noqa: E402
from tests.goldens import SEED  # noqa: E402
from tests.test_gpu_leaf_box import _engine  # noqa: E402
from tests.test_gpu_parity import run  # noqa: E402

pytestmark = pytest.mark.gpu
APP_EYE, APP_FACING = (0.1, 2.0, 0.0), (-0.1, -0.5, -1.0)
MONKEY_C = CENTERS["Monkey"]
KEYS = ("fb", "face", "casts", "t", "rgb")
# parts this file adds to test_gpu_scenes' table: the Cube as a one-node tree, the Monkey by brute force
TS.PARTS.setdefault("cube_tiny", ("Cube", CENTERS["Cube"], 6, True))
TS.PARTS.setdefault("monkey_bf", ("Monkey", MONKEY_C, 300, False))
TS.PARTS.setdefault("monkey_moved", ("Monkey", (MONKEY_C[0] + 1.5, MONKEY_C[1] + 0.4, MONKEY_C[2]), 64, True))


@pytest.fixture(scope="module")
def pair():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    off, on = _engine(ATR_SKY_PATH="0"), _engine(ATR_SKY_PATH=None)
    yield off, on
    off.close()
    on.close()


@pytest.fixture(autouse=True)
def _restore_tuning(pair):
    base = pair[1].tuning()
    yield
    for e in pair:
        e.set_tuning(**base)


def ubits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b, what):
    """Two engine renders, every output bit for bit."""
    for k in KEYS:
        assert np.array_equal(ubits(a[k]), ubits(b[k])), (what, k, int((ubits(a[k]) != ubits(b[k])).sum()))
    assert a["traced"] == b["traced"], (what, "traced", a["traced"], b["traced"])


def same_oracle(o, r, what, pix=None):
    """An engine render against the oracle's frame (pix: the slots' pixels of a PACKED render), rgb too
    bit for bit: a primary frame's colour is one emission divided by one sample."""
    TS.same(o, r, what, pix)
    want = r["rgb"] if pix is None else r["rgb"].reshape(-1, 3)[pix]
    assert np.array_equal(ubits(np.asarray(o["rgb"], np.float32)), ubits(np.asarray(want, np.float32))), (what, "rgb")


class Case:
    def __init__(self, sc, W, H, eye=APP_EYE, facing=APP_FACING, sky="some"):
        self.sc, self.W, self.H, self.eye, self.facing, self.sky = sc, W, H, tuple(eye), tuple(facing), sky

    def cam(self, eye=None):
        return E.camera(self.W, self.H, eye=eye or self.eye, facing=self.facing)

    def ref(self, eye=None):
        return TS.ref(self.sc, self.W, self.H, eye=eye or self.eye, facing=self.facing)


MONKEY, TWO = TS.Sc(["monkey"], [1]), ["monkey", "cube"]
CASES = {
    # sky: "all" = every cell takes the path, "none" = no cell, "some" = cells clear of the boxes, cells
    # inside them and cells on their silhouette, "off" = the scene switches the path off
    # the model well to the left, the camera looking along +z: no ray's line meets the root box
    "all_cells_miss": Case(MONKEY, 64, 48, eye=(6.0, 2.0, 0.0), facing=(0.0, 0.0, 1.0), sky="all"),
    # the app's eye turned away from the model: nothing is hit, yet box_check passes the box behind the
    # eye for the rays whose line runs back through it (aabb.h asks no t > 0)
    "box_behind_the_eye": Case(MONKEY, 64, 48, facing=(0.0, 0.0, 1.0), sky="behind"),
    "eye_in_root_box": Case(MONKEY, 64, 48, eye=(0.9, 1.6, -1.5),
                            facing=(MONKEY_C[0] - 0.9, MONKEY_C[1] - 1.6, MONKEY_C[2] + 1.5), sky="none"),
    "silhouette_cells": Case(MONKEY, 64, 48),
    "partial_cells_61x45": Case(MONKEY, 61, 45),
    # facing -z at the model's centre: column 36 has d.x = 0, row 28 d.y = 0: inf and NaN slabs in box_check
    "minus_z_zero_components": Case(MONKEY, 72, 56, eye=(MONKEY_C[0], MONKEY_C[1], MONKEY_C[2] + 3.0), facing=(0.0, 0.0, -1.0)),
    "cube_root_leaf": Case(TS.Sc(["cube"], [1]), 64, 48),
    "cube_one_node_tree": Case(TS.Sc(["cube_tiny"], [1]), 64, 48),
    "monkey_brute_force_160x120": Case(TS.Sc(["monkey_bf"], [1]), 160, 120),
    "two_trees": Case(TS.Sc(TWO, [2, 1]), TS.W, TS.H),
    "tree_and_brute_force": Case(TS.Sc(["monkey", "cube_bf"], [2, 4]), TS.W, TS.H),
    "two_trees_sphere": Case(TS.Sc(TWO, [2, 1], TS.MATS, TS.SPHERES), TS.W, TS.H, sky="off"),
    "two_trees_sphere_plane": Case(TS.Sc(TWO, [2, 1], TS.MATS, TS.SPHERES, TS.PLANES), TS.W, TS.H, sky="off"),
    "five_models": Case(TS.Sc(["cube%d" % k for k in range(5)], [1 + k % 4 for k in range(5)]), TS.W, TS.H, sky="off"),
}


# ---- the float64 projection ------------------------------------------------------------------------------

def v3(v):
    return np.array([v.x, v.y, v.z], np.float64)


def box_mask(cam, box, brute):
    """Per pixel (row y, column x as the outputs index them): does the pixel's ray, in float64, meet
    the box -- its whole line for a tree model (box_check asks no t > 0), its forward half for a
    brute-force one (box_entry)."""
    W, H = cam.width, cam.height
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    fx = ((-1.0 + 2.0 * (x / W)) * float(cam.h_fov)) * float(cam.aspect_ratio)
    fy = -1.0 + 2.0 * (y / H)
    eye = v3(cam.eye)
    d = v3(cam.frame_center) + fx[..., None] * v3(cam.camera_x) + fy[..., None] * v3(cam.camera_y) - eye
    lo, hi = np.asarray(box[:3], np.float64), np.asarray(box[3:], np.float64)
    with np.errstate(all="ignore"):
        t1, t2 = (lo - eye) / d, (hi - eye) / d
        par = d == 0.0  # parallel to a slab: inside it or not, whatever t
        inside = (eye >= lo) & (eye <= hi)
        near = np.where(par, np.where(inside, -np.inf, np.inf), np.minimum(t1, t2)).max(axis=-1)
        far = np.where(par, np.where(inside, np.inf, -np.inf), np.maximum(t1, t2)).min(axis=-1)
    return (near <= far) & ((far > 0) if brute else True)


def dilate(m, r):
    out = np.zeros_like(m)
    H, W = m.shape
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            out[max(0, dy):H + min(0, dy), max(0, dx):W + min(0, dx)] |= m[max(0, -dy):H + min(0, -dy), max(0, -dx):W + min(0, -dx)]
    return out


def cells_without(m):
    """8x8 cells of a whole-frame tile (partial ones at the right and top edges) with no pixel of m set."""
    H, W = m.shape
    return sum(1 for y0 in range(0, H, 8) for x0 in range(0, W, 8) if not m[y0:y0 + 8, x0:x0 + 8].any())


def projection(rec, cam):
    """(cells at least 2 px clear of every recorded box, a cell has both kinds of pixel, the boxes' mask)."""
    m = np.zeros((cam.height, cam.width), bool)
    for i in range(rec["n"]):
        m |= box_mask(cam, rec["boxes"][i], (rec["brute"] >> i) & 1)
    H, W = m.shape
    straddle = any(0 < int(m[y0:y0 + 8, x0:x0 + 8].sum()) < m[y0:y0 + 8, x0:x0 + 8].size
                   for y0 in range(0, H, 8) for x0 in range(0, W, 8))
    return cells_without(dilate(m, 2)), straddle, m


# ---- the launches ------------------------------------------------------------------------------------------

def run_cameras(eng, cams, tiles, layout, variant):
    """len(cams) frames in one launch, every output; traced = the launch's count."""
    W, H = cams[0].width, cams[0].height
    n = W * H if layout == E.ATR_LAYOUT_IMAGE else E.packed_size(tiles)
    nf = len(cams)
    dev = torch.device("cuda", 0)
    fb = torch.full((nf * n,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    face = torch.full((nf * n,), -7, dtype=torch.int32, device=dev)
    t = torch.zeros(nf * n, dtype=torch.float32, device=dev)
    rgb = torch.full((3 * nf * n,), -1.0, dtype=torch.float32, device=dev)
    casts = torch.full((nf * n,), -1, dtype=torch.int32, device=dev)
    traced = torch.zeros(1, dtype=torch.int64, device=dev)
    fr = E.atr_frame(layout, fb.data_ptr(), face.data_ptr(), t.data_ptr(), rgb.data_ptr(), casts.data_ptr(), traced.data_ptr())
    eng.render_start_cameras(cams, tiles, fr, n, SEED, stream=torch.cuda.current_stream().cuda_stream, variant=variant)
    rc, _ = eng.wait()
    assert rc == 0
    torch.cuda.synchronize()
    fb, face, t, casts = (a.cpu().numpy() for a in (fb, face, t, casts))
    rgb = rgb.cpu().numpy().reshape(-1, 3)
    return [{"fb": fb[f * n:(f + 1) * n].view(np.uint32), "face": face[f * n:(f + 1) * n].view(np.uint32),
             "t": t[f * n:(f + 1) * n], "casts": casts[f * n:(f + 1) * n].view(np.uint32), "rgb": rgb[f * n:(f + 1) * n],
             "traced": int(traced.item())} for f in range(nf)]


def check_case(pair, c, name):
    off, on = pair
    for e in pair:
        c.sc.upload(e)
    r = c.ref()
    W, H = c.W, c.H
    cam = c.cam()
    whole = [[0, 0, W - 1, H - 1]]
    halves = [[0, 0, W // 2 - 1, H - 1], [W // 2, 0, W - 1, H - 1]]
    pix = E.packed_pixel_map(halves, W, H)
    settings = [(E.ATR_KERNEL_HYBRID, occ) for occ in (6, 7, 8)] + [(E.ATR_KERNEL_AUTO, 0), (E.ATR_KERNEL_FLAT, 0)]
    for variant, occ in settings:
        for e in pair:
            e.set_tuning(primary_occ=occ)
        x, y = run(off, cam, variant=variant), run(on, cam, variant=variant)
        same(x, y, (name, variant, occ))
        same_oracle(y, r, (name, variant, occ, "oracle"))
        px, py = (run(e, cam, tiles=halves, layout=E.ATR_LAYOUT_PACKED, variant=variant) for e in pair)
        same(px, py, (name, variant, occ, "PACKED"))
        same_oracle(py, r, (name, variant, occ, "PACKED", "oracle"), pix)
        # three cameras in one launch (the kernel's per-frame cameras), both layouts: each frame its own render's
        eyes = [c.eye, tuple(float(np.float32(v) + np.float32(0.03) * (abs(np.float32(v)) + np.float32(1.0))) for v in c.eye),
                tuple(float(np.float32(v) - np.float32(0.02) * (abs(np.float32(v)) + np.float32(1.0))) for v in c.eye)]
        cams = [c.cam(eye=ey) for ey in eyes]
        for layout, tiles in ((E.ATR_LAYOUT_IMAGE, whole), (E.ATR_LAYOUT_PACKED, halves)):
            fa, fb_ = run_cameras(off, cams, tiles, layout, variant), run_cameras(on, cams, tiles, layout, variant)
            for f in range(3):
                same(fa[f], fb_[f], (name, variant, occ, layout, "frame", f))
            first = dict(fb_[0], traced=None)  # frame 0 is the case's own camera
            if layout == E.ATR_LAYOUT_IMAGE:
                first = {k: v if v is None else v.reshape((H, W, 3) if k == "rgb" else (H, W)) for k, v in first.items()}
            same_oracle(first, r, (name, variant, occ, layout, "frame 0 of three"), None if layout == E.ATR_LAYOUT_IMAGE else pix)
    for e in pair:
        e.set_tuning(primary_occ=0)
    # the instrumented render walks the scene for every wave: its counters are the switched-off context's,
    # and every ray counts one box test per model at the least
    nmodels = len(c.sc.names)
    for variant in (E.ATR_KERNEL_HYBRID, E.ATR_KERNEL_FLAT):
        ca, cb = off.counters(cam, whole, SEED, variant), on.counters(cam, whole, SEED, variant)
        assert ca == cb, (name, variant, ca, cb)
        assert cb["n_rays"] == W * H and cb["n_box"] >= W * H * nmodels, (name, variant, cb)
        assert off.sky_cells(cam, whole, SEED, variant) == 0, name
        sky = on.sky_cells(cam, whole, SEED, variant)
        ncells = ((W + 7) // 8) * ((H + 7) // 8)
        no_hit = cells_without(r["face"] != E.MISS)
        rec = on.sky_record()
        clear, straddle, mask = projection(rec, cam)
        print(name, variant, "cells", ncells, "sky", sky, "clear by 2 px", clear, "without a hit", no_hit, "n_box", cb["n_box"])
        if c.sky == "off":
            assert rec["on"] == 0 and sky == 0, (name, sky, rec)
            continue
        assert rec["on"] == 1 and rec["n"] == nmodels, (name, rec)
        assert not ((r["face"] != E.MISS) & ~dilate(mask, 1)).any(), name  # the projection holds every hit pixel
        assert clear <= sky <= no_hit, (name, clear, sky, no_hit)
        if c.sky == "all":
            assert sky == ncells == no_hit, (name, sky, ncells)
        elif c.sky == "none":
            assert sky == 0 and mask.all(), (name, sky)
        else:
            assert 0 < clear and sky < ncells and straddle, (name, clear, sky, ncells, straddle)
            assert (no_hit == ncells) == (c.sky == "behind"), (name, no_hit)
    assert on.sky_cells(cam, whole, SEED, E.ATR_KERNEL_LANE) == 0, name  # a kernel without the path


@pytest.mark.parametrize("name", list(CASES))
def test_frames_counters_and_sky_cells(pair, name):
    c = CASES[name]
    if c.sky not in ("all", "behind"):
        assert int((c.ref()["face"] != E.MISS).sum()) > 20, name  # a model is in view
    check_case(pair, c, name)


def test_eye_in_root_box_is_inside_the_recorded_box(pair):
    c = CASES["eye_in_root_box"]
    c.sc.upload(pair[1])
    b = pair[1].sky_record()["boxes"][0]
    e = np.asarray(c.eye, np.float32)
    assert (b[:3] < e).all() and (e < b[3:]).all()


def test_a_reupload_refreshes_the_record(pair):
    """The same mesh moved: the second upload's launches test the new root box, not the first one's."""
    off, on = pair
    here, there = TS.Sc(["monkey"], [1]), TS.Sc(["monkey_moved"], [1])
    W, H = 64, 48
    cam, whole = E.camera(W, H), [[0, 0, W - 1, H - 1]]
    recs, frames, skies = [], [], []
    for sc in (here, there, here):
        for e in pair:
            sc.upload(e)
        recs.append(on.sky_record()["boxes"][0].copy())
        x, y = run(off, cam, variant=E.ATR_KERNEL_HYBRID), run(on, cam, variant=E.ATR_KERNEL_HYBRID)
        same(x, y, sc.names)
        same_oracle(y, TS.ref(sc, W, H), (sc.names, "oracle"))
        frames.append(y)
        skies.append(on.sky_cells(cam, whole, SEED, E.ATR_KERNEL_HYBRID))
    assert not np.array_equal(recs[0], recs[1]) and np.array_equal(recs[0], recs[2])
    assert np.allclose(recs[1][[0, 3]] - recs[0][[0, 3]], 1.5, atol=1e-3)  # the box moved with the model
    assert not np.array_equal(frames[0]["face"], frames[1]["face"])
    same(frames[0], frames[2], "back again")
    assert skies[0] == skies[2] > 0 and skies[1] > 0


def test_the_record_of_an_uploaded_scene_is_the_host_s(pair):
    """The context's record equals atr_sky_record_host's of the same arguments, but for the switch."""
    off, on = pair
    for sc in (CASES["tree_and_brute_force"].sc, CASES["five_models"].sc, CASES["two_trees_sphere"].sc):
        for e in pair:
            sc.upload(e)
        want = E.sky_record(sc.materials, sc.models(), len(sc.spheres), len(sc.planes))
        for e, on_ in ((on, want["on"]), (off, 0)):
            got = e.sky_record()
            assert got["on"] == on_, sc.names
            for k in ("n", "brute", "face"):
                assert got[k] == want[k], (sc.names, k)
            for k in ("t", "emission", "boxes"):
                assert np.array_equal(ubits(got[k]), ubits(want[k])), (sc.names, k)
