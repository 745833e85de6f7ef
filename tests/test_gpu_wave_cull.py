"""The primary kernels' wave cull (ATR_WAVE_CULL): before the per-ray cluster tests
of a leaf step, HYBRID's primary kernels test each distinct leaf's clusters once per wave against
the hull of the wave's ray directions and visit the survivors only. A culled cluster fails the
loose box test in every lane, so nothing may change: two contexts in one process, one created with
ATR_WAVE_CULL=0, must agree bit for bit on every output, both must equal the oracle, and the COUNT
kernels' work counters must agree wherever the visiting order is the same (lane-private steps).
Needs an MI355X (-m gpu)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from atray_amd.assets import CENTERS, asset_path  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests.goldens import SEED  # noqa: E402
from tests.test_gpu_camera_pads import cam_at, frames_of, run_cameras  # noqa: E402
from tests.test_gpu_cluster import grazing_soup  # noqa: E402
from tests.test_gpu_parity import MODEL, SKY, run  # noqa: E402

pytestmark = pytest.mark.gpu
OUT_KEYS = ("fb", "face", "casts")
# the deal rule of a leaf step (hybrid_a, hybrid_b): the default, every step dealt, no step dealt
DEAL = {"default": (2, 0), "always": (0, -1), "never": (2, 4096)}


def _engine(switch):
    """A context created with ATR_WAVE_CULL = switch (None: unset); the variable is read at creation."""
    old = os.environ.get("ATR_WAVE_CULL")
    try:
        if switch is None:
            os.environ.pop("ATR_WAVE_CULL", None)
        else:
            os.environ["ATR_WAVE_CULL"] = switch
        return E.Engine(0)
    finally:
        if old is None:
            os.environ.pop("ATR_WAVE_CULL", None)
        else:
            os.environ["ATR_WAVE_CULL"] = old


@pytest.fixture(scope="module")
def pair():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    off, on = _engine("0"), _engine(None)
    yield off, on
    off.close()
    on.close()


def same(a, b, what=""):
    for k in OUT_KEYS:
        assert np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))
    assert np.array_equal(a["t"].view(np.uint32), b["t"].view(np.uint32)), (what, "t")
    assert a["traced"] == b["traced"], (what, "traced")


MONKEY_C = CENTERS["Monkey"]
SOUP = {}


def _soup():
    if not SOUP:
        SOUP["txt"] = grazing_soup(12000, 1, (1.0, 4.0))  # det 1-4 x kTol, adjacent and far duplicates
    return SOUP["txt"]


# name -> (asset or None for the soup, leaf size, cluster size, W, H, eye, facing)
APP_EYE, APP_FACING = (0.1, 2.0, 0.0), (-0.1, -0.5, -1.0)
SCENES = {
    "dragon": ("Dragon", 300, 16, 96, 54, APP_EYE, APP_FACING),
    "monkey": ("Monkey", 300, 16, 64, 48, APP_EYE, APP_FACING),
    "monkey_leaf32": ("Monkey", 32, 16, 64, 48, APP_EYE, APP_FACING),  # several leaves per wave and step
    "monkey_61x45": ("Monkey", 300, 16, 61, 45, APP_EYE, APP_FACING),  # partial cells
    # facing exactly -z at the model's centre: the middle cells straddle d.x = 0 and d.y = 0 (72 / 2 and
    # 56 / 2 are no multiples of the cell's 8)
    "monkey_minus_z": ("Monkey", 300, 16, 72, 56, (MONKEY_C[0], MONKEY_C[1], MONKEY_C[2] + 3.0), (0.0, 0.0, -1.0)),
    # the eye inside the model's root box (x -1.46 .. 1.22, y -0.07 .. 1.85, z -3.04 .. -1.42), in its
    # upper front corner, looking at the model's centre
    "monkey_inside": ("Monkey", 300, 16, 64, 48, (0.9, 1.6, -1.5),
                      (MONKEY_C[0] - 0.9, MONKEY_C[1] - 1.6, MONKEY_C[2] + 1.5)),
    "monkey_cluster4": ("Monkey", 300, 4, 64, 48, APP_EYE, APP_FACING),  # up to 75 clusters per leaf
    "soup": (None, 300, 16, 128, 96, APP_EYE, APP_FACING),
}
_built = {}


def scene(name):
    """(engine model tuple, oracle face, oracle t, camera, cluster size) of a scene, built once."""
    if name not in _built:
        asset, leaf, cs, W, H, eye, facing = SCENES[name]
        if asset is None:
            m = E.Mesh.parse_obj(_soup())
            box = m.aabb()
            s = O.Scene(obj_text=_soup(), center=None, max_faces=leaf)
        else:
            m = E.Mesh.load_obj(asset_path(asset))
            box = m.translate_to(m.aabb(), CENTERS[asset])
            s = O.Scene(asset_path(asset), center=CENTERS[asset], max_faces=leaf)
        face, t, _ = s.primary_hits(O.Camera(W, H, eye=eye, facing=facing))
        _built[name] = ((m, E.Octree.build(m, leaf), box, 1), face, t, E.camera(W, H, eye=eye, facing=facing), cs)
    return _built[name]


def upload(pair, name):
    md, face, t, cam, cs = scene(name)
    for e in pair:
        e.set_tuning(cluster_size=cs, hybrid_a=DEAL["default"][0], hybrid_b=DEAL["default"][1])
        e.upload([SKY, MODEL], [md])
    return face, t, cam


@pytest.fixture(autouse=True)
def _restore_tuning(pair):
    yield
    for e in pair:
        e.set_tuning(cluster_size=16, hybrid_a=DEAL["default"][0], hybrid_b=DEAL["default"][1])


@pytest.mark.parametrize("name", list(SCENES))
def test_cull_on_equals_cull_off_and_the_oracle(pair, name):
    off, on = pair
    face_o, t_o, cam = upload(pair, name)
    W, H = cam.width, cam.height
    if name == "monkey_inside":
        box = scene(name)[0][2]
        eye = SCENES[name][5]
        assert all(box[i] < eye[i] < box[3 + i] for i in range(3)), (box, eye)
    assert int((face_o != E.MISS).sum()) > 50  # the model is in view
    whole = [[0, 0, W - 1, H - 1]]
    halves = [[0, 0, W // 2 - 1, H - 1], [W // 2, 0, W - 1, H - 1]]
    for deal, (a, b) in DEAL.items():
        for e in pair:
            e.set_tuning(hybrid_a=a, hybrid_b=b)
        x, y = run(off, cam, variant=E.ATR_KERNEL_HYBRID), run(on, cam, variant=E.ATR_KERNEL_HYBRID)
        same(x, y, (name, deal))
        for o in (x, y):  # and both are the reference's hits
            assert np.array_equal(o["face"], face_o), (name, deal, int((o["face"] != face_o).sum()))
            assert np.array_equal(o["t"].view(np.uint32), t_o.view(np.uint32)), (name, deal)
        # FLAT sends primary-only frames to HYBRID's 6-wave primary kernel
        same(x, run(on, cam, variant=E.ATR_KERNEL_FLAT), (name, deal, "FLAT"))
        same(run(off, cam, variant=E.ATR_KERNEL_FLAT), x, (name, deal, "FLAT off"))
        for variant in (E.ATR_KERNEL_HYBRID, E.ATR_KERNEL_FLAT):
            same(run(off, cam, tiles=halves, layout=E.ATR_LAYOUT_PACKED, variant=variant),
                 run(on, cam, tiles=halves, layout=E.ATR_LAYOUT_PACKED, variant=variant), (name, deal, variant, "PACKED"))
        ca = off.counters(cam, whole, SEED, E.ATR_KERNEL_HYBRID)
        cb = on.counters(cam, whole, SEED, E.ATR_KERNEL_HYBRID)
        print(name, deal, "off", ca, "on", cb)
        assert ca["cluster_boxes"] >= ca["n_leaf"] > 0 and ca["screened"] > 0  # the cluster tests did run
        for k in ("n_rays", "n_box", "n_leaf"):
            assert ca[k] == cb[k], (name, deal, k, ca, cb)
        if deal == "never":  # lane-private steps: each lane's sequence of bounds is what it was
            for k in ("cluster_boxes", "screened", "n_tri"):
                assert ca[k] == cb[k], (name, deal, k, ca, cb)


@pytest.mark.parametrize("layout", [E.ATR_LAYOUT_IMAGE, E.ATR_LAYOUT_PACKED])
def test_three_cameras_in_one_launch(pair, layout):
    off, on = pair
    upload(pair, "dragon")
    W, H = 96, 54
    tiles = [[0, 0, W - 1, H - 1]] if layout == E.ATR_LAYOUT_IMAGE else [[0, 0, 39, H - 1], [40, 0, W - 1, H - 1]]
    cams = [cam_at(W, H, k) for k in (0, 3, 5)]
    got = []
    for e in (off, on):
        n, bufs = run_cameras(e, cams, tiles, layout)
        rc, _ = e.wait()
        assert rc == 0
        torch.cuda.synchronize()
        got.append(frames_of(n, len(cams), bufs))
    for f in range(len(cams)):
        same(got[0][f], got[1][f], f)
    assert not np.array_equal(got[1][0]["face"], got[1][1]["face"])  # the cameras do differ


def test_culled_counter(pair):
    off, on = pair
    _, _, cam = upload(pair, "dragon")
    whole = [[0, 0, cam.width - 1, cam.height - 1]]
    for variant in (E.ATR_KERNEL_HYBRID, E.ATR_KERNEL_FLAT):
        c_on, c_off = on.cull_counters(cam, whole, SEED, variant), off.cull_counters(cam, whole, SEED, variant)
        print("dragon", variant, "on", c_on, "off", c_off)
        assert c_on["culled"] > 0
        assert c_off["culled"] == 0
    # a frame of axis-straddling cells only: the column of cells around d.x = 0, the row around d.y = 0
    _, _, cam = upload(pair, "monkey_minus_z")
    W, H = cam.width, cam.height
    assert (W // 2) % 8 and (H // 2) % 8
    print("minus z, whole frame", on.cull_counters(cam, [[0, 0, W - 1, H - 1]], SEED, E.ATR_KERNEL_HYBRID))
    for tiles in ([[W // 2 // 8 * 8, 0, W // 2 // 8 * 8 + 7, H - 1]], [[0, H // 2 // 8 * 8, W - 1, H // 2 // 8 * 8 + 7]]):
        c = on.counters(cam, tiles, SEED, E.ATR_KERNEL_HYBRID)
        assert c["cluster_boxes"] > 0  # these cells do scan leaves
        assert on.cull_counters(cam, tiles, SEED, E.ATR_KERNEL_HYBRID)["culled"] == 0, tiles
