"""The per-camera table of box growths (ATR_CAMERA_PADS): HYBRID's primary kernels
read each cluster's {loose, tight} growth per (camera, cluster) from a table instead of computing
it per (ray, cluster). The table holds the values the inline path computes, so nothing may change:
two contexts in one process, one created with ATR_CAMERA_PADS=0 (inline) and one with the default
(table), must agree bit for bit on every output and on the COUNT kernels' work counters -- equal
cluster box, screen and triangle counts show that the table's bits are the inline values, not
merely that the result survived. Needs an MI355X (-m gpu)."""
import math
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from atray_amd.assets import CENTERS, asset_path  # noqa: E402
from tests.goldens import SEED  # noqa: E402
from tests.test_gpu_parity import MODEL, SKY, run  # noqa: E402

pytestmark = pytest.mark.gpu
OUT_KEYS = ("fb", "face", "casts")


def _engine(switch):
    """A context created with ATR_CAMERA_PADS = switch (None: unset); the variable is read at creation."""
    old = os.environ.get("ATR_CAMERA_PADS")
    try:
        if switch is None:
            os.environ.pop("ATR_CAMERA_PADS", None)
        else:
            os.environ["ATR_CAMERA_PADS"] = switch
        return E.Engine(0)
    finally:
        if old is None:
            os.environ.pop("ATR_CAMERA_PADS", None)
        else:
            os.environ["ATR_CAMERA_PADS"] = old


@pytest.fixture(scope="module")
def pair():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    off, on = _engine("0"), _engine(None)
    yield off, on
    off.close()
    on.close()


_models = {}


def model(asset, center=None, leaf=300):
    key = (asset, center, leaf)
    if key not in _models:
        m = E.Mesh.load_obj(asset_path(asset))
        box = m.translate_to(m.aabb(), center or CENTERS[asset])
        _models[key] = (m, E.Octree.build(m, leaf), box, 1)
    return _models[key]


def same(a, b, what=""):
    for k in OUT_KEYS:
        assert np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))
    assert np.array_equal(a["t"].view(np.uint32), b["t"].view(np.uint32)), (what, "t")
    assert a["traced"] == b["traced"], (what, "traced")


def orbit(k, n=8, r=0.5):
    """Eye k of a small orbit around the app eye (the benchmark's kind of camera path)."""
    a = 2.0 * math.pi * k / n
    return (0.1 + r * math.cos(a), 2.0, r * math.sin(a))


def cam_at(W, H, k, spp=1, bounces=1):
    return E.camera(W, H, spp, bounces, eye=orbit(k))


@pytest.mark.parametrize("asset,W,H", [("Dragon", 96, 54), ("Monkey", 64, 48)])
def test_table_on_equals_table_off(pair, asset, W, H):
    off, on = pair
    md = model(asset)
    assert md[1].stats()["leaves"] - md[1].stats()["empty_leaves"] > 4  # a tree with several leaves
    for e in pair:
        e.upload([SKY, MODEL], [md])
    cam = E.camera(W, H)
    a, b = run(off, cam, variant=E.ATR_KERNEL_HYBRID), run(on, cam, variant=E.ATR_KERNEL_HYBRID)
    assert int((a["face"] != E.MISS).sum()) > 50  # the model is in view
    same(a, b, asset)
    # FLAT sends primary-only frames to HYBRID's 6-wave primary kernel: that build reads the table too
    same(a, run(on, cam, variant=E.ATR_KERNEL_FLAT), (asset, "FLAT"))
    tiles = [[0, 0, W - 1, H - 1]]
    ca = off.counters(cam, tiles, SEED, E.ATR_KERNEL_HYBRID)
    cb = on.counters(cam, tiles, SEED, E.ATR_KERNEL_HYBRID)
    assert ca["cluster_boxes"] > ca["n_leaf"] > 0 and ca["screened"] > 0  # the cluster tests did run
    assert ca == cb, (ca, cb)


def run_cameras(eng, cams, tiles, layout, stream=None):
    W, H = cams[0].width, cams[0].height
    n = W * H if layout == E.ATR_LAYOUT_IMAGE else E.packed_size(tiles)
    nf = len(cams)
    dev = torch.device("cuda", 0)
    fb = torch.full((nf * n,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
    face = torch.full((nf * n,), -7, dtype=torch.int32, device=dev)
    t = torch.zeros(nf * n, dtype=torch.float32, device=dev)
    casts = torch.full((nf * n,), -1, dtype=torch.int32, device=dev)
    fr = E.atr_frame(layout, fb.data_ptr(), face.data_ptr(), t.data_ptr(), None, casts.data_ptr(), None)
    eng.render_start_cameras(cams, tiles, fr, n, SEED, stream=stream or torch.cuda.current_stream().cuda_stream,
                             variant=E.ATR_KERNEL_HYBRID)
    return n, (fb, face, t, casts)


def frames_of(n, nf, bufs):
    fb, face, t, casts = (x.cpu().numpy() for x in bufs)
    return [{"fb": fb[f * n:(f + 1) * n].view(np.uint32), "face": face[f * n:(f + 1) * n].view(np.uint32),
             "t": t[f * n:(f + 1) * n], "casts": casts[f * n:(f + 1) * n].view(np.uint32), "traced": 0}
            for f in range(nf)]


@pytest.mark.parametrize("layout", [E.ATR_LAYOUT_IMAGE, E.ATR_LAYOUT_PACKED])
def test_each_frame_reads_its_own_row(pair, layout):
    off, on = pair
    W, H = 96, 54
    for e in pair:
        e.upload([SKY, MODEL], [model("Dragon")])
    tiles = [[0, 0, W - 1, H - 1]] if layout == E.ATR_LAYOUT_IMAGE else [[0, 0, 39, H - 1], [40, 0, W - 1, H - 1]]
    cams = [cam_at(W, H, k) for k in (0, 3, 5)]
    n, bufs = run_cameras(on, cams, tiles, layout)
    rc, _ = on.wait()
    assert rc == 0
    torch.cuda.synchronize()
    got = frames_of(n, len(cams), bufs)
    for f, cam in enumerate(cams):
        for eng in (off, on):  # its own one-camera render, inline and from a one-row table
            want = run(eng, cam, tiles=tiles, layout=layout, variant=E.ATR_KERNEL_HYBRID)
            want = {k: (v.reshape(-1) if isinstance(v, np.ndarray) and k != "rgb" else v) for k, v in want.items()}
            want["traced"] = 0
            same(got[f], want, (f, eng is on))
    assert not np.array_equal(got[0]["face"], got[1]["face"])  # the cameras do differ


def test_models_index_the_table_from_their_own_base(pair):
    off, on = pair
    W, H = 96, 72
    two = [model("Monkey"), model("Deer")]
    two.sort(key=lambda m: m[0].info()[2])  # fewer faces (so fewer clusters) first
    assert two[0][0].info()[2] < two[1][0].info()[2]
    for e in pair:
        e.upload([SKY, MODEL], two)
    cam = E.camera(W, H)
    a = run(off, cam, variant=E.ATR_KERNEL_HYBRID)
    b = run(on, cam, variant=E.ATR_KERNEL_HYBRID)
    lane = run(on, cam, variant=E.ATR_KERNEL_LANE)
    same(a, b, "on/off")
    same(b, lane, "table/LANE")
    tiles = [[0, 0, W - 1, H - 1]]
    assert off.counters(cam, tiles, SEED, E.ATR_KERNEL_HYBRID) == on.counters(cam, tiles, SEED, E.ATR_KERNEL_HYBRID)
    # each model alone is in view, so the rays scan both models' clusters
    hits = []
    for md in two:
        on.upload([SKY, MODEL], [md])
        hits.append(int((run(on, cam, variant=E.ATR_KERNEL_HYBRID)["face"] != E.MISS).sum()))
    assert min(hits) > 20, hits


def test_slots_two_launches_in_flight(pair):
    """Two multi-camera launches with different cameras on two streams, no wait between them."""
    off, on = pair
    W, H = 96, 54
    for e in pair:
        e.upload([SKY, MODEL], [model("Dragon")])
    tiles = [[0, 0, W - 1, H - 1]]
    sets = [[cam_at(W, H, k) for k in (0, 1)], [cam_at(W, H, k) for k in (4, 6)]]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    launched = [run_cameras(on, cs, tiles, E.ATR_LAYOUT_IMAGE, stream=s.cuda_stream) for cs, s in zip(sets, streams)]
    for s in streams:
        s.synchronize()
    torch.cuda.synchronize()
    for cs, (n, bufs) in zip(sets, launched):
        got = frames_of(n, len(cs), bufs)
        for f, cam in enumerate(cs):
            want = run(off, cam, variant=E.ATR_KERNEL_HYBRID)
            want = {k: (v.reshape(-1) if isinstance(v, np.ndarray) and k != "rgb" else v) for k, v in want.items()}
            want["traced"] = 0
            same(got[f], want, f)


def test_slots_hit_miss_and_rebuild(pair):
    """Back-to-back single-frame launches alternating between two eyes: with more distinct eyes in
    between than there are slots, a launch meets a cached table, a missing one and a rebuilt one."""
    off, on = pair
    W, H = 96, 54
    for e in pair:
        e.upload([SKY, MODEL], [model("Dragon")])
    want = {k: run(off, cam_at(W, H, k), variant=E.ATR_KERNEL_HYBRID) for k in range(7)}
    for k in (0, 3, 0, 3):  # miss, miss, hit, hit
        same(run(on, cam_at(W, H, k), variant=E.ATR_KERNEL_HYBRID), want[k], k)
    for k in (1, 2, 4, 5, 6, 0, 3, 0):  # every slot rebuilt, then the first two eyes again
        same(run(on, cam_at(W, H, k), variant=E.ATR_KERNEL_HYBRID), want[k], k)


def test_slots_forget_the_scene_on_upload(pair):
    off, on = pair
    W, H = 64, 48
    cam = E.camera(W, H)
    on.upload([SKY, MODEL], [model("Dragon")])
    first = run(on, cam, variant=E.ATR_KERNEL_HYBRID)
    on.upload([SKY, MODEL], [model("Monkey")])  # same eye, another scene: the cached table is stale
    again = run(on, cam, variant=E.ATR_KERNEL_HYBRID)
    fresh = _engine(None)
    try:
        fresh.upload([SKY, MODEL], [model("Monkey")])
        same(again, run(fresh, cam, variant=E.ATR_KERNEL_HYBRID), "re-upload")
    finally:
        fresh.close()
    assert not np.array_equal(first["face"], again["face"])


def test_other_flavours_untouched(pair):
    """Bounce rays and the path engine never read the table: a 2-spp, 3-bounce render is the same."""
    off, on = pair
    W, H = 48, 27
    for e in pair:
        e.upload([SKY, MODEL], [model("Dragon")])
    cam = E.camera(W, H, 2, 3)
    for variant in (E.ATR_KERNEL_AUTO, E.ATR_KERNEL_HYBRID, E.ATR_KERNEL_FLAT):
        a, b = run(off, cam, variant=variant), run(on, cam, variant=variant)
        same(a, b, variant)
        assert np.array_equal(a["rgb"].view(np.uint32), b["rgb"].view(np.uint32)), variant
