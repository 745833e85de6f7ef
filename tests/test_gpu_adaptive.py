"""Adaptive sampling (atr_render_start_adaptive): sample passes that skip the pixels that have
stopped. After any number of passes every pixel's outputs equal the oracle's one-shot render at
that pixel's own sample count, bit for bit, and the sample-count map and the info counts equal a
host model computed from oracle renders alone (tests/adaptive_model.py). Needs an MI355X (-m gpu)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from atray_amd.assets import CENTERS, asset_path  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import adaptive_model as M  # noqa: E402
from tests.goldens import GOLD, SEED, render  # noqa: E402

pytestmark = pytest.mark.gpu
DRAGON, MONKEY_AA = "dragon_120x68_s64_b5", "monkey_72x40_s100_b3_aa"
PASSES, TOL = [4, 4, 8, 16, 32], 0.01
AA_PASSES = [3, 5, 12, 30]
FLAG = np.uint32(E.ATR_SAMPLES_CONVERGED)
COUNT_FILL = 0x7F7F7F7F  # no pass's first_sample (at most 2^24)


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    e = E.Engine(0)
    yield e
    e.close()


_scenes = {}


def upload(eng, asset, tree=True):
    key = (asset, tree)
    if key not in _scenes:
        m = E.Mesh.load_obj(asset_path(asset))
        box = m.translate_to(m.aabb(), CENTERS[asset])
        _scenes[key] = (m, E.Octree.build(m, 300) if tree else None, box)
    m, t, box = _scenes[key]
    eng.upload([O.SKY, O.MODEL_MAT], [(m, t, box, 1)])


_oracle = {}


def scene_of(name):
    g = GOLD["render"][name]
    if (name, "scene") not in _oracle:
        _oracle[name, "scene"] = O.Scene(asset_path(g["asset"]), center=CENTERS[g["asset"]])
    return _oracle[name, "scene"]


def oracle(name, total):
    """The oracle's render of golden config `name` at `total` samples: (rgb, fb, casts, n_rays),
    computed once per module (the committed golden at the config's own sample count)."""
    g = GOLD["render"][name]
    if (name, total) not in _oracle:
        if total == g["spp"]:
            rgb, fb, casts = render(name)
            _oracle[name, total] = (rgb, fb, casts, g["counters"]["n_rays"])
        else:
            rgb, fb, casts, ctr = scene_of(name).render(
                O.Camera(g["W"], g["H"], spp=total, bounces=g["bounces"], aa=g["aa"]), SEED)
            _oracle[name, total] = (rgb, fb, casts, ctr["n_rays"])
    return _oracle[name, total]


def model(name, passes, tol, pixels=None, waves=1):
    """The host model's (count map, info) per pass for golden config `name`."""
    key = (name, "model", tuple(passes), tol, None if pixels is None else np.asarray(pixels).tobytes(), waves)
    if key not in _oracle:
        g = GOLD["render"][name]
        means = {int(t): oracle(name, int(t))[0] for t in np.cumsum(passes)}
        _oracle[key] = M.run(means, passes, tol, M.block_ids(g["W"], g["H"], pixels, waves))
    return _oracle[key]


class Frame:
    """A frame's output buffers with its running-sum and sample-count buffers, filled with values no
    render leaves (the sums with NaN: a first pass that read them would poison every pixel)."""

    def __init__(self, n, layout=E.ATR_LAYOUT_IMAGE):
        dev = torch.device("cuda", 0)
        self.n, self.layout = n, layout
        self.fb = torch.full((n,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
        self.face = torch.full((n,), -7, dtype=torch.int32, device=dev)
        self.t = torch.full((n,), -3.0, dtype=torch.float32, device=dev)
        self.rgb = torch.full((3 * n,), -1.0, dtype=torch.float32, device=dev)
        self.casts = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.traced = torch.zeros(1, dtype=torch.int64, device=dev)
        self.sum = torch.full((3 * n,), float("nan"), dtype=torch.float32, device=dev)
        self.count = torch.full((n,), COUNT_FILL, dtype=torch.int32, device=dev)
        self.fr = E.atr_frame(layout, self.fb.data_ptr(), self.face.data_ptr(), self.t.data_ptr(),
                              self.rgb.data_ptr(), self.casts.data_ptr(), self.traced.data_ptr())

    def host(self, shape=None):
        torch.cuda.synchronize()
        o = {"fb": self.fb.cpu().numpy().view(np.uint32), "face": self.face.cpu().numpy().view(np.uint32),
             "t": self.t.cpu().numpy().view(np.uint32), "rgb": self.rgb.cpu().numpy().view(np.uint32).reshape(-1, 3),
             "casts": self.casts.cpu().numpy().view(np.uint32), "sum": self.sum.cpu().numpy().reshape(-1, 3),
             "count": self.count.cpu().numpy().view(np.uint32), "traced": int(self.traced.item())}
        if shape is not None:
            H, W = shape
            for k in ("fb", "face", "t", "casts", "count"):
                o[k] = o[k].reshape(H, W)
            o["rgb"], o["sum"] = o["rgb"].reshape(H, W, 3), o["sum"].reshape(H, W, 3)
        return o


def run_adaptive(eng, g, passes, tol, tiles=None, layout=E.ATR_LAYOUT_IMAGE, wait_each=True, after=None):
    """The adaptive passes of one frame of golden config g, in order on the current stream;
    after(i, total, frame, info) once pass i is done. Returns the frame and every pass's info."""
    W, H = g["W"], g["H"]
    if tiles is None:
        tiles = [[0, 0, W - 1, H - 1]]
    f = Frame(W * H if layout == E.ATR_LAYOUT_IMAGE else E.packed_size(tiles), layout)
    stream = torch.cuda.current_stream().cuda_stream
    first, infos = 0, []
    for i, n in enumerate(passes):
        cam = E.camera(W, H, n, g["bounces"], g["aa"])
        eng.render_start_adaptive(cam, tiles, f.fr, SEED, first, f.sum.data_ptr(), f.count.data_ptr(), tol,
                                  stream=stream)
        first += n
        if wait_each or after is not None:
            rc, done = eng.wait()
            assert rc == 0 and done == len(tiles)
            infos.append(eng.adaptive_info())
        if after is not None:
            after(i, first, f, infos[-1])
    rc, _ = eng.wait()
    assert rc == 0
    if not infos:
        infos.append(eng.adaptive_info())
    return f, infos


def assert_state(o, name, want_count, pix=None):
    """Every pixel's framebuffer, rgb bits and ray_casts are the oracle's render at the pixel's own
    count, the running sum's mean is the rgb output, and traced_rays lies within the bounds a path's
    rays allow. o: host arrays; pix: the slots' pixel indices (PACKED), None for an image."""
    count = o["count"].reshape(-1)
    want = want_count.reshape(-1) if pix is None else want_count.reshape(-1)[pix]
    assert np.array_equal(count, want)
    n = (count & ~FLAG).astype(np.uint32)
    fb, rgb, casts, summ = o["fb"].reshape(-1), o["rgb"].reshape(-1, 3), o["casts"].reshape(-1), o["sum"].reshape(-1, 3)
    for total in np.unique(n):
        orgb, ofb, ocasts, _ = oracle(name, int(total))
        sel = n == total
        src = np.flatnonzero(sel) if pix is None else pix[sel]
        assert np.array_equal(fb[sel], ofb.reshape(-1)[src]), total
        assert np.array_equal(casts[sel], ocasts.reshape(-1)[src]), total
        assert np.array_equal(rgb[sel], orgb.view(np.uint32).reshape(-1, 3)[src]), total
    mean = (summ / n.astype(np.float32)[:, None]).astype(np.float32)
    assert np.array_equal(mean.view(np.uint32), rgb)
    # a path traces its non-sky bounces (its ray_casts) plus one ray if it ended in the sky
    lo = int(casts.astype(np.int64).sum())
    assert lo <= o["traced"] <= lo + int(n.astype(np.int64).sum()), (lo, o["traced"])


def test_model_matches_the_recorded_schedule():
    """The inputs are not degenerate: the host model gives the values recorded when the cases were
    chosen, so pixels freeze in every pass and some never do."""
    res = model(DRAGON, PASSES, TOL)
    assert [r[1] for r in res] == [(8160, 135, 510, 8160), (8160, 135, 510, 826), (826, 28, 118, 514),
                                   (514, 26, 142, 247), (247, 25, 129, 91)]
    assert set(np.unique(res[-1][0] & ~FLAG).tolist()) == {8, 16, 32, 64}
    aa = model(MONKEY_AA, AA_PASSES, TOL)
    assert [r[1][0] for r in aa] == [2880, 2880, 90, 60] and aa[-1][1][3] == 34
    for name, passes in ((DRAGON, PASSES), (MONKEY_AA, AA_PASSES)):
        means = {int(t): oracle(name, int(t))[0] for t in np.cumsum(passes)}
        assert M.threshold_margin(means, passes, TOL) > 1.0  # no pixel within an ulp of the threshold


def test_tolerance_zero_equals_golden(eng):
    """Tolerance 0 never stops a pixel: the schedule is atr_render_start_samples' and ends at the
    golden; every count is 64 with no flag and every pixel is live in every pass."""
    g = GOLD["render"][DRAGON]
    upload(eng, g["asset"], g["tree"])
    f, infos = run_adaptive(eng, g, PASSES, 0.0)
    o = f.host((g["H"], g["W"]))
    grgb, gfb, gcasts = render(DRAGON)
    assert np.array_equal(o["fb"], gfb)
    assert np.array_equal(o["casts"], gcasts)
    assert np.array_equal(o["rgb"], grgb.view(np.uint32))
    assert o["traced"] == g["counters"]["n_rays"]
    mean = (o["sum"] / np.float32(64)).astype(np.float32)
    assert np.array_equal(mean.view(np.uint32), o["rgb"])
    assert (o["count"] == 64).all()
    assert [i[0] for i in infos] == [8160] * 5 and [i[3] for i in infos] == [8160] * 5
    face, t, _ = scene_of(DRAGON).primary_hits(O.Camera(g["W"], g["H"]))
    assert np.array_equal(o["face"], face) and np.array_equal(o["t"], t.view(np.uint32))


@pytest.mark.parametrize("name,passes", [(DRAGON, PASSES), (MONKEY_AA, AA_PASSES)])
def test_every_pass_equals_model_and_oracle(eng, name, passes):
    """After every pass: the count map with flags and the four info values are the model's, and
    every pixel is the oracle's render at its own count. The AA case's passes of 5, 12 and 30
    samples make path groups straddle pixels."""
    g = GOLD["render"][name]
    upload(eng, g["asset"], g["tree"])
    want = model(name, passes, TOL)

    def after(i, total, f, info):
        assert info == want[i][1], i
        assert_state(f.host((g["H"], g["W"])), name, want[i][0])

    run_adaptive(eng, g, passes, TOL, after=after)


def test_frozen_pixels_are_untouched(eng):
    """A pixel that is not live is neither read (beyond its count) nor written: sentinels put into
    the frozen pixels' outputs after pass 3 survive pass 4 (a NaN sum would poison a pixel that read
    it), and the primary hit outputs, written by pass 1, are left alone by every later pass."""
    g = GOLD["render"][DRAGON]
    H, W = g["H"], g["W"]
    upload(eng, g["asset"], g["tree"])
    want = model(DRAGON, PASSES[:4], TOL)
    frozen = torch.from_numpy((want[2][0] != 16).reshape(-1)).cuda()
    seen = {}

    def after(i, total, f, info):
        if i == 0:
            o = f.host((H, W))
            seen["hits"] = (o["face"], o["t"])
            f.face.fill_(-9)
            f.t.fill_(-5.0)
        if i == 2:
            f.fb[frozen] = 0x11111111
            f.casts[frozen] = 0x22222222
            f.rgb.view(-1, 3)[frozen] = -2.0
            f.sum.view(-1, 3)[frozen] = float("nan")

    f, _ = run_adaptive(eng, g, PASSES[:4], TOL, after=after)
    o = f.host((H, W))
    fz = frozen.cpu().numpy().reshape(H, W)
    assert fz.sum() == W * H - 514
    assert (o["fb"][fz] == 0x11111111).all() and (o["casts"][fz] == 0x22222222).all()
    assert (o["rgb"][fz] == np.float32(-2.0).view(np.uint32)).all() and np.isnan(o["sum"][fz]).all()
    assert np.array_equal(o["count"], want[3][0])
    orgb = {t: oracle(DRAGON, t)[0].view(np.uint32) for t in (16, 32)}
    n = o["count"] & ~FLAG
    for t in (16, 32):  # the live pixels went on as if nothing had happened
        assert np.array_equal(o["rgb"][~fz & (n == t)], orgb[t][~fz & (n == t)])
    face, t, _ = scene_of(DRAGON).primary_hits(O.Camera(W, H))
    assert np.array_equal(seen["hits"][0], face) and np.array_equal(seen["hits"][1], t.view(np.uint32))
    assert (o["face"] == np.uint32(0xFFFFFFF7)).all()  # -9: the poison
    assert (o["t"] == np.float32(-5.0).view(np.uint32)).all()


def test_packed_layout(eng):
    """Three ranks' shard tiles with PACKED outputs, sums and counts: slot by slot the model and
    the oracle, through the slot -> pixel map."""
    g = GOLD["render"][DRAGON]
    W, H = g["W"], g["H"]
    upload(eng, g["asset"], g["tree"])
    full = model(DRAGON, PASSES, TOL)
    for r in range(3):
        tiles = E.make_shard_tiles(W, H, 40, r, 3)
        pix = E.packed_pixel_map(tiles, W, H)
        want = model(DRAGON, PASSES, TOL, pixels=pix)
        f, infos = run_adaptive(eng, g, PASSES, TOL, tiles=tiles, layout=E.ATR_LAYOUT_PACKED)
        assert infos == [w[1] for w in want], r
        assert_state(f.host(), DRAGON, full[-1][0], pix=pix)


@pytest.mark.parametrize("how", ["one_wait", "batches", "no_sort", "cell_plan"])
def test_scheduling_variations_change_nothing(eng, how):
    """The final state is the model's and the oracle's however the passes are scheduled: enqueued
    back to back with one wait; 2^12 paths per batch (a live list per batch, dozens of batches);
    without the queue sort; with every cell planned over two waves (blocks are row bands)."""
    g = GOLD["render"][DRAGON]
    W, H = g["W"], g["H"]
    upload(eng, g["asset"], g["tree"])
    base = eng.tuning()
    waves = 2 if how == "cell_plan" else 1
    want = model(DRAGON, PASSES, TOL, waves=waves)
    try:
        if how == "batches":
            eng.set_tuning(path_batch_log2=12)
        if how == "no_sort":
            eng.set_tuning(path_sort_bits=0)
        if how == "cell_plan":
            eng.set_cell_plan(W, H, np.full(((W + 7) // 8) * ((H + 7) // 8), 2, np.uint8))
        f, infos = run_adaptive(eng, g, PASSES, TOL, wait_each=how != "one_wait")
    finally:
        eng.set_cell_plan(W, H, None)
        eng.set_tuning(**base)
    if how == "one_wait":
        assert infos == [want[-1][1]]
    else:
        assert infos == [w[1] for w in want]
    assert_state(f.host((H, W)), DRAGON, want[-1][0])


def snapshot(f):
    o = f.host()
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in o.items()}


def assert_same(a, b):
    for k in a:
        if k == "sum":
            assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
        else:
            assert np.array_equal(a[k], b[k]), k


def test_passes_that_do_nothing(eng):
    """A pass whose first_sample matches no pixel's count, and a pass after everything converged
    (tolerance 1e30: the second pass stops every pixel), leave every buffer and traced_rays as they
    were and report no live pixel."""
    g = GOLD["render"][DRAGON]
    W, H = g["W"], g["H"]
    tiles = [[0, 0, W - 1, H - 1]]
    upload(eng, g["asset"], g["tree"])
    f, _ = run_adaptive(eng, g, [4, 4], TOL)
    before = snapshot(f)
    eng.render_start_adaptive(E.camera(W, H, 8, g["bounces"]), tiles, f.fr, SEED, 5, f.sum.data_ptr(),
                              f.count.data_ptr(), TOL, stream=torch.cuda.current_stream().cuda_stream)
    assert eng.wait()[0] == 0
    assert eng.adaptive_info() == (0, 0, 0, 0)
    assert_same(before, snapshot(f))

    f, infos = run_adaptive(eng, g, [4, 4], 1e30)
    assert infos[1] == (8160, 135, 510, 0)
    before = snapshot(f)
    assert (before["count"] == (np.uint32(8) | FLAG)).all()
    eng.render_start_adaptive(E.camera(W, H, 8, g["bounces"]), tiles, f.fr, SEED, 8, f.sum.data_ptr(),
                              f.count.data_ptr(), 1e30, stream=torch.cuda.current_stream().cuda_stream)
    assert eng.wait()[0] == 0
    assert eng.adaptive_info() == (0, 0, 0, 0)
    assert_same(before, snapshot(f))


def test_invalid_arguments(eng):
    g = GOLD["render"][DRAGON]
    W, H = g["W"], g["H"]
    tiles = [[0, 0, W - 1, H - 1]]
    f = Frame(W * H)
    fresh = E.Engine(0)
    try:
        with pytest.raises(E.AtrError, match="ATR_E_INVALID"):  # no adaptive pass enqueued yet
            fresh.adaptive_info()
        with pytest.raises(E.AtrError, match="ATR_E_NOSCENE"):  # before atr_scene_upload
            fresh.render_start_adaptive(E.camera(W, H, 1, 5), tiles, f.fr, SEED, 0, f.sum.data_ptr(),
                                        f.count.data_ptr(), TOL)
        with pytest.raises(E.AtrError, match="ATR_E_INVALID"):  # a rejected pass is no pass
            fresh.adaptive_info()
    finally:
        fresh.close()
    upload(eng, g["asset"], g["tree"])
    ok = dict(cam=E.camera(W, H, 1, 5), first=0, tol=TOL)
    bad = [dict(ok, count_ptr=None), dict(ok, sum_ptr=None),
           dict(ok, tol=-1.0), dict(ok, tol=float("nan")), dict(ok, tol=float("inf")),
           dict(ok, variant=E.ATR_KERNEL_FLAT), dict(ok, variant=E.ATR_KERNEL_LANE),
           dict(ok, variant=E.ATR_KERNEL_HYBRID), dict(ok, variant=5),
           dict(ok, cam=E.camera(W, H, 1, 65)), dict(ok, cam=E.camera(W, H, 1, 65), variant=E.ATR_KERNEL_PATHS),
           dict(ok, cam=E.camera(W, H, 0, 5), first=4),
           dict(ok, cam=E.camera(W, H, 2, 5), first=2**24 - 1)]
    for kw in bad:
        with pytest.raises(E.AtrError, match="ATR_E_INVALID"):
            eng.render_start_adaptive(kw["cam"], tiles, f.fr, SEED, kw["first"], kw.get("sum_ptr", f.sum.data_ptr()),
                                      kw.get("count_ptr", f.count.data_ptr()), kw["tol"],
                                      variant=kw.get("variant", E.ATR_KERNEL_AUTO))
    o = f.host()  # and no rejected call touched a buffer
    assert (o["fb"] == 0x7F7F7F7F).all() and np.isnan(o["sum"]).all() and o["traced"] == 0
    assert (o["count"] == COUNT_FILL).all() and (o["casts"] == 0xFFFFFFFF).all()


def test_renderer_adaptive_live_view(eng):
    """renderer.start_render_from_camera(sample_passes=..., adaptive_tolerance=...): tolerance 0 is
    the one-shot render; with 0.01 sample_counts takes only the schedule's totals and pixels_live is
    the info call's value."""
    from atray_amd import renderer as R
    scene = R.app_scene(asset_path("Monkey"), center=CENTERS["Monkey"])
    R.prep_scene(scene, eng)
    rs = R.RenderSettings(resolution=(320, 180), samples_per_pixel=16, bounce_limit=5)

    def info():
        return R.RenderInfo(camera=R.set_camera((0.1, 2.0, 0.0), (-0.1, -0.5, -1.0), rs, 1.0), scene=scene, seed=SEED)

    def finish(i):
        while R.wait_for_render_from_camera_to_finish(i, eng, 33):
            pass
        return i

    one = info()
    R.start_render_from_camera(one, eng)
    finish(one)
    zero = info()
    R.start_render_from_camera(zero, eng, sample_passes=[4, 4, 8], adaptive_tolerance=0.0)
    finish(zero)
    assert np.array_equal(zero.camera_tex, one.camera_tex)
    assert zero.total_ray_casts == one.total_ray_casts
    assert [j.ray_casts for j in zero.jobs] == [j.ray_casts for j in one.jobs]
    assert (zero.sample_counts == 16).all() and zero.sample_counts.shape == (180, 320)
    assert zero.pixels_live == 320 * 180 and zero.samples_done == 16

    ad = info()
    R.start_render_from_camera(ad, eng, sample_passes=[4, 4, 8], adaptive_tolerance=0.01)
    finish(ad)
    assert ad.sample_counts.dtype == np.uint32
    assert set(np.unique(ad.sample_counts).tolist()) == {8, 16}
    assert ad.pixels_live == eng.adaptive_info()[3]
    assert 0 < ad.pixels_live < int((ad.sample_counts == 16).sum()) + 1
    # the pixels that ran the whole schedule are the one-shot render's
    full = ad.sample_counts == 16
    assert np.array_equal(ad.camera_tex[full], one.camera_tex[full])
    assert ad.total_ray_casts <= one.total_ray_casts
    with pytest.raises(ValueError):
        R.start_render_from_camera(info(), eng, adaptive_tolerance=0.01)
