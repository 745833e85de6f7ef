"""Sample-progressive rendering (atr_render_start_samples): a frame's samples rendered in passes
that continue a running f32 sum. Passes covering [0, N) leave every output equal, bit for bit, to
the one-shot N-spp render -- here the committed goldens, which are the oracle's output -- and after
every pass the outputs are the oracle's render at "spp = samples so far". Needs an MI355X (-m gpu)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from atray_amd.assets import CENTERS, asset_path  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests.goldens import GOLD, SEED, render  # noqa: E402

pytestmark = pytest.mark.gpu
PASS_VARIANTS = [E.ATR_KERNEL_PATHS, E.ATR_KERNEL_FLAT]


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


class Frame:
    """A frame's output buffers and its running-sum buffer, filled with values no render leaves
    (the sums with NaN: a first pass that read them would poison every pixel)."""

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
        self.fr = E.atr_frame(layout, self.fb.data_ptr(), self.face.data_ptr(), self.t.data_ptr(),
                              self.rgb.data_ptr(), self.casts.data_ptr(), self.traced.data_ptr())

    def host(self, shape=None):
        torch.cuda.synchronize()
        o = {"fb": self.fb.cpu().numpy().view(np.uint32), "face": self.face.cpu().numpy().view(np.uint32),
             "t": self.t.cpu().numpy().view(np.uint32), "rgb": self.rgb.cpu().numpy().view(np.uint32).reshape(-1, 3),
             "casts": self.casts.cpu().numpy().view(np.uint32), "sum": self.sum.cpu().numpy().reshape(-1, 3),
             "traced": int(self.traced.item())}
        if shape is not None:
            H, W = shape
            for k in ("fb", "face", "t", "casts"):
                o[k] = o[k].reshape(H, W)
            o["rgb"], o["sum"] = o["rgb"].reshape(H, W, 3), o["sum"].reshape(H, W, 3)
        return o


def run_passes(eng, g, passes, variant, tiles=None, layout=E.ATR_LAYOUT_IMAGE, wait_each=True, after=None):
    """The passes of one frame of golden config g, in order on the current stream (variant: one
    for every pass, or one per pass)."""
    W, H = g["W"], g["H"]
    if tiles is None:
        tiles = [[0, 0, W - 1, H - 1]]
    f = Frame(W * H if layout == E.ATR_LAYOUT_IMAGE else E.packed_size(tiles), layout)
    stream = torch.cuda.current_stream().cuda_stream
    first = 0
    for i, n in enumerate(passes):
        cam = E.camera(W, H, n, g["bounces"], g["aa"])
        v = variant[i] if isinstance(variant, (list, tuple)) else variant
        eng.render_start_samples(cam, tiles, f.fr, SEED, first, f.sum.data_ptr(), stream=stream, variant=v)
        first += n
        if wait_each or after is not None:
            rc, done = eng.wait()
            assert rc == 0 and done == len(tiles)
        if after is not None:
            after(i, first, f)
    rc, _ = eng.wait()
    assert rc == 0
    return f


def assert_golden(o, name, spp):
    g = GOLD["render"][name]
    grgb, gfb, gcasts = render(name)
    assert np.array_equal(o["fb"], gfb)
    assert np.array_equal(o["casts"], gcasts)
    assert np.array_equal(o["rgb"], grgb.view(np.uint32))
    assert o["traced"] == g["counters"]["n_rays"]
    # the running sum is the accumulator itself: its mean is the rgb output, bit for bit
    mean = (o["sum"] / np.float32(spp)).astype(np.float32)
    assert np.array_equal(mean.view(np.uint32), o["rgb"])


# 120 x 68: the top row of cells is half masked; 3-, 5-, 12- and 59-sample passes are no power of
# two, so a camera-kernel wavefront (64 paths) straddles pixels
@pytest.mark.parametrize("variant", PASS_VARIANTS)
@pytest.mark.parametrize("passes", [[64], [16, 16, 16, 16], [1, 3, 12, 48], [5, 59]])
def test_dragon_passes_equal_golden(eng, passes, variant):
    name = "dragon_120x68_s64_b5"
    g = GOLD["render"][name]
    upload(eng, g["asset"], g["tree"])
    f = run_passes(eng, g, passes, variant)
    assert_golden(f.host((g["H"], g["W"])), name, 64)


# AA: the jitter draws come from the offset sample's stream
@pytest.mark.parametrize("variant", PASS_VARIANTS)
@pytest.mark.parametrize("passes", [[100], [1, 99], [33, 33, 34]])
def test_monkey_aa_passes_equal_golden(eng, passes, variant):
    name = "monkey_72x40_s100_b3_aa"
    g = GOLD["render"][name]
    upload(eng, g["asset"], g["tree"])
    f = run_passes(eng, g, passes, variant)
    assert_golden(f.host((g["H"], g["W"])), name, 100)


# the brute-force model; and a mostly-sky frame, whose sky pixels resolve through the all-sky
# shortcut in a pass with first_sample > 0
@pytest.mark.parametrize("variant", PASS_VARIANTS)
@pytest.mark.parametrize("name", ["monkey_160x90_s2_b2_bf", "deer_256x144_s2_b5"])
def test_two_single_sample_passes_equal_golden(eng, name, variant):
    g = GOLD["render"][name]
    upload(eng, g["asset"], g["tree"])
    f = run_passes(eng, g, [1, 1], variant)
    assert_golden(f.host((g["H"], g["W"])), name, 2)


_oracle = {}


def oracle_dragon(spp):
    """The oracle's 120 x 68 Dragon render at spp samples (computed once per spp)."""
    if spp not in _oracle:
        g = GOLD["render"]["dragon_120x68_s64_b5"]
        if "scene" not in _oracle:
            _oracle["scene"] = O.Scene(asset_path("Dragon"), center=CENTERS["Dragon"])
            _oracle["hits"] = _oracle["scene"].primary_hits(O.Camera(g["W"], g["H"]))
        _oracle[spp] = _oracle["scene"].render(O.Camera(g["W"], g["H"], spp=spp, bounces=g["bounces"]), SEED)
    return _oracle[spp]


@pytest.mark.parametrize("variant", PASS_VARIANTS)
def test_intermediate_passes_equal_oracle(eng, variant):
    """After each pass of [1, 3, 12] every output is the oracle's render at 1, 4 and 16 spp; the
    primary hit outputs are written by the first pass and left alone by the later ones."""
    g = GOLD["render"]["dragon_120x68_s64_b5"]
    H, W = g["H"], g["W"]
    upload(eng, g["asset"], g["tree"])
    seen = []

    def after(i, total, f):
        o = f.host((H, W))
        rgb, fb, casts, ctr = oracle_dragon(total)
        assert np.array_equal(o["fb"], fb), total
        assert np.array_equal(o["casts"], casts), total
        assert np.array_equal(o["rgb"], rgb.view(np.uint32)), total
        assert o["traced"] == ctr["n_rays"], total
        seen.append((o["face"], o["t"]))
        if i == 1:  # the third pass must leave them alone: any write of its would replace these values
            f.face.fill_(-9)
            f.t.fill_(-5.0)

    run_passes(eng, g, [1, 3, 12], variant, after=after)
    face, t, _ = _oracle["hits"]
    assert np.array_equal(seen[0][0], face) and np.array_equal(seen[0][1], t.view(np.uint32))
    assert np.array_equal(seen[1][0], seen[0][0]) and np.array_equal(seen[1][1], seen[0][1])
    assert (seen[2][0] == np.uint32(0xFFFFFFF7)).all()  # -9: untouched by the third pass
    assert (seen[2][1] == np.float32(-5.0).view(np.uint32)).all()


@pytest.mark.parametrize("variant", PASS_VARIANTS)
def test_packed_layout_passes(eng, variant):
    """Three ranks' shard tiles, passes [4, 60] into PACKED buffers (the sum buffer too): unpacked,
    they are the golden framebuffer."""
    name = "dragon_120x68_s64_b5"
    g = GOLD["render"][name]
    W, H = g["W"], g["H"]
    upload(eng, g["asset"], g["tree"])
    grgb, gfb, gcasts = render(name)
    img = torch.full((W * H,), 0x7F7F7F7F, dtype=torch.int32, device="cuda")
    cimg = torch.full((W * H,), -1, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    for r in range(3):
        tiles = E.make_shard_tiles(W, H, 40, r, 3)
        f = run_passes(eng, g, [4, 60], variant, tiles=tiles, layout=E.ATR_LAYOUT_PACKED)
        eng.unpack(tiles, W, f.fb.data_ptr(), img.data_ptr(), s)
        eng.unpack(tiles, W, f.casts.data_ptr(), cimg.data_ptr(), s)
        o = f.host()
        mean = (o["sum"] / np.float32(64)).astype(np.float32)
        assert np.array_equal(mean.view(np.uint32), o["rgb"])
        pix = E.packed_pixel_map(tiles, W, H)  # slot -> pixel
        assert np.array_equal(o["rgb"], grgb.view(np.uint32).reshape(-1, 3)[pix])
    torch.cuda.synchronize()
    assert np.array_equal(img.cpu().numpy().view(np.uint32).reshape(H, W), gfb)
    assert np.array_equal(cimg.cpu().numpy().view(np.uint32).reshape(H, W), gcasts)


@pytest.mark.parametrize("variant", PASS_VARIANTS)
def test_passes_back_to_back_without_waits(eng, variant):
    """The default schedule's seven passes enqueued on one stream, then one wait."""
    name = "dragon_120x68_s64_b5"
    g = GOLD["render"][name]
    upload(eng, g["asset"], g["tree"])
    f = run_passes(eng, g, [1, 1, 2, 4, 8, 16, 32], variant, wait_each=False)
    assert_golden(f.host((g["H"], g["W"])), name, 64)


@pytest.mark.parametrize("variants", [[E.ATR_KERNEL_PATHS, E.ATR_KERNEL_FLAT, E.ATR_KERNEL_PATHS],
                                      [E.ATR_KERNEL_FLAT, E.ATR_KERNEL_PATHS, E.ATR_KERNEL_FLAT]])
def test_passes_may_change_engine(eng, variants):
    """A pass continues sums another engine wrote -- what the path engine's out-of-memory fallback
    to the cell kernel does in the middle of a frame."""
    name = "dragon_120x68_s64_b5"
    g = GOLD["render"][name]
    upload(eng, g["asset"], g["tree"])
    f = run_passes(eng, g, [5, 27, 32], variants, wait_each=False)
    assert_golden(f.host((g["H"], g["W"])), name, 64)


@pytest.mark.parametrize("variant", [E.ATR_KERNEL_AUTO] + PASS_VARIANTS)
@pytest.mark.parametrize("spp,bounces", [(2, 5), (1, 1)])
def test_first_pass_with_every_sample_equals_render_start(eng, spp, bounces, variant):
    """first_sample = 0 with the full sample count is atr_render_start_ex, hit_face and hit_t
    included -- also for a one-sample, one-bounce frame, which render_start gives to HYBRID."""
    g = dict(GOLD["render"]["dragon_240x135_s2_b5"], bounces=bounces)
    W, H = g["W"], g["H"]
    upload(eng, g["asset"], g["tree"])
    want = Frame(W * H)
    eng.render_start(E.camera(W, H, spp, bounces), [[0, 0, W - 1, H - 1]], want.fr, SEED,
                     stream=torch.cuda.current_stream().cuda_stream)
    assert eng.wait()[0] == 0
    a, b = want.host(), run_passes(eng, g, [spp], variant).host()
    for k in ("fb", "face", "t", "rgb", "casts", "traced"):
        assert np.array_equal(a[k], b[k]), k


def test_invalid_arguments(eng):
    g = GOLD["render"]["dragon_120x68_s64_b5"]
    W, H = g["W"], g["H"]
    tiles = [[0, 0, W - 1, H - 1]]
    f = Frame(W * H)
    fresh = E.Engine(0)
    try:
        with pytest.raises(E.AtrError, match="ATR_E_NOSCENE"):  # before atr_scene_upload
            fresh.render_start_samples(E.camera(W, H, 1, 5), tiles, f.fr, SEED, 0, f.sum.data_ptr())
    finally:
        fresh.close()
    upload(eng, g["asset"], g["tree"])
    bad = [dict(cam=E.camera(W, H, 1, 5), first=0, sum_ptr=None),
           dict(cam=E.camera(W, H, 0, 5), first=4),                    # a pass of no samples
           dict(cam=E.camera(W, H, 2, 5), first=2**24 - 1),            # first + spp > 2^24
           dict(cam=E.camera(W, H, 2**24, 5), first=1),
           dict(cam=E.camera(W, H, 1, 5), first=0, variant=E.ATR_KERNEL_LANE),
           dict(cam=E.camera(W, H, 1, 5), first=0, variant=E.ATR_KERNEL_HYBRID),
           dict(cam=E.camera(W, H, 1, 1), first=0, variant=E.ATR_KERNEL_HYBRID),
           dict(cam=E.camera(W, H, 1, 5), first=0, variant=5)]
    for kw in bad:
        with pytest.raises(E.AtrError, match="ATR_E_INVALID"):
            eng.render_start_samples(kw["cam"], tiles, f.fr, SEED, kw["first"], kw.get("sum_ptr", f.sum.data_ptr()),
                                     variant=kw.get("variant", E.ATR_KERNEL_AUTO))
    o = f.host()  # and no rejected call touched a buffer
    assert (o["fb"] == 0x7F7F7F7F).all() and np.isnan(o["sum"]).all() and o["traced"] == 0


@pytest.mark.parametrize("cell_waves", [0, 2])
def test_path_split_tuning_is_ignored_by_passes(eng, cell_waves):
    """tuning path_split = 1 (one-batch launches of at least 1,024 cells run as two halves on two
    streams): a sample pass still runs as one range and equals the golden. 320 x 180 is 920 cells,
    below the split's threshold, so the case is also run with every cell planned over two waves:
    1,840 blocks, which a one-shot launch does split."""
    name = "monkey_320x180_s4_b5"
    g = GOLD["render"][name]
    W, H = g["W"], g["H"]
    upload(eng, g["asset"], g["tree"])
    base = eng.tuning()
    try:
        eng.set_tuning(path_split=1)
        if cell_waves:
            eng.set_cell_plan(W, H, np.full(((W + 7) // 8) * ((H + 7) // 8), cell_waves, np.uint8))
        f = run_passes(eng, g, [1, 3], E.ATR_KERNEL_PATHS, wait_each=False)
        assert_golden(f.host((H, W)), name, 4)
    finally:
        eng.set_cell_plan(W, H, None)
        eng.set_tuning(**base)


def test_renderer_sample_progressive_live_view(eng):
    """renderer.start_render_from_camera(sample_passes=True): samples_done never decreases and ends
    at spp; camera_tex, the per-tile ray_casts and total_ray_casts are the one-shot call's."""
    from atray_amd import renderer as R
    scene = R.app_scene(asset_path("Monkey"), center=CENTERS["Monkey"])
    R.prep_scene(scene, eng)
    rs = R.RenderSettings(resolution=(320, 180), samples_per_pixel=4, bounce_limit=5)

    def info():
        return R.RenderInfo(camera=R.set_camera((0.1, 2.0, 0.0), (-0.1, -0.5, -1.0), rs, 1.0), scene=scene, seed=SEED)

    one = info()
    R.start_render_from_camera(one, eng)
    while R.wait_for_render_from_camera_to_finish(one, eng, 33):
        pass
    for passes in (True, [3, 1]):
        prog = info()
        R.start_render_from_camera(prog, eng, sample_passes=passes)
        seen = [prog.samples_done]
        while R.wait_for_render_from_camera_to_finish(prog, eng, 0):
            seen.append(prog.samples_done)
            if prog.samples_done:  # a whole (noisy) frame is there once the first pass is done
                assert prog.camera_tex is not None and prog.camera_tex.shape == (180, 320)
        seen.append(prog.samples_done)
        assert seen == sorted(seen) and seen[0] == 0 and seen[-1] == 4
        assert set(seen) <= ({0, 1, 2, 4} if passes is True else {0, 3, 4})
        assert np.array_equal(prog.camera_tex, one.camera_tex)
        assert [j.ray_casts for j in prog.jobs] == [j.ray_casts for j in one.jobs]
        assert prog.total_ray_casts == one.total_ray_casts and prog.jobs_done == one.jobs_done == 40
    _, gfb, _ = render("monkey_320x180_s4_b5")
    assert np.array_equal(one.camera_tex, gfb)
    with pytest.raises(ValueError):
        R.start_render_from_camera(info(), eng, tiles_per_launch=3, sample_passes=True)
    with pytest.raises(ValueError):
        R.start_render_from_camera(info(), eng, sample_passes=[1, 2])  # does not sum to spp
