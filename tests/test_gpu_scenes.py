"""GPU parity on scenes the one-model tests never reach: several models in one scene (trees of
different depths, a root-leaf tree, brute force, smooth and flat normals, a material per model,
coincident and interpenetrating meshes, eight models and the upload limits), scenes without models,
cameras with another h_fov, portrait and square frames and an eye among the triangles, and bounce
rays on the grazing triangle soup. Every output of every kernel variant must equal the composed
oracle (oracle.Scene.compose, pinned by tests/test_oracle_scenes.py): framebuffer, ray_casts, hit
face, the bits of t and the traced-ray count exactly, rgb as test_gpu_parity.assert_rgb asks.
Needs an MI355X (-m gpu)."""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from atray_amd.assets import CENTERS, asset_path  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests.goldens import SEED  # noqa: E402
from tests.test_gpu_camera_pads import pair  # noqa: E402,F401
from tests.test_gpu_cluster import grazing_soup  # noqa: E402
from tests.test_gpu_parity import SKY, VARIANTS, assert_rgb, eng, run  # noqa: E402,F401
from tests.test_oracle_scenes import closest_of_singles  # noqa: E402

pytestmark = pytest.mark.gpu
ALL = list(VARIANTS) + [E.ATR_KERNEL_AUTO]
MISS = 0xFFFFFFFF
W, H = 96, 72

# part name -> (asset, centre, leaf size, tree?)
PARTS = {
    "cube": ("Cube", CENTERS["Cube"], 300, True),              # 12 faces: the root is a leaf
    "monkey": ("Monkey", CENTERS["Monkey"], 64, True),          # smooth normals, a tree of depth 5
    "deer": ("Deer", CENTERS["Deer"], 300, True),               # no normals: flat shading
    "cube_bf": ("Cube", (1.3, 0.5, -3.2), 300, False),          # brute force, overlapping the others
    "cube_in_monkey": ("Cube", CENTERS["Monkey"], 300, True),   # around the Monkey, which only its ears leave
    "cube_low": ("Cube", (-0.12, -0.31, -2.63), 300, True),     # cuts through the Monkey's lower half
}
EIGHT = [(-3.9 + 2.6 * (k % 4), 1.6 - 2.5 * (k // 4), -8.5 + 0.4 * k) for k in range(8)]
for _k, _c in enumerate(EIGHT):
    PARTS["cube%d" % _k] = ("Cube", _c, 300, True)
SOUP = dict(n=3000, seed=5, det=(1.0, 100.0), leaf=64)

# emission, reflection, scatter: scatter 0 (diffuse), 0.3, 1 (mirror); every emission distinct
MATS = [SKY, ((0.5, 0.1, 0.1), (0.9, 0.6, 0.3), 0.0), ((0.05, 0.3, 0.1), (0.7, 0.9, 0.7), 0.3),
        ((0.1, 0.1, 0.45), (0.95, 0.95, 0.95), 1.0), ((0.35, 0.3, 0.0), (0.5, 0.6, 0.9), 0.3),
        ((0.0, 0.2, 0.2), (0.8, 0.8, 0.4), 0.6), ((0.02, 0.02, 0.02), (0.6, 0.6, 0.6), 0.1)]
SPHERES = [((-1.6, 1.7, -3.4), 0.5, 5)]
# a floor below the Deer (which reaches y = -204): nearer floors hide the little of it that is in view
PLANES = [((0.0, 1.0, 0.0), -250.0, 6)]

_oparts, _eparts, _composed, _refs = {}, {}, {}, {}


def soup_text():
    if "soup" not in _oparts:
        _oparts["soup"] = grazing_soup(SOUP["n"], SOUP["seed"], SOUP["det"])
    return _oparts["soup"]


def opart(name, material):
    """The oracle's one-model scene of a part (cached; compose copies its model record)."""
    key = (name, material)
    if key not in _oparts:
        if name == "soup":
            _oparts[key] = O.Scene(obj_text=soup_text(), center=None, max_faces=SOUP["leaf"], model_material=material)
        else:
            asset, center, leaf, tree = PARTS[name]
            _oparts[key] = O.Scene(asset_path(asset), center=center, max_faces=leaf, use_tree=tree,
                                   model_material=material)
    return _oparts[key]


def epart(name):
    """The engine's (mesh, tree, box) of a part (cached)."""
    if name not in _eparts:
        if name == "soup":
            m = E.Mesh.parse_obj(soup_text())
            _eparts[name] = (m, E.Octree.build(m, SOUP["leaf"]), m.aabb())
        else:
            asset, center, leaf, tree = PARTS[name]
            m = E.Mesh.load_obj(asset_path(asset))
            box = m.translate_to(m.aabb(), center)
            _eparts[name] = (m, E.Octree.build(m, leaf) if tree else None, box)
    return _eparts[name]


class Sc:
    """A scene: part names with a material each, the material table, spheres and planes."""

    def __init__(self, names, model_mats, materials=MATS, spheres=(), planes=()):
        self.names, self.model_mats = tuple(names), tuple(model_mats)
        self.materials, self.spheres, self.planes = list(materials), list(spheres), list(planes)
        self.key = (self.names, self.model_mats, repr(self.materials), repr(self.spheres), repr(self.planes))

    def parts(self):
        return [opart(n, m) for n, m in zip(self.names, self.model_mats)]

    def oracle(self):
        if self.key not in _composed:
            _composed[self.key] = O.Scene.compose(self.parts(), self.materials, self.spheres, self.planes)
        return _composed[self.key]

    def models(self):
        return [epart(n) + (m,) for n, m in zip(self.names, self.model_mats)]

    def upload(self, eng):
        eng.upload(self.materials, self.models(), self.spheres, self.planes)

    def permuted(self, order):
        return Sc([self.names[i] for i in order], [self.model_mats[i] for i in order], self.materials, self.spheres,
                  self.planes)


MIXED = Sc(["cube", "monkey", "deer", "cube_bf"], [1, 2, 3, 4], MATS, SPHERES, PLANES)
TIES = [Sc(["monkey", "monkey"], m) for m in ([1, 2], [2, 1])]
INSIDE = {"same_centre": Sc(["monkey", "cube_in_monkey"], [2, 1]), "offset": Sc(["monkey", "cube_low"], [2, 1])}
CUBES8 = Sc(["cube%d" % k for k in range(8)], [1 + k % 4 for k in range(8)])
SOUP_SC = Sc(["soup"], [1], [SKY, O.MODEL_MAT])


def ref(sc, W, H, spp=1, bounces=1, **cam):
    """The oracle's outputs for one render of a scene (computed once, shared by the variants)."""
    key = (sc.key, W, H, spp, bounces, repr(sorted(cam.items())))
    if key not in _refs:
        s = sc.oracle()
        face, t, _ = s.primary_hits(O.Camera(W, H, **cam))
        rgb, fb, casts, ctr = s.render(O.Camera(W, H, spp=spp, bounces=bounces, **cam), SEED)
        for a in (face, t, rgb, fb, casts):
            a.setflags(write=False)
        _refs[key] = {"face": face, "t": t, "rgb": rgb, "fb": fb, "casts": casts, "traced": ctr["n_rays"]}
    return _refs[key]


def same(o, r, what="", pix=None):
    """Engine outputs o against oracle outputs r; pix: the slots' pixel indices of a PACKED render."""
    for k in ("face", "fb", "casts"):
        want = r[k] if pix is None else r[k].reshape(-1)[pix]
        bad = np.argwhere(np.asarray(o[k]) != want)
        assert len(bad) == 0, (what, k, len(bad), bad[:5].tolist())
    want_t = r["t"] if pix is None else r["t"].reshape(-1)[pix]
    assert np.array_equal(np.asarray(o["t"]).view(np.uint32), want_t.view(np.uint32)), (what, "t")
    assert_rgb(np.asarray(o["rgb"]), r["rgb"] if pix is None else r["rgb"].reshape(-1, 3)[pix])
    if o.get("traced") is not None:
        assert o["traced"] == r["traced"], (what, "traced", o["traced"], r["traced"])


def check(eng, sc, variant, W=W, H=H, renders=((1, 1), (2, 5)), **cam):
    for spp, bounces in renders:
        same(run(eng, E.camera(W, H, spp, bounces, **cam), variant=variant), ref(sc, W, H, spp, bounces, **cam),
             (variant, spp, bounces))


def seen(sc, W=W, H=H, **cam):
    """Pixels whose primary hit is model i's, per model: the closest of the parts' own one-model
    hits, where the composed scene reports a triangle (no sphere or plane in front)."""
    _, _, who = closest_of_singles(sc.parts(), O.Camera(W, H, **cam))
    tri = ref(sc, W, H, **cam)["face"] != MISS
    return [int(((who == i) & tri).sum()) for i in range(len(sc.names))]


def later_hits(r, spp):
    """Second-or-later bounces that hit something: ray_casts counts a path's non-sky hits, and every
    sample of a pixel shares the primary ray (no anti-aliasing)."""
    first = r["casts"] >= spp  # the primary ray hit: each sample counts it
    return int(r["casts"].astype(np.int64).sum()) - spp * int(first.sum())


# ---- a. the mixed scene ---------------------------------------------------------------------------

def test_mixed_scene_is_in_view():
    """The inputs are not degenerate (oracle only): every model, the sphere and the plane own primary
    pixels, and bounce rays do hit again."""
    assert min(seen(MIXED)) >= 50, seen(MIXED)
    r = ref(MIXED, W, H, 1, 1)
    assert len(np.unique(r["fb"])) == 7  # the sky, four models, the sphere, the plane
    assert later_hits(ref(MIXED, W, H, 2, 5), 2) > 2000
    assert opart("cube", 1).tree_stats()["nodes"] == 1 and opart("monkey", 2).tree_stats()["inner"] > 4
    assert opart("monkey", 2).mesh.nn > 0 and opart("deer", 3).mesh.nn == 0  # smooth and flat


@pytest.mark.parametrize("variant", ALL)
def test_mixed_scene_matches_oracle(eng, variant):
    MIXED.upload(eng)
    check(eng, MIXED, variant)


# ---- b. model order -------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ALL)
@pytest.mark.parametrize("order", [(3, 2, 1, 0), (1, 3, 0, 2)])
def test_model_order_matches_oracle(eng, order, variant):
    sc = MIXED.permuted(order)  # brute force first; the root-leaf tree after the deep one
    sc.upload(eng)
    check(eng, sc, variant)


# ---- c. ties between models ------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ALL)
@pytest.mark.parametrize("first", [0, 1])
def test_coincident_models_first_wins(eng, first, variant):
    sc = TIES[first]
    a, b = (ref(s, W, H, 1, 1)["fb"] for s in TIES)
    assert int((a != b).sum()) > 500  # the order shows in the hit pixels
    assert int((ref(sc, W, H, 2, 4)["casts"] > 0).sum()) > 500  # bounce rays leave the doubly covered surface
    assert later_hits(ref(sc, W, H, 2, 4), 2) >= 50               # and some come back to it
    sc.upload(eng)
    check(eng, sc, variant, renders=((1, 1), (2, 4)))


# ---- d. interpenetrating models ---------------------------------------------------------------------

@pytest.mark.parametrize("variant", ALL)
@pytest.mark.parametrize("where", list(INSIDE))
def test_interpenetrating_models_match_oracle(eng, where, variant):
    """A Cube at the Monkey's centre (from this eye the Cube hides the Monkey: every bounce ray
    starts on the Cube, within or beside the Monkey's boxes), and a Cube through its lower half (both
    in view, rays bouncing between the two)."""
    sc = INSIDE[where]
    if where == "same_centre":
        assert seen(sc)[1] >= 50, seen(sc)
    else:
        assert min(seen(sc)) >= 50, seen(sc)
        assert later_hits(ref(sc, W, H, 2, 5), 2) >= 200
    sc.upload(eng)
    check(eng, sc, variant)


# ---- e. cluster size with several models ------------------------------------------------------------

@pytest.mark.parametrize("variant", [E.ATR_KERNEL_HYBRID, E.ATR_KERNEL_PATHS])
@pytest.mark.parametrize("cluster_size", [1, 5, 16])
def test_cluster_size_with_several_models(eng, cluster_size, variant):
    """cluster_size sets each model's cluster count, so each later model's first cluster."""
    base = eng.tuning()
    try:
        eng.set_tuning(cluster_size=cluster_size)
        MIXED.upload(eng)  # cluster_size applies at upload
        check(eng, MIXED, variant)
    finally:
        eng.set_tuning(**base)


@pytest.mark.parametrize("cluster_size", [1, 5, 16])
def test_growth_table_rows_with_several_models(pair, cluster_size):
    """HYBRID's primaries read a cluster's box growths from the per-camera table at the model's
    first cluster plus the cluster's index. The growths are rounding pads, so a row read from the
    wrong place rarely changes a hit: besides the outputs against the oracle, the work counters of
    a context that reads the table must equal those of one that computes the growths per ray
    (ATR_CAMERA_PADS=0). Two model orders (the one-cluster Cube first; the huge Deer before the
    Monkey), two eyes."""
    off, on = pair
    base = on.tuning()
    tiles = [[0, 0, W - 1, H - 1]]
    try:
        for e in pair:
            e.set_tuning(cluster_size=cluster_size)
        for sc in (MIXED, MIXED.permuted((3, 2, 1, 0))):
            for e in pair:
                sc.upload(e)
            for eye in ((0.1, 2.0, 0.0), orbit(3)):
                cam = E.camera(W, H, eye=eye)
                for e in pair:
                    same(run(e, cam, variant=E.ATR_KERNEL_HYBRID), ref(sc, W, H, eye=eye), (sc.names, eye, e is on))
                ca = off.counters(cam, tiles, SEED, E.ATR_KERNEL_HYBRID)
                cb = on.counters(cam, tiles, SEED, E.ATR_KERNEL_HYBRID)
                assert ca["cluster_boxes"] > ca["n_leaf"] > 0 and ca["screened"] > 0  # the cluster tests did run
                assert ca == cb, (sc.names, eye, ca, cb)
    finally:
        for e in pair:
            e.set_tuning(**base)


# ---- f. the other entry points ----------------------------------------------------------------------

def orbit(k, n=8, r=0.5):
    a = 2.0 * math.pi * k / n
    return (0.1 + r * math.cos(a), 2.0, r * math.sin(a))


class Buffers:
    """nf frames' output buffers of n slots each, filled with values no render leaves."""

    def __init__(self, n, nf=1, layout=E.ATR_LAYOUT_IMAGE):
        dev = torch.device("cuda", 0)
        self.n, self.nf = n, nf
        self.fb = torch.full((nf * n,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
        self.face = torch.full((nf * n,), -7, dtype=torch.int32, device=dev)
        self.t = torch.full((nf * n,), -3.0, dtype=torch.float32, device=dev)
        self.rgb = torch.full((3 * nf * n,), -1.0, dtype=torch.float32, device=dev)
        self.casts = torch.full((nf * n,), -1, dtype=torch.int32, device=dev)
        self.traced = torch.zeros(1, dtype=torch.int64, device=dev)
        self.sum = torch.full((3 * n,), float("nan"), dtype=torch.float32, device=dev)
        self.count = torch.full((n,), 0x7F7F7F7F, dtype=torch.int32, device=dev)
        self.fr = E.atr_frame(layout, self.fb.data_ptr(), self.face.data_ptr(), self.t.data_ptr(),
                              self.rgb.data_ptr(), self.casts.data_ptr(), self.traced.data_ptr())

    def frame(self, f, shape=None):
        torch.cuda.synchronize()
        n = self.n
        o = {"fb": self.fb[f * n:(f + 1) * n].cpu().numpy().view(np.uint32),
             "face": self.face[f * n:(f + 1) * n].cpu().numpy().view(np.uint32),
             "t": self.t[f * n:(f + 1) * n].cpu().numpy(),
             "rgb": self.rgb[3 * f * n:3 * (f + 1) * n].cpu().numpy().reshape(-1, 3),
             "casts": self.casts[f * n:(f + 1) * n].cpu().numpy().view(np.uint32), "traced": None}
        if shape is not None:
            for k in ("fb", "face", "t", "casts"):
                o[k] = o[k].reshape(shape)
            o["rgb"] = o["rgb"].reshape(shape + (3,))
        return o


@pytest.mark.parametrize("variant", [E.ATR_KERNEL_HYBRID, E.ATR_KERNEL_PATHS])
@pytest.mark.parametrize("spp,bounces", [(1, 1), (2, 3)])
def test_cameras_per_launch_match_oracle(eng, spp, bounces, variant):
    """atr_render_start_cameras: three eyes in one launch (HYBRID's primaries read a row of the table
    of box growths per camera, each model from its own first cluster)."""
    MIXED.upload(eng)
    eyes = [orbit(k) for k in (0, 3, 5)]
    b = Buffers(W * H, len(eyes))
    eng.render_start_cameras([E.camera(W, H, spp, bounces, eye=e) for e in eyes], [[0, 0, W - 1, H - 1]], b.fr,
                             W * H, SEED, stream=torch.cuda.current_stream().cuda_stream, variant=variant)
    rc, _ = eng.wait()
    assert rc == 0
    refs = [ref(MIXED, W, H, spp, bounces, eye=e) for e in eyes]
    for f, r in enumerate(refs):
        assert min(seen(MIXED, eye=eyes[f])) >= 30, (f, seen(MIXED, eye=eyes[f]))
        same(b.frame(f, (H, W)), r, (variant, f))
    assert int(b.traced.item()) == sum(r["traced"] for r in refs)
    assert not np.array_equal(refs[0]["face"], refs[1]["face"])  # the cameras do differ


@pytest.mark.parametrize("variant", [E.ATR_KERNEL_PATHS, E.ATR_KERNEL_FLAT])
def test_sample_passes_match_oracle(eng, variant):
    """atr_render_start_samples: passes of 1 and 3 samples leave the oracle's 4-spp render."""
    MIXED.upload(eng)
    b = Buffers(W * H)
    first = 0
    for n in (1, 3):
        eng.render_start_samples(E.camera(W, H, n, 5), [[0, 0, W - 1, H - 1]], b.fr, SEED, first, b.sum.data_ptr(),
                                 stream=torch.cuda.current_stream().cuda_stream, variant=variant)
        first += n
    rc, _ = eng.wait()
    assert rc == 0
    o = b.frame(0, (H, W))
    o["traced"] = int(b.traced.item())
    same(o, ref(MIXED, W, H, 4, 5), variant)


def test_adaptive_passes_at_tolerance_zero_match_oracle(eng):
    """atr_render_start_adaptive at tolerance 0 stops no pixel: the same passes, the same frame."""
    MIXED.upload(eng)
    b = Buffers(W * H)
    first = 0
    for n in (1, 3):
        eng.render_start_adaptive(E.camera(W, H, n, 5), [[0, 0, W - 1, H - 1]], b.fr, SEED, first, b.sum.data_ptr(),
                                  b.count.data_ptr(), 0.0, stream=torch.cuda.current_stream().cuda_stream)
        first += n
    rc, _ = eng.wait()
    assert rc == 0
    o = b.frame(0, (H, W))
    o["traced"] = int(b.traced.item())
    same(o, ref(MIXED, W, H, 4, 5), "adaptive")
    assert (b.count.cpu().numpy().view(np.uint32) == 4).all()


def test_packed_tiles_match_oracle(eng):
    """A PACKED render of two side-by-side tiles, mapped back with atr_packed_pixel_map."""
    MIXED.upload(eng)
    tiles = [[0, 0, 47, H - 1], [48, 0, W - 1, H - 1]]
    pix = E.packed_pixel_map(tiles, W, H)
    assert len(pix) == E.packed_size(tiles) and np.array_equal(np.sort(pix), np.arange(W * H))
    o = run(eng, E.camera(W, H, 2, 5), tiles=tiles, layout=E.ATR_LAYOUT_PACKED)
    same(o, ref(MIXED, W, H, 2, 5), "packed", pix=pix)


# ---- g. eight models, and the limits ------------------------------------------------------------------

@pytest.mark.parametrize("variant", ALL)
def test_eight_models_match_oracle(eng, variant):
    assert min(seen(CUBES8)) >= 50, seen(CUBES8)
    CUBES8.upload(eng)
    check(eng, CUBES8, variant, renders=((1, 1), (2, 3)) if variant == E.ATR_KERNEL_AUTO else ((1, 1),))


def test_rejected_uploads_keep_the_scene(eng):
    """A ninth model, or a model material equal to the material count, is ATR_E_INVALID, and the
    scene uploaded before stays as it was."""
    CUBES8.upload(eng)
    cam = E.camera(W, H, 2, 3)
    before = run(eng, cam)
    same(before, ref(CUBES8, W, H, 2, 3), "before")
    nine = CUBES8.models() + [epart("monkey") + (1,)]
    bad_material = CUBES8.models()[:2] + [epart("monkey") + (len(MATS),)]
    for models in (nine, bad_material):
        with pytest.raises(E.AtrError, match="ATR_E_INVALID"):
            eng.upload(MATS, models)
        after = run(eng, cam)
        for k in ("fb", "face", "t", "casts", "rgb"):
            assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k
        assert before["traced"] == after["traced"]
    eng.upload(MATS, CUBES8.models()[:2] + [epart("monkey") + (len(MATS) - 1,)])  # the last material is valid


# ---- h. no models -------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", [E.ATR_KERNEL_AUTO, E.ATR_KERNEL_FLAT, E.ATR_KERNEL_PATHS])
@pytest.mark.parametrize("empty", [False, True])
def test_scene_without_models_matches_oracle(eng, empty, variant):
    sc = Sc([], [], MATS) if empty else Sc([], [], MATS, SPHERES + [((0.3, 0.6, -3.0), 0.7, 3)], PLANES)
    r = ref(sc, W, H, 1, 1)
    assert (r["face"] == MISS).all()
    assert len(np.unique(r["fb"])) == (1 if empty else 4)  # all sky; or the sky, two spheres and the plane
    sc.upload(eng)
    check(eng, sc, variant)


# ---- i. cameras -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ALL)
@pytest.mark.parametrize("W,H,h_fov", [(96, 72, 0.35), (96, 72, 2.5), (54, 96, 1.0), (40, 40, 1.0)])
def test_camera_shapes_match_oracle(eng, W, H, h_fov, variant):
    hits = int((ref(MIXED, W, H, h_fov=h_fov)["face"] != MISS).sum())
    assert hits >= 150, hits
    MIXED.upload(eng)
    check(eng, MIXED, variant, W, H, renders=((1, 1), (2, 3)), h_fov=h_fov)


# an eye inside the soup's bounding box, among its triangles (a closed mesh would show its culled back faces)
EYE_IN = dict(eye=(-0.4, 0.0, -4.0), facing=(-0.1, -0.5, -1.0))


@pytest.mark.parametrize("variant", ALL)
def test_eye_among_the_triangles_matches_oracle(eng, variant):
    box = opart("soup", 1).surrounding_aabb
    e = EYE_IN["eye"]
    assert all(box[k] < e[k] < box[3 + k] for k in range(3)), box
    assert int((ref(SOUP_SC, W, H, **EYE_IN)["face"] != MISS).sum()) >= 200
    SOUP_SC.upload(eng)
    check(eng, SOUP_SC, variant, renders=((1, 1), (2, 3)), **EYE_IN)


# ---- j. bounce rays on the grazing soup ---------------------------------------------------------------

@pytest.mark.parametrize("variant", ALL)
def test_bounce_rays_on_grazing_soup_match_oracle(eng, variant):
    """Bounce rays start on a triangle: the t > tolerance self-hit edge and, on the soup's exact
    duplicates, the equal-t leaf-order rule, in the bounce flavours of the clustered scan."""
    r = ref(SOUP_SC, 128, 96, 2, 5)
    assert later_hits(r, 2) >= 1000, later_hits(r, 2)
    SOUP_SC.upload(eng)
    check(eng, SOUP_SC, variant, 128, 96, renders=((2, 5),))
