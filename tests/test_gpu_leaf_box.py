"""The primary kernels' leaf boxes (ATR_LEAF_BOX): the wave-walked pass of HYBRID's
primary table kernels leaves out a leaf whose per-(camera, leaf) box the lane's ray misses. No cluster
of such a leaf passes its loose test for that ray, so nothing may change: a context created with
ATR_LEAF_BOX=0, the default context and the oracle must agree bit for bit on the framebuffer, hit_face,
hit_t and ray_casts, through HYBRID, AUTO and FLAT-primary, at 6 / 7 / 8 waves, in both layouts, with
one camera and with three per launch. The instrumented render, which scans every leaf, must count no
unsound skip, some skipped visits where the eye is outside the boxes, and every earlier counter as the
switched-off context does. The row read back with atr_camera_leaf_boxes_row -- built by the kernels a
launch runs -- must hold every cluster box grown by that row's table growth (float64). Needs an
MI355X (-m gpu)."""
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from atray_amd.assets import CENTERS, asset_path  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import analytic_scenes as AS  # noqa: E402
from tests import scale_scenes as S  # noqa: E402
from tests import test_gpu_scenes as TS  # noqa: E402
from tests import test_gpu_wave_cull as WC  # noqa: E402
from tests.goldens import SEED  # noqa: E402
from tests.test_deep_trees_cpu import IMG_H, IMG_W, epart as deep_epart, inside_camera, opart as deep_opart, outside_camera  # noqa: E402
from tests.test_gpu_camera_pads import frames_of, run_cameras  # noqa: E402
from tests.test_gpu_parity import MODEL, SKY, run  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
OUT_KEYS = ("fb", "face", "casts")
APP_EYE, APP_FACING = WC.APP_EYE, WC.APP_FACING
MONKEY_C = CENTERS["Monkey"]
PAD_CAP = 256 << 20  # the tables' cap (capi.cpp kPadMaxBytes)


def _engine(**env):
    """A context created with these variables set (None: unset); they are read at creation."""
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        return E.Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def pair():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    off, on = _engine(ATR_LEAF_BOX="0"), _engine(ATR_LEAF_BOX=None)
    yield off, on
    off.close()
    on.close()


@pytest.fixture(autouse=True)
def _restore_tuning(pair):
    base = pair[1].tuning()
    yield
    for e in pair:
        e.set_tuning(**base)


def same(a, b, what=""):
    for k in OUT_KEYS:
        assert np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))
    assert np.array_equal(np.asarray(a["t"]).view(np.uint32), np.asarray(b["t"]).view(np.uint32)), (what, "t")
    assert a["traced"] == b["traced"], (what, "traced")


# ---- the scenes ----------------------------------------------------------------------------------------

class Case:
    """A scene and a camera: the engine's upload arguments, the oracle's scene, the frame, the cluster
    size, and whether some (ray, leaf) visit must be skipped (None: decided from the row, see below;
    "may": not asserted either way)."""

    def __init__(self, models, oracle, W, H, eye=APP_EYE, facing=APP_FACING, cluster=16, materials=(SKY, MODEL),
                 spheres=(), planes=(), skips=True):
        self.models, self.oracle, self.W, self.H = models, oracle, W, H
        self.eye, self.facing, self.cluster = tuple(float(x) for x in eye), tuple(float(x) for x in facing), cluster
        self.materials, self.spheres, self.planes, self.skips = list(materials), list(spheres), list(planes), skips
        self._ref = None

    def upload(self, pair):
        for e in pair:
            e.set_tuning(cluster_size=self.cluster)
            e.upload(self.materials, self.models(), self.spheres, self.planes)

    def cam(self, eye=None):
        return E.camera(self.W, self.H, eye=eye or self.eye, facing=self.facing)

    def ref(self):
        """The oracle's frame, computed once: hits, framebuffer, ray_casts."""
        if self._ref is None:
            s = self.oracle()
            face, t, _ = s.primary_hits(O.Camera(self.W, self.H, eye=self.eye, facing=self.facing))
            _, fb, casts, ctr = s.render(O.Camera(self.W, self.H, spp=1, bounces=1, eye=self.eye, facing=self.facing), SEED)
            for a in (face, t, fb, casts):
                a.setflags(write=False)
            self._ref = {"face": face, "t": t, "fb": fb, "casts": casts, "traced": ctr["n_rays"]}
        return self._ref


_assets, _texts = {}, {}


def asset_case(asset, leaf, W, H, **kw):
    def models():
        key = (asset, leaf)
        if key not in _assets:
            m = E.Mesh.load_obj(asset_path(asset))
            box = m.translate_to(m.aabb(), CENTERS[asset])
            _assets[key] = (m, E.Octree.build(m, leaf), box, 1)
        return [_assets[key]]
    return Case(models, lambda: O.Scene(asset_path(asset), center=CENTERS[asset], max_faces=leaf), W, H, **kw)


def soup_case():
    def models():
        if "soup" not in _texts:
            m = E.Mesh.parse_obj(WC._soup())
            _texts["soup"] = (m, E.Octree.build(m, 300), m.aabb(), 1)
        return [_texts["soup"]]
    return Case(models, lambda: O.Scene(obj_text=WC._soup(), center=None, max_faces=300), 128, 96)


def deep_case(name, camera):
    kw = camera(name)
    return Case(lambda: [deep_epart(name) + (1,)], lambda: deep_opart(name), IMG_W, IMG_H, skips=None, **kw)


def scale_case(key):
    sc = S.scene(*key)
    plain = AS.TextSc(sc.text, True, sc.leaf, 1, [SKY, MODEL])
    return Case(lambda: plain.models(), lambda: plain.oracle(), S.RW, S.RH, skips=None, **sc.cam)


TWO = TS.Sc(["monkey", "deer"], [2, 3], TS.MATS, TS.SPHERES, TS.PLANES)  # two trees (lf_base), a sphere, a plane

CASES = {
    "cube_root_leaf": lambda: asset_case("Cube", 300, 64, 48, skips=False),  # the root never split: no pass
    # one inner node, eight leaves; the Cube's twelve triangles span its faces, so each leaf's content is
    # its whole octant and a ray that enters the octant enters the box: nothing to skip is no failure
    "cube_tiny_tree": lambda: asset_case("Cube", 6, 64, 48, skips="may"),
    "monkey_160x120": lambda: asset_case("Monkey", 300, 160, 120),
    "monkey_rewalks": lambda: asset_case("Monkey", 16, 64, 48),              # rays with > 8 candidate leaves
    "soup_near_ktol": soup_case,
    "monkey_61x45": lambda: asset_case("Monkey", 300, 61, 45),               # partial cells
    # facing exactly -z at the model's centre: column 36 has d.x = 0 and row 28 d.y = 0, 1 / d is infinite
    # there and those lanes skip nothing
    "monkey_minus_z": lambda: asset_case("Monkey", 300, 72, 56, eye=(MONKEY_C[0], MONKEY_C[1], MONKEY_C[2] + 3.0),
                                         facing=(0.0, 0.0, -1.0)),
    "monkey_eye_in_root": lambda: asset_case("Monkey", 300, 64, 48, eye=(0.9, 1.6, -1.5),
                                             facing=(MONKEY_C[0] - 0.9, MONKEY_C[1] - 1.6, MONKEY_C[2] + 1.5)),
    "monkey_cluster4": lambda: asset_case("Monkey", 300, 64, 48, cluster=4),
    "two_trees_sphere_plane": lambda: Case(TWO.models, TWO.oracle, TS.W, TS.H, materials=TWO.materials,
                                           spheres=TWO.spheres, planes=TWO.planes),
    "deep_d9_outside": lambda: deep_case("d9", outside_camera),              # a tree deeper than 8 levels
    "deep_d9_inside": lambda: deep_case("d9", inside_camera),
}
for _k in S.SWITCHED:  # the far-scale scenes
    CASES["scale_" + S.key_id(_k)] = (lambda k: (lambda: scale_case(k)))(_k)
_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = CASES[name]()
    return _cases[name]


def skippable(eng, eye):
    """From the row the launch reads: is there a leaf whose box the eye lies outside of (or an empty one)?
    Where every grown box holds the eye -- far out the growths exceed the scene -- no ray from the eye
    can miss any of them, and only then is a scene exempt from 'something is skipped'."""
    lo, hi, flag, _ = eng.camera_leaf_boxes_row(eye)
    e = np.asarray(F(eye))
    holds = ((lo <= e) & (e <= hi)).all(axis=1)
    return bool(((flag == 0) & ~holds).any() or (flag == 1).any()), flag


def check_case(pair, c, name):
    off, on = pair
    c.upload(pair)
    r = c.ref()
    W, H = c.W, c.H
    cam = c.cam()
    halves = [[0, 0, W // 2 - 1, H - 1], [W // 2, 0, W - 1, H - 1]]
    for occ in (6, 7, 8):  # HYBRID's primary table kernel at each occupancy
        for e in pair:
            e.set_tuning(primary_occ=occ)
        x, y = run(off, cam, variant=E.ATR_KERNEL_HYBRID), run(on, cam, variant=E.ATR_KERNEL_HYBRID)
        same(x, y, (name, occ))
        same(y, r, (name, occ, "oracle"))
        same(run(off, cam, tiles=halves, layout=E.ATR_LAYOUT_PACKED, variant=E.ATR_KERNEL_HYBRID),
             run(on, cam, tiles=halves, layout=E.ATR_LAYOUT_PACKED, variant=E.ATR_KERNEL_HYBRID), (name, occ, "PACKED"))
    for e in pair:
        e.set_tuning(primary_occ=0)
    for variant in (E.ATR_KERNEL_AUTO, E.ATR_KERNEL_FLAT):  # FLAT sends primary frames to the 6-wave kernel
        same(run(on, cam, variant=variant), r, (name, variant, "oracle"))
        same(run(off, cam, variant=variant), r, (name, variant, "off", "oracle"))
        same(run(off, cam, tiles=halves, layout=E.ATR_LAYOUT_PACKED, variant=variant),
             run(on, cam, tiles=halves, layout=E.ATR_LAYOUT_PACKED, variant=variant), (name, variant, "PACKED"))
    # three cameras in one launch (rows 0..2 of one table), both layouts: each frame its own render's
    eyes = [c.eye, tuple(F(v) + F(0.03) * (abs(F(v)) + F(1.0)) for v in c.eye),
            tuple(F(v) - F(0.02) * (abs(F(v)) + F(1.0)) for v in c.eye)]
    cams = [c.cam(eye=tuple(float(v) for v in ey)) for ey in eyes]
    for layout, tiles in ((E.ATR_LAYOUT_IMAGE, [[0, 0, W - 1, H - 1]]), (E.ATR_LAYOUT_PACKED, halves)):
        got = []
        for e in pair:
            n, bufs = run_cameras(e, cams, tiles, layout)
            rc, _ = e.wait()
            assert rc == 0
            torch.cuda.synchronize()
            got.append(frames_of(n, len(cams), bufs))
        for f in range(len(cams)):
            same(got[0][f], got[1][f], (name, layout, f))
        if layout == E.ATR_LAYOUT_IMAGE:
            for k in OUT_KEYS:
                assert np.array_equal(got[1][0][k].reshape(H, W), r[k]), (name, "frame 0 of three", k)
    # the instrumented render
    whole = [[0, 0, W - 1, H - 1]]
    for variant in (E.ATR_KERNEL_HYBRID, E.ATR_KERNEL_FLAT):
        ca, cb = off.counters(cam, whole, SEED, variant), on.counters(cam, whole, SEED, variant)
        assert ca == cb, (name, variant, ca, cb)
        assert off.cull_counters(cam, whole, SEED, variant) == on.cull_counters(cam, whole, SEED, variant), name
        assert off.fold_counters(cam, whole, SEED, variant) == on.fold_counters(cam, whole, SEED, variant), name
        lb, lb0 = on.leaf_box_counters(cam, whole, SEED, variant), off.leaf_box_counters(cam, whole, SEED, variant)
        print(name, variant, cb, lb)
        assert lb0 == {"skipped_visits": 0, "unsound_skips": 0}, (name, lb0)
        assert lb["unsound_skips"] == 0, (name, lb)
        assert lb["skipped_visits"] <= cb["n_leaf"], (name, lb, cb)
        want = c.skips
        if want == "may":
            continue
        if want is None:
            want, flag = skippable(on, c.eye)
            print(name, "skippable from the row:", want, "flags", np.bincount(flag, minlength=3).tolist())
            if not want:
                continue
            want = cb["n_leaf"] > 0
        if want:
            assert lb["skipped_visits"] > 0, (name, lb, cb)
        else:
            assert lb["skipped_visits"] == 0, (name, lb)
    return on


@pytest.mark.parametrize("name", list(CASES))
def test_frames_and_counters(pair, name):
    c = case(name)
    assert int((c.ref()["face"] != E.MISS).sum()) > 20 or name.startswith("scale_")  # the model is in view
    check_case(pair, c, name)


def test_rewalk_scene_does_rewalk():
    """Monkey at a leaf limit of 16: rays that hit and rays that miss scan more than kLeafBuf = 8 leaves."""
    s = O.Scene(asset_path("Monkey"), center=MONKEY_C, max_faces=16)
    cam = O.Camera(64, 48, eye=APP_EYE, facing=APP_FACING)
    leaves, _ = s.leaf_trace(cam, cap=64)
    hit = case("monkey_rewalks").ref()["face"] != E.MISS
    n = (leaves >= 0).sum(axis=-1)
    assert (n[hit] > 8).sum() > 5 and (n[~hit] > 8).sum() > 50


def _eye_case(pair, where):
    """An eye inside a leaf's content box, or on a cluster box face, from the app row's own boxes."""
    off, on = pair
    base = case("monkey_160x120")
    base.upload(pair)
    lo, hi, flag, rng = on.camera_leaf_boxes_row(APP_EYE)
    _, boxes, _ = on.camera_pads_row(APP_EYE)
    k = int(np.argmax(np.where(flag == 0, (hi - lo).prod(axis=1), -1.0)))  # the largest tested leaf
    eye = ((lo[k].astype(np.float64) + hi[k]) / 2).astype(F)
    if where == "face":
        c0 = int(rng[k, 0])
        eye[0] = boxes[c0, 0]  # lo.x of the leaf's first cluster
    eye = tuple(float(v) for v in eye)
    facing = tuple(float(MONKEY_C[i] - eye[i]) if abs(MONKEY_C[i] - eye[i]) > 1e-3 else 0.37 for i in range(3))
    c = asset_case("Monkey", 300, 64, 48, eye=eye, facing=facing, skips=None)
    lo2, hi2, flag2, _ = on.camera_leaf_boxes_row(eye)
    e = np.asarray(F(eye))
    assert flag2[k] == 0 and (lo2[k] <= e).all() and (e <= hi2[k]).all()  # the eye is inside that leaf's box
    return c


@pytest.mark.parametrize("where", ["inside", "face"])
def test_eye_inside_a_leaf_box_and_on_a_box_face(pair, where):
    c = _eye_case(pair, where)
    check_case(pair, c, "eye_" + where)


# ---- the row ---------------------------------------------------------------------------------------------

def row_holds_the_clusters(eng, eye, what):
    lo, hi, flag, rng = eng.camera_leaf_boxes_row(eye)
    row, boxes, _ = eng.camera_pads_row(eye)
    assert len(flag) > 0 and int(rng[:, 1].sum()) == len(row), what  # every cluster belongs to one leaf
    assert ((flag == 1) == (rng[:, 1] == 0)).all(), what               # empty leaves, and only they, carry flag 1
    g = row[:, 0].astype(np.float64)[:, None]
    glo, ghi = boxes[:, 0:3].astype(np.float64) - g, boxes[:, 4:7].astype(np.float64) + g
    tested = 0
    for k in np.flatnonzero(flag == 0):
        a, n = int(rng[k, 0]), int(rng[k, 1])
        assert (lo[k].astype(np.float64) <= glo[a:a + n]).all() and (hi[k].astype(np.float64) >= ghi[a:a + n]).all(), (what, k)
        # and not wastefully: within the slack g (1 + 2^-10) + 2^-20 F and a few floats of the tightest bound
        F_ = np.maximum(np.abs(boxes[a:a + n, 0:3].astype(np.float64) - eye), np.abs(boxes[a:a + n, 4:7].astype(np.float64) - eye))
        room = g[a:a + n] * 2.0 ** -9 + 2.0 ** -19 * F_ + 2.0 ** -21 * np.abs(boxes[a:a + n, 0:3]).astype(np.float64) + 1e-37
        assert (lo[k].astype(np.float64) >= (glo[a:a + n] - room).min(axis=0)).all(), (what, k, "LO too low")
        tested += 1
    for k in np.flatnonzero(flag == 2):  # never skippable: some operand is not finite
        a, n = int(rng[k, 0]), int(rng[k, 1])
        with np.errstate(all="ignore"):
            big = row[a:a + n, 0].astype(F) * F(1.0009765625)
        assert not (np.isfinite(boxes[a:a + n, 0:7]).all() and np.isfinite(big).all()
                    and np.isfinite(np.asarray(eye, F)).all()) or np.abs(boxes[a:a + n, 0:7]).max() > 1e37, (what, k)
    return tested, row


def test_row_holds_every_grown_cluster_box(pair):
    off, on = pair
    nofold = _engine(ATR_FACING_FOLD="0")
    try:
        for name in ("monkey_160x120", "monkey_cluster4", "two_trees_sphere_plane", "cube_tiny_tree"):
            c = case(name)
            c.upload(pair)
            nofold.set_tuning(cluster_size=c.cluster)
            nofold.upload(c.materials, c.models(), c.spheres, c.planes)
            tested, row = row_holds_the_clusters(on, c.eye, name)
            assert tested > 0, name
            # switched off, the readback still builds the row as a launch would
            for a, b in zip(off.camera_leaf_boxes_row(c.eye), on.camera_leaf_boxes_row(c.eye)):
                assert np.array_equal(a, b), name
            # ATR_FACING_FOLD=0: the boxes are sized by the unfolded growths (boxes[:, 8] of the pads row)
            t2, row2 = row_holds_the_clusters(nofold, c.eye, (name, "no fold"))
            _, boxes2, _ = nofold.camera_pads_row(c.eye)
            assert np.array_equal(row2[:, 0], boxes2[:, 8]), name
            assert (row2[:, 0] >= row[:, 0]).all()
            lo_f, hi_f, _, _ = on.camera_leaf_boxes_row(c.eye)
            lo_u, hi_u, _, _ = nofold.camera_leaf_boxes_row(c.eye)
            assert (lo_u <= lo_f).all() and (hi_u >= hi_f).all(), name
            if name == "monkey_160x120":
                assert (row2[:, 0] > row[:, 0]).any() and ((lo_u < lo_f) | (hi_u > hi_f)).any()  # the fold does shrink some
    finally:
        nofold.close()


@pytest.mark.parametrize("key", S.SWITCHED, ids=[S.key_id(k) for k in S.SWITCHED])
def test_row_at_scale(pair, key):
    c = case("scale_" + S.key_id(key))
    c.upload(pair)
    row_holds_the_clusters(pair[1], c.eye, key)


# ---- the table's slots -----------------------------------------------------------------------------------

def test_rows_are_reused_and_rebuilt(pair):
    """The same eyes twice read the cached rows; more eyes than slots rebuild them; an upload forgets them."""
    off, on = pair
    mk, dr = case("monkey_160x120"), asset_case("Dragon", 300, 96, 54)
    dr.upload(pair)
    eyes = [(0.1 + 0.3 * k, 2.0, 0.1 * k) for k in range(7)]
    want = {k: run(off, dr.cam(eye=eyes[k]), variant=E.ATR_KERNEL_HYBRID) for k in range(7)}
    for k in (0, 3, 0, 3, 1, 2, 4, 5, 6, 0, 3, 0):  # miss, miss, hit, hit, every slot rebuilt, again
        same(run(on, dr.cam(eye=eyes[k]), variant=E.ATR_KERNEL_HYBRID), want[k], k)
    first = run(on, dr.cam(), variant=E.ATR_KERNEL_HYBRID)
    cam = E.camera(96, 54)
    on.set_tuning(cluster_size=16)
    on.upload(mk.materials, mk.models())  # same eye, another scene: the cached rows are stale
    again = run(on, cam, variant=E.ATR_KERNEL_HYBRID)
    fresh = _engine(ATR_LEAF_BOX="0")
    try:
        fresh.upload(mk.materials, mk.models())
        same(again, run(fresh, cam, variant=E.ATR_KERNEL_HYBRID), "re-upload")
    finally:
        fresh.close()
    assert not np.array_equal(first["face"], again["face"])


def test_scene_over_the_cap_renders_inline(pair):
    """373,248 small triangles (|ab x ac| around 1e-3, above the tolerance) at a leaf limit of 4, some
    400,000 leaves: with 24 cameras the rows of box growths stay far below the cap, but with the leaf
    boxes they pass it, and the launch takes the inline kernels."""
    off, on = pair
    g = 72
    rng = np.random.default_rng(3)
    idx = np.stack(np.meshgrid(*[np.arange(g)] * 3, indexing="ij"), -1).reshape(-1, 3)
    cell = 8.0 / g
    ctr = (idx + 0.5) * cell + np.array([-4.0, -3.0, -12.0]) + rng.uniform(-0.2, 0.2, idx.shape) * cell
    v = (ctr[:, None, :] + rng.uniform(-0.3, 0.3, (len(ctr), 3, 3)) * cell).astype(F).reshape(-1, 3)
    f = np.arange(len(v), dtype=np.int32).reshape(-1, 3)
    h = C.c_void_p()
    E.check(E.lib().atr_mesh_from_arrays(v.ctypes.data, len(v), f.ctypes.data, len(f), None, 0, None, C.byref(h)), "mesh")
    m = E.Mesh(h.value)
    tree = E.Octree.build(m, 4)
    assert tree.stats()["depth"] <= 8
    for e in pair:
        e.set_tuning(cluster_size=16)
        e.upload([SKY, MODEL], [(m, tree, m.aabb(), 1)])
    nleaves = int(E.lib().atr_camera_leaf_boxes_row(on.h, (C.c_float * 3)(*APP_EYE), None, None, 0))
    nclus = int(E.lib().atr_camera_pads_row(on.h, (C.c_float * 3)(*APP_EYE), None, None, None, 0))
    nf = 24
    assert nf * nclus * 8 < PAD_CAP < nf * (nclus * 8 + nleaves * 32), (nleaves, nclus)
    W, H = 64, 48
    cams = [E.camera(W, H, eye=(0.1 + 0.02 * k, 2.0, 0.0)) for k in range(nf)]
    tiles = [[0, 0, W - 1, H - 1]]
    got = []
    for e in pair:
        n, bufs = run_cameras(e, cams, tiles, E.ATR_LAYOUT_IMAGE)
        rc, _ = e.wait()
        assert rc == 0
        torch.cuda.synchronize()
        got.append(frames_of(n, nf, bufs))
    for k in range(nf):
        same(got[0][k], got[1][k], k)
    assert int((got[1][0]["face"] != E.MISS).sum()) > 50
    lane = run(on, cams[5], variant=E.ATR_KERNEL_LANE)  # and it is the reference's frame
    for k in OUT_KEYS:
        assert np.array_equal(got[1][5][k].reshape(H, W), lane[k]), k
    one = run(on, cams[5], variant=E.ATR_KERNEL_HYBRID)  # one camera: under the cap, from the table
    same(one, lane, "one camera")
