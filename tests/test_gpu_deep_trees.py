"""GPU parity on octrees deeper and wider than any asset's (tests/deep_trees.py; their depths and
inner-node counts are pinned by tests/test_deep_trees_cpu.py): the high half of the traversal's mask
stack (an inner node at depth 8 to 14), the near-first pass with its fullest register stack (depth 8)
and the fallback from it by depth (9, 15) and by inner-node count (2^16 or more), per model; the depth
limit of an upload (15 accepted, 16 rejected) and ATR_E_TREE_LAYOUT through the API, each leaving
the scene uploaded before in place; the device build at depth. Every comparison is bit for bit, against the
oracle or the occlusion reference: face, the bits of t, uv and rgb, framebuffer, ray counts, work
counters and occlusion bytes. Needs an MI355X (-m gpu)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import deep_trees as D  # noqa: E402
from tests import occlusion_ref as OR  # noqa: E402
from tests import ray_sets as R  # noqa: E402
from tests import test_gpu_scenes as TS  # noqa: E402
from tests import test_gpu_trace_rays as TR  # noqa: E402
from tests.goldens import SEED  # noqa: E402
from tests.test_deep_trees_cpu import (IMG_H, IMG_W, deep_scan_share, epart, exported, inside_camera,  # noqa: E402
                                       opart, outside_camera)
from tests.test_gpu_build import _same  # noqa: E402
from tests.test_gpu_occlusion import occl  # noqa: E402
from tests.test_gpu_parity import MODEL, SKY, VARIANTS, eng, run  # noqa: E402,F401

pytestmark = pytest.mark.gpu
F = np.float32
ALL = list(VARIANTS) + [E.ATR_KERNEL_AUTO]
BOUNCE = (E.ATR_KERNEL_AUTO, E.ATR_KERNEL_PATHS, E.ATR_KERNEL_FLAT)
QUERY = (E.ATR_KERNEL_AUTO, E.ATR_KERNEL_LANE)
SORTS = (0, -1)
SCENES = ["d8", "d9", "d15", "wide", "twin"]
CAMERAS = {"inside": inside_camera, "outside": outside_camera}
SPP, BOUNCES = 2, 3
N_AIMED, N_SMALL = 4097, 1025

_refs, _rays, _traces, _occl = {}, {}, {}, {}
_uploaded = [None]


def upload(eng, name):
    """One generated tree as the scene's only model (skipped while it is the scene already)."""
    if _uploaded[0] != (id(eng), name):
        _uploaded[0] = None
        eng.upload([SKY, MODEL], [epart(name) + (1,)])
        _uploaded[0] = (id(eng), name)


def ref(name, cam, spp=1, bounces=1):
    """The oracle's outputs of one render (computed once, read-only)."""
    key = (name, cam, spp, bounces)
    if key not in _refs:
        s, kw = opart(name), CAMERAS[cam](name)
        face, t, ctr = s.primary_hits(O.Camera(IMG_W, IMG_H, **kw))
        rgb, fb, casts, rc = s.render(O.Camera(IMG_W, IMG_H, spp=spp, bounces=bounces, **kw), SEED)
        for a in (face, t, rgb, fb, casts):
            a.setflags(write=False)
        _refs[key] = {"face": face, "t": t, "rgb": rgb, "fb": fb, "casts": casts, "traced": rc["n_rays"],
                      "counters": ctr}
    return _refs[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_render(o, r, what, keys=("fb", "face", "t", "rgb", "casts")):
    for k in keys:
        bad = np.argwhere(bits(o[k]) != bits(r[k]))
        assert len(bad) == 0, (what, k, len(bad), bad[:5].tolist())
    assert o["traced"] == r["traced"], (what, "traced", o["traced"], r["traced"])


def tree_depth(name):
    return int(D.node_depths(exported(name)[1]).max())


def deep_inner_box(name):
    return D.deepest_inner(*exported(name)[:2])[2]


def rays(name, kind):
    """A named batch of a scene (cached, read-only): `inside` the deepest inner node's box, `aimed` at
    the boxes of the leaves at depth 9 or more (at the deepest leaves of a shallower tree) and, every
    other ray, at the first triangle of such a leaf, `second`: from the hit points of the aimed batch."""
    if (name, kind) not in _rays:
        bounds, children, first, count, verts = exported(name)[:5]
        if kind == "inside":
            o, d = R.inside(deep_inner_box(name), N_SMALL, 41)
        elif kind == "aimed":
            lvl = min(9, tree_depth(name))
            boxes = D.leaf_boxes(bounds, children, count, lvl) + D.leaf_triangle_boxes(children, first, count, verts, lvl)
            o, d = R.aimed(boxes, N_AIMED, 42)
        else:
            ao, ad = rays(name, "aimed")
            o, d = R.second_generation(ao, ad, trace(name, "aimed")[1], 43, N_SMALL)
        o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
        assert R.passes(o, d).all(), (name, kind)
        o.setflags(write=False)
        d.setflags(write=False)
        _rays[name, kind] = (o, d)
    return _rays[name, kind]


def trace(name, kind):
    """The oracle's (face, t, uv) of a batch (cached, read-only)."""
    if (name, kind) not in _traces:
        face, t, uv, _ = opart(name).trace(*rays(name, kind))
        for a in (face, t, uv):
            a.setflags(write=False)
        _traces[name, kind] = (face, t, uv)
    return _traces[name, kind]


def occluded(name, kind):
    """(t_max, the reference's bytes) of a batch, t_max taken as tests/test_gpu_occlusion.py takes its
    random set (cached, read-only)."""
    if (name, kind) not in _occl:
        tm = OR.random_tmax(trace(name, kind)[1])
        w = OR.occluded(opart(name), *rays(name, kind), tm)
        tm.setflags(write=False)
        w.setflags(write=False)
        _occl[name, kind] = (tm, w)
    return _occl[name, kind]


# ---- 1. primary hits ----------------------------------------------------------------------------------

def assert_cap(name):
    """The inside camera's primaries do walk the deep levels (asserted on the CPU as well)."""
    if name in ("d9", "d15"):
        share = deep_scan_share(name, **inside_camera(name))
        assert share >= 0.9, (name, share)


@pytest.mark.parametrize("cam", list(CAMERAS))
@pytest.mark.parametrize("name", SCENES)
def test_primary_hits_match_oracle(eng, name, cam):
    """HYBRID and AUTO walk the tree with traverse_pass_wave, LANE, FLAT and PATHS with traverse_pass."""
    if cam == "inside":
        assert_cap(name)
    r = ref(name, cam)
    assert int((r["face"] != E.MISS).sum()) >= 100, (name, cam)
    upload(eng, name)
    for variant in ALL:
        o = run(eng, E.camera(IMG_W, IMG_H, **CAMERAS[cam](name)), variant=variant)
        same_render(o, r, (name, cam, variant), keys=("face", "t", "fb"))


# ---- 2. work counters ------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", VARIANTS)
def test_work_counters_equal_reference_work_at_depth(eng, variant):
    """As test_gpu_work_counters_equal_reference_work, on the depth-15 tree from inside: equal box
    tests mean the walk order and the five-hit break are the reference's on the deep levels too."""
    assert_cap("d15")
    want = ref("d15", "inside")["counters"]
    upload(eng, "d15")
    c = eng.counters(E.camera(IMG_W, IMG_H, **inside_camera("d15")), [[0, 0, IMG_W - 1, IMG_H - 1]], SEED, variant)
    for k in ["n_rays", "n_box", "n_leaf"]:
        assert c[k] == want[k], (k, c[k], want[k])
    if variant != E.ATR_KERNEL_LANE:
        # the clustered scan visits the same leaves but skips provably irrelevant triangles
        assert 0 < c["n_tri"] <= want["n_tri"], (c["n_tri"], want["n_tri"])
    else:
        assert c["n_tri"] == want["n_tri"], (c["n_tri"], want["n_tri"])


# ---- 3. multi-bounce renders -------------------------------------------------------------------------------

@pytest.mark.parametrize("cam", list(CAMERAS))
@pytest.mark.parametrize("name", ["d8", "d9", "d15", "wide"])
def test_multibounce_render_matches_oracle(eng, name, cam):
    """Bounce rays: depth 8 is the near-first pass with its fullest stack, depth 9 and 15 fall back
    from it by depth, the wide tree by its inner-node count."""
    r = ref(name, cam, SPP, BOUNCES)
    assert TS.later_hits(r, SPP) >= 15, (name, cam, TS.later_hits(r, SPP))  # bounce rays do hit again
    upload(eng, name)
    st = epart(name)[1].stats()
    assert (st["depth"] <= 8 and st["inner"] < 65536) == (name == "d8")  # which pass the bounces take
    for variant in BOUNCE:
        o = run(eng, E.camera(IMG_W, IMG_H, SPP, BOUNCES, **CAMERAS[cam](name)), variant=variant)
        same_render(o, r, (name, cam, variant))


# ---- 4. ray queries ----------------------------------------------------------------------------------------

def check_queries(eng, name, kind, rows=None):
    orig, dirs = rays(name, kind)
    want = trace(name, kind)
    tm, wocc = occluded(name, kind)
    if rows is not None:
        orig, dirs, tm, wocc = orig[rows], dirs[rows], tm[rows], wocc[rows]
        want = tuple(a[rows] for a in want)
    for variant in QUERY:
        for sb in SORTS:
            what = (name, kind, variant, sb)
            res = TR.query(eng, orig, dirs, variant, sb)
            TR.assert_parity(res, want, what)
            assert res["traced"] == len(orig), (what, res["traced"])
            got, traced = occl(eng, orig, dirs, tm, variant, sb)
            bad = np.flatnonzero(got != wocc)
            assert len(bad) == 0, (what, "occluded", len(bad), bad[:8].tolist())
            assert traced == len(orig), (what, traced)


@pytest.mark.parametrize("kind", ["inside", "aimed", "second"])
@pytest.mark.parametrize("name", SCENES)
def test_ray_queries_match_oracle(eng, name, kind):
    orig, _ = rays(name, kind)
    if kind == "inside":  # every origin lies at the bottom of the tree
        at = D.inner_depth_at(*exported(name)[:2], orig)
        assert (at == tree_depth(name) - 1).all(), (name, np.unique(at).tolist())
        if name in ("d9", "d15"):
            assert (at >= 8).all() and (name != "d15" or (at == 14).all())
    # the inputs are not degenerate: triangles are hit (the grid's fill 1 % of a cell: fewer there)
    assert len(orig) >= 500 and int((trace(name, kind)[0] != R.MISS).sum()) >= 15, (name, kind, len(orig))
    assert set(np.unique(occluded(name, kind)[1]).tolist()) == {0, 1}
    upload(eng, name)
    check_queries(eng, name, kind)


@pytest.mark.parametrize("n", [1, 65])
def test_ray_queries_at_wave_tails(eng, n):
    upload(eng, "d15")
    check_queries(eng, "d15", "aimed", slice(0, n))


# ---- 5. near_ok is per model --------------------------------------------------------------------------------

@pytest.mark.parametrize("order", [("d15", "monkey"), ("monkey", "d15")])
def test_near_first_pass_is_chosen_per_model(eng, order):
    """The depth-15 tree beside the Monkey at leaf size 64 (depth 5), which it overlaps: the shallow
    model takes the near-first pass, the deep one the fallback, in either upload order."""
    mats = {"d15": 1, "monkey": 2}
    eparts = {"d15": epart("d15"), "monkey": TS.epart("monkey")}
    oparts = {"d15": opart("d15", 1), "monkey": TS.opart("monkey", 2)}
    assert eparts["monkey"][1].stats()["depth"] <= 8 < eparts["d15"][1].stats()["depth"]
    s = O.Scene.compose([oparts[n] for n in order], TS.MATS)
    _uploaded[0] = None
    eng.upload(TS.MATS, [eparts[n] + (mats[n],) for n in order])
    face, t, _ = s.primary_hits(O.Camera(IMG_W, IMG_H))
    rgb, fb, casts, ctr = s.render(O.Camera(IMG_W, IMG_H, spp=SPP, bounces=BOUNCES), SEED)
    r = {"face": face, "t": t, "rgb": rgb, "fb": fb, "casts": casts, "traced": ctr["n_rays"]}
    own = {n: oparts[n].primary_hits(O.Camera(IMG_W, IMG_H))[1] for n in order}
    assert int((own["monkey"] < own["d15"]).sum()) >= 100 and int((own["d15"] < own["monkey"]).sum()) >= 100
    assert TS.later_hits(r, SPP) >= 100  # both models in view, and bounce rays hit again
    for variant in BOUNCE:
        same_render(run(eng, E.camera(IMG_W, IMG_H, SPP, BOUNCES), variant=variant), r, (order, variant))
    bounds, children, _, count = exported("d15")[:4]
    boxes = []
    for b in D.leaf_boxes(bounds, children, count, 9, limit=7):  # every other ray at the Monkey
        boxes += [np.asarray(oparts["monkey"].surrounding_aabb, F), b]
    ao, ad = R.aimed(boxes, N_AIMED, 44)
    o, d = R.second_generation(ao, ad, s.trace(ao, ad)[1], 45, N_SMALL)
    assert len(o) >= 500 and R.passes(o, d).all()
    want = s.trace(o, d)[:3]
    own = {n: oparts[n].trace(o, d)[1] for n in order}  # bounce rays hit either model
    assert int((own["monkey"] < own["d15"]).sum()) >= 30 and int((own["d15"] < own["monkey"]).sum()) >= 30
    for variant in QUERY:
        for sb in SORTS:
            TR.assert_parity(TR.query(eng, o, d, variant, sb), want, (order, variant, sb))


# ---- 6. the depth limit, and the layout check ------------------------------------------------------------------

def assert_unchanged(eng, cam, before, what):
    after = run(eng, cam)
    for k in ("fb", "face", "t", "casts", "rgb"):
        assert np.array_equal(bits(before[k]), bits(after[k])), (what, k)
    assert before["traced"] == after["traced"], what


def test_depth_limit_of_an_upload(eng):
    """Depth 15 is accepted and reported; depth 16 is ATR_E_TREE_DEPTH, alone or beside a brute-force
    model, and the scene uploaded before stays as it was."""
    upload(eng, "d15")
    assert eng.scene_info()["max_depth"] == epart("d15")[1].stats()["depth"] == 15
    cam = E.camera(IMG_W, IMG_H, SPP, BOUNCES, **inside_camera("d15"))
    before = run(eng, cam)
    same_render(before, ref("d15", "inside", SPP, BOUNCES), "before")
    assert epart("d16")[1].stats()["depth"] == 16
    brute = epart("d8")[:1] + (None,) + epart("d8")[2:]
    for models in ([epart("d16") + (1,)], [brute + (1,), epart("d16") + (1,)]):
        with pytest.raises(E.AtrError, match="ATR_E_TREE_DEPTH"):
            eng.upload([SKY, MODEL], models)
        assert eng.scene_info()["max_depth"] == 15
        assert_unchanged(eng, cam, before, len(models))


def test_tree_layout_error_through_the_api(eng):
    """A child's bound one ulp off its parent's split point: from_nodes takes the tree (it checks
    the indices only), the upload reports ATR_E_TREE_LAYOUT and leaves the scene in place."""
    upload(eng, "d9")
    cam = E.camera(IMG_W, IMG_H, SPP, BOUNCES, **inside_camera("d9"))
    before = run(eng, cam)
    same_render(before, ref("d9", "inside", SPP, BOUNCES), "before")
    bounds, children, first, count, verts, face = (np.array(a) for a in exported("d9"))
    node, depth, _ = D.deepest_inner(bounds, children)
    assert depth == 8
    kid = children[node] + 5
    bounds[kid, 3] = np.nextafter(bounds[kid, 3], F(np.inf))
    bad = E.Octree.from_nodes(bounds, children, first, count, verts, face)
    assert bad.stats()["depth"] == 9
    m, _, box = epart("d9")
    with pytest.raises(E.AtrError, match="ATR_E_TREE_LAYOUT"):
        eng.upload([SKY, MODEL], [(m, bad, box, 1)])
    assert_unchanged(eng, cam, before, "layout")


# ---- 7. the device build -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["d15", "d16", "wide"])
def test_device_build_bit_identical_at_depth(name):
    m, t, _ = epart(name)
    _same(E.Octree.build_device(m, D.leaf_size(name)), t)
