"""Every kernel on geometry far from unit scale and from the origin (tests/scale_scenes.py; the regimes
are pinned on the oracle by tests/test_scale_cpu.py): the Monkey from 2^-5 (|ab x ac| below the
tolerance) to 2^20, moved up to 2^20 from the origin, the Cube and the Monkey at 2^34 .. 2^63 (det >=
2^64 takes recip_det's IEEE branch; P, q and the box growths become inf or NaN; then the reference's
own products overflow and nothing hits), ray origins 2^8 .. 2^23 box diagonals away, and one mesh that
mixes sizes over seven orders of magnitude. Renders of every variant, the fold, cull and pads switches
in two contexts each, the row of the growth table, atr_trace_rays, atr_occluded_rays one ulp around
each hit, the two gathers, atr_radiance_rays and the device tree build: all against the oracle (or
the host build) for equal bits; rendered rgb goes through test_gpu_parity.assert_rgb. Needs an MI355X
(-m gpu)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from tests import analytic_scenes as AS  # noqa: E402
from tests import gather_radiance_ref as GRR  # noqa: E402
from tests import gather_ref as GR  # noqa: E402
from tests import occlusion_ref as OR  # noqa: E402
from tests import radiance_ref as RR  # noqa: E402
from tests import ray_sets as R  # noqa: E402
from tests import scale_scenes as S  # noqa: E402
from tests import test_gpu_camera_pads as CP  # noqa: E402
from tests import test_gpu_facing_fold as FF  # noqa: E402
from tests import test_gpu_gather as TG  # noqa: E402
from tests import test_gpu_gather_radiance as TGR  # noqa: E402
from tests import test_gpu_occlusion as TO  # noqa: E402
from tests import test_gpu_radiance as TRA  # noqa: E402
from tests import test_gpu_trace_rays as TR  # noqa: E402
from tests import test_gpu_wave_cull as WC  # noqa: E402
from tests.goldens import SEED  # noqa: E402
from tests.test_gpu_build import _same as same_build  # noqa: E402
from tests.test_gpu_camera_pads import pair as pads_pair  # noqa: E402,F401
from tests.test_gpu_facing_fold import pair as fold_pair  # noqa: E402,F401
from tests.test_gpu_parity import MODEL, SKY, eng, run  # noqa: E402,F401
from tests.test_gpu_scenes import ALL, check  # noqa: E402
from tests.test_gpu_wave_cull import pair as cull_pair  # noqa: E402,F401

pytestmark = pytest.mark.gpu
F = np.float32
VARIANTS = (E.ATR_KERNEL_AUTO, E.ATR_KERNEL_LANE)
SORTS = (0, 5)
NS, BOUNCES = 16, 3


def ids(keys):
    return [S.key_id(k) for k in keys]


# ---- 1. renders ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ALL)
@pytest.mark.parametrize("key", S.RENDERED, ids=ids(S.RENDERED))
def test_renders_match_the_oracle(eng, key, variant):
    """LANE, FLAT, HYBRID (pads table, fold and wave cull at their defaults), PATHS with its bounce
    flavours, and AUTO; the Cube at 2^34 is the frame whose every primary direction is NaN."""
    sc = S.scene(*key)
    sc.upload(eng)
    check(eng, sc, variant, S.RW, S.RH, renders=((1, 1), (2, 3)), **sc.cam)


# ---- 2. the fold, cull and pads switches ---------------------------------------------------------------

def plain(key):
    """A switched scene as the two-context tests upload it ([SKY, MODEL], the model's material 1):
    (its name, the engine's model tuple, the composed oracle scene, the scene)."""
    sc = S.scene(*key)
    p = AS.TextSc(sc.text, True, sc.leaf, 1, [SKY, MODEL])
    return S.key_id(key), p.models()[0], p.oracle(), sc


def fold_upload(pair, key):
    """The scene in both contexts of a pair, as test_gpu_facing_fold uploads its own (cluster size 16)."""
    name, md, s, sc = plain(key)
    for e in pair:
        e.set_tuning(cluster_size=16)
        e.upload([SKY, MODEL], [md])
    return name, s, sc


@pytest.mark.parametrize("key", S.SWITCHED, ids=ids(S.SWITCHED))
def test_fold_on_equals_fold_off_and_the_oracle(fold_pair, key):
    name, s, sc = fold_upload(fold_pair, key)
    want = FF.oracle_frame(s, (name, sc.leaf), S.RW, S.RH, sc.cam["eye"], sc.cam["facing"])
    FF.both_equal_the_oracle(fold_pair, want, E.camera(S.RW, S.RH, **sc.cam), name)


@pytest.mark.parametrize("key", S.SWITCHED, ids=ids(S.SWITCHED))
def test_growth_table_row_obeys_the_bound(fold_pair, key):
    """atr_camera_pads_row entry by entry against cluster_grow's pair and the float64 bound
    (test_gpu_facing_fold.row_obeys_the_bound). The loose growth is W (36 eps P / (0.9 kTol) + 12 eps): it
    grows with the cube of the scale and with the distance from the origin, the boxes with the scale
    alone, so far out every grown box holds the eye, no cone of rays is left to bound det over and no
    cluster may fold (delta = kTol in every entry). Only then is the row not asked for a folded cluster."""
    name, _, sc = fold_upload(fold_pair, key)
    row, boxes, _ = fold_pair[1].camera_pads_row(sc.cam["eye"])
    eye = np.asarray(F(sc.cam["eye"]), np.float64)
    g = boxes[:, 8].astype(np.float64)[:, None]
    inside = ((boxes[:, 0:3] - g <= eye) & (eye <= boxes[:, 4:7] + g)).all(axis=1)
    print(name, "clusters", len(row), "whose grown box holds the eye", int(inside.sum()))
    assert (row[inside, 2] == F(FF.K_TOL)).all()
    FF.row_obeys_the_bound(fold_pair, name, sc.cam["eye"], must_fold=not inside.all())


def two_contexts(pair, same, key, deals=((2, 0),)):
    """HYBRID and FLAT, whole and as a PACKED render of two halves, in a context with the switch off and
    one with it on: equal to each other and to the oracle's hits."""
    off, on = pair
    name, md, s, sc = plain(key)
    W, H = S.RW, S.RH
    face_o, t_o = S.frame_hits(sc)
    cam = E.camera(W, H, **sc.cam)
    halves = [[0, 0, W // 2 - 1, H - 1], [W // 2, 0, W - 1, H - 1]]
    base = on.tuning()
    try:
        for e in pair:
            e.set_tuning(cluster_size=16)
            e.upload([SKY, MODEL], [md])
        for a, b in deals:
            for e in pair:
                e.set_tuning(hybrid_a=a, hybrid_b=b)
            for variant in (E.ATR_KERNEL_HYBRID, E.ATR_KERNEL_FLAT):
                x, y = run(off, cam, variant=variant), run(on, cam, variant=variant)
                same(x, y, (name, a, b, variant))
                assert np.array_equal(y["face"], face_o), (name, a, b, variant, int((y["face"] != face_o).sum()))
                assert np.array_equal(y["t"].view(np.uint32), t_o.view(np.uint32)), (name, a, b, variant)
                same(run(off, cam, tiles=halves, layout=E.ATR_LAYOUT_PACKED, variant=variant),
                     run(on, cam, tiles=halves, layout=E.ATR_LAYOUT_PACKED, variant=variant), (name, a, b, variant, "PACKED"))
        return off, on, cam
    finally:
        for e in pair:
            e.set_tuning(**base)


@pytest.mark.parametrize("key", S.SWITCHED, ids=ids(S.SWITCHED))
def test_cull_on_equals_cull_off_and_the_oracle(cull_pair, key):
    """ATR_WAVE_CULL=0 against unset, under the three deal rules of a leaf step."""
    off, on, cam = two_contexts(cull_pair, WC.same, key, deals=tuple(WC.DEAL.values()))
    whole = [[0, 0, S.RW - 1, S.RH - 1]]
    ca, cb = (e.counters(cam, whole, SEED, E.ATR_KERNEL_HYBRID) for e in (off, on))
    for k in ("n_rays", "n_box", "n_leaf"):
        assert ca[k] == cb[k], (key, k, ca, cb)


@pytest.mark.parametrize("key", S.SWITCHED, ids=ids(S.SWITCHED))
def test_table_on_equals_table_off_and_the_oracle(pads_pair, key):
    """ATR_CAMERA_PADS=0 (the growths computed per ray) against the table: the outputs and every work
    counter."""
    off, on, cam = two_contexts(pads_pair, CP.same, key)
    whole = [[0, 0, S.RW - 1, S.RH - 1]]
    ca, cb = (e.counters(cam, whole, SEED, E.ATR_KERNEL_HYBRID) for e in (off, on))
    assert ca == cb, (key, ca, cb)


# ---- 3. atr_trace_rays ---------------------------------------------------------------------------------

@pytest.mark.parametrize("key", S.KEYS, ids=ids(S.KEYS))
def test_trace_rays_match_the_oracle(eng, key):
    """t, face and uv bits of every batch; the rows whose origins overflowed come back invalid and
    untraced, between the valid ones."""
    sc = S.scene(*key)
    sc.upload(eng)
    for kind in S.kinds(sc):
        o, d = S.raw_batch(sc, kind)
        if len(o) == 0:
            continue
        ok = R.passes(o, d)
        vo, vd = S.batch(sc, kind)
        # the oracle's record of the valid rows; the invalid record (a miss) in the others
        want = (np.full(len(o), R.MISS, np.uint32), np.full(len(o), R.MAX_FLOAT, F), np.zeros((len(o), 2), F))
        if len(vo):
            for full, part in zip(want, S.trace(sc, kind, vo, vd)):
                full[ok] = part
        for variant in VARIANTS:
            for sb in SORTS:
                what = (S.key_id(key), kind, variant, sb)
                res = TR.query(eng, o, d, variant, sb)
                assert res["traced"] == int(ok.sum()), (what, res["traced"], int(ok.sum()))
                TR.assert_parity(res, want, what)
                assert (res["kind"][~ok] == E.ATR_RAY_INVALID).all() and (res["kind"][ok] != E.ATR_RAY_INVALID).all(), what
                assert (TR.bits(res["normal"][~ok]) == 0).all() and (res["model"][~ok] == -1).all(), what


# ---- 4. atr_occluded_rays ------------------------------------------------------------------------------

@pytest.mark.parametrize("key", S.KEYS, ids=ids(S.KEYS))
def test_occluded_rays_one_ulp_around_each_hit(eng, key):
    """t_max one ulp above each oracle hit: occluded. One ulp below: what tests/occlusion_ref.py gives
    (another surface below the bound may still occlude). Invalid rows come back as ATR_OCCL_INVALID."""
    sc = S.scene(*key)
    sc.upload(eng)
    for kind in S.kinds(sc):
        o, d = S.raw_batch(sc, kind)
        if len(o) == 0:
            continue
        ok = R.passes(o, d)
        vo, vd = S.batch(sc, kind)
        t = S.trace(sc, kind, vo, vd)[1] if len(vo) else np.zeros(0, F)
        for which in ("up", "down"):
            tv = AS.tmax(t, which)
            w = np.full(len(o), E.ATR_OCCL_INVALID, np.uint8)
            if len(vo):
                w[ok] = OR.occluded(sc.oracle(), vo, vd, tv)
                if which == "up":
                    assert np.array_equal(w[ok], (t < R.MAX_FLOAT).astype(np.uint8)), (S.key_id(key), kind)
            tm = np.full(len(o), R.MAX_FLOAT, F)
            tm[ok] = tv
            for variant in VARIANTS:
                for sb in SORTS:
                    got, traced = TO.occl(eng, o, d, tm, variant, sb)
                    TO.same(got, w, (S.key_id(key), kind, which, variant, sb))
                    assert traced == int(ok.sum()), (S.key_id(key), kind, which, variant, sb, traced)


# ---- 5. the gathers and the paths ------------------------------------------------------------------------

@pytest.mark.parametrize("key", S.GATHERED, ids=ids(S.GATHERED))
def test_gather_occlusion_matches_the_reference(eng, key):
    sc = S.scene(*key)
    sc.upload(eng)
    p, n = S.points(sc)
    diag = float(np.sqrt(R.len2((sc.box()[3:] - sc.box()[:3])[None]))[0])
    for tm in (None, np.full(len(p), F(0.25 * diag), F)):
        w = GR.gather(sc.oracle(), p, n, NS, tm, TG.FIRST, TG.BASE, SEED)
        assert w["traced"] > 0
        for variant in VARIANTS:
            TG.same(TG.gather(eng, p, n, NS, tm, variant, TG.FIRST, TG.BASE, SEED), w, (S.key_id(key), tm is None, variant))


@pytest.mark.parametrize("key", S.GATHERED, ids=ids(S.GATHERED))
def test_radiance_rays_match_the_reference(eng, key):
    sc = S.scene(*key)
    sc.upload(eng)
    o, d, _ = S.hit_rays(sc)
    w = RR.radiance(sc.oracle(), o, d, NS, BOUNCES, SEED)
    for sb in SORTS:
        TRA.same(TRA.radiance(eng, o, d, NS, BOUNCES, seed=SEED, sort_bits=sb), w, (S.key_id(key), sb))


@pytest.mark.parametrize("key", S.GATHERED, ids=ids(S.GATHERED))
def test_gather_radiance_matches_the_reference(eng, key):
    sc = S.scene(*key)
    sc.upload(eng)
    p, n = S.points(sc)
    w = GRR.gather_radiance(sc.oracle(), p, n, NS, BOUNCES, SEED)
    for sb in SORTS:
        TGR.same(TGR.gather(eng, p, n, NS, BOUNCES, seed=SEED, sort_bits=sb), w, (S.key_id(key), sb))


# ---- 6. the device tree build ----------------------------------------------------------------------------

@pytest.mark.parametrize("key", S.KEYS, ids=ids(S.KEYS))
def test_device_build_bit_identical(key):
    """An area sum that overflows (s >= 2^41), NaN split points, vertices collapsed onto a lattice."""
    sc = S.scene(*key)
    m, tree, _, _ = sc.models()[0]
    same_build(E.Octree.build_device(m, sc.leaf), tree)
