"""Spheres and planes at their edges in every kernel that reads them, on the GPU: the scenes, batches
and point sets of tests/analytic_scenes.py (duplicates, nested and touching spheres, r = 0, r < 0,
centres at 1e30 and NaN, zero, NaN and non-unit plane normals, exact ties with each other and with a
model, 70 spheres, 40 planes, tangent rays and plane denominators stepped in ulps across their
edges). atr_trace_rays against the numpy-float32 reference of tests/analytic_ref.py (pinned to the
oracle, with the coverage of these inputs, in tests/test_analytic_cpu.py); atr_occluded_rays with
t_max at, one ulp above and one ulp below the closest hit; the two gathers and the radiance query
against their references; renders from eyes inside spheres and on a plane, and on the scene boxes a
degenerate sphere list leaves the queue sort, against the oracle. Every comparison is for equal bits;
rendered rgb goes through test_gpu_parity.assert_rgb. Needs an MI355X (-m gpu)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from tests import analytic_ref as A  # noqa: E402
from tests import analytic_scenes as S  # noqa: E402
from tests import gather_radiance_ref as GRR  # noqa: E402
from tests import gather_ref as GR  # noqa: E402
from tests import occlusion_ref as OR  # noqa: E402
from tests import radiance_ref as RR  # noqa: E402
from tests import ray_sets as R  # noqa: E402
from tests import test_gpu_gather as TG  # noqa: E402
from tests import test_gpu_gather_radiance as TGR  # noqa: E402
from tests import test_gpu_occlusion as TO  # noqa: E402
from tests import test_gpu_radiance as TRA  # noqa: E402
from tests import test_gpu_trace_rays as TR  # noqa: E402
from tests.test_gpu_parity import eng, run  # noqa: E402,F401
from tests.test_gpu_scenes import ALL, ref, same as same_render  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
VARIANTS = (E.ATR_KERNEL_AUTO, E.ATR_KERNEL_LANE)
RENDERS = ((1, 1), (2, 5))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_hits(res, w, what):
    """Every output of atr_trace_rays against the reference record, bit for bit (NaN matches NaN)."""
    for k in ("t", "uv", "normal"):
        bad = np.flatnonzero((bits(res[k]) != bits(w[k])).reshape(len(w[k]), -1).any(axis=1))
        assert len(bad) == 0, (what, k, len(bad), bad[:5].tolist(), res[k][bad[:5]].tolist(), w[k][bad[:5]].tolist(),
                               w["kind"][bad[:5]].tolist(), w["index"][bad[:5]].tolist())
    for k in ("face", "model", "kind", "material"):
        bad = np.flatnonzero(res[k] != w[k])
        assert len(bad) == 0, (what, k, len(bad), bad[:5].tolist(), res[k][bad[:5]].tolist(), w[k][bad[:5]].tolist(),
                               w["index"][bad[:5]].tolist())
    assert res["traced"] == len(w["t"]), (what, res["traced"])


# ---- 1. the closest hit -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(S.SCENES))
def test_trace_rays_match_the_reference(eng, name):
    sc = S.SCENES[name]
    sc.upload(eng)
    for n, kind in S.BATCHES:
        if n != name:
            continue
        o, d = S.batch(name, kind)
        w = S.reference(name, kind)
        want = sc.oracle().trace(o, d)[:3] if sc.names else None
        for variant in VARIANTS:
            for sb in (0, 5):
                res = TR.query(eng, o, d, variant, sb)
                assert_hits(res, w, (name, kind, variant, sb))
                if want is not None:  # t, face and uv against the oracle itself
                    TR.assert_parity(res, want, (name, kind, variant, sb, "oracle"))


# ---- 2. the occlusion bound ----------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["edge", "edge_model_tree", "edge_model_bf"])
def test_occluded_rays_around_the_closest_hit(eng, name):
    """kTol < t < T with T the closest hit's t, one ulp above it, one ulp below it, and unbounded."""
    sc = S.SCENES[name]
    sc.upload(eng)
    for kind in S.EDGE_KINDS:
        o, d = S.batch(name, kind)
        t = S.reference(name, kind)["t"]
        hit = (t < R.MAX_FLOAT).astype(np.uint8)
        for which in ("t", "up", "down", "null"):
            tm = None if which == "null" else np.array(t, F) if which == "t" else S.tmax(t, which)
            w = OR.occluded(sc.oracle(), o, d, tm)
            # no ray is occluded by its own closest hit; one ulp on, every ray that hits is
            assert np.array_equal(w, hit if which in ("up", "null") else np.zeros_like(hit)), (name, kind, which)
            for variant in VARIANTS:
                for sb in (0, 5):
                    got, traced = TO.occl(eng, o, d, tm, variant, sb)
                    TO.same(got, w, (name, kind, which, variant, sb))
                    assert traced == len(o)


# ---- 3. the gathers and the paths -------------------------------------------------------------------------

def test_gather_occlusion_on_sphere_and_plane_points(eng):
    S.EDGE.upload(eng)
    p, n = S.points()
    first, base, seed = S.GATHER_ARGS
    for tm in (None, np.full(len(p), S.GATHER_TMAX, F)):
        w = GR.gather(S.EDGE.oracle(), p, n, S.GATHER_NS, tm, first, base, seed)
        for variant in VARIANTS:
            got = TG.gather(eng, p, n, S.GATHER_NS, tm, variant, first, base, seed)
            TG.same(got, w, ("edge", tm is None, variant))


def test_radiance_rays_on_bounce_rays(eng):
    S.EDGE.upload(eng)
    o, d = (a[:256] for a in S.batch("edge", "second"))
    ns, bl = S.PATHS
    w = RR.radiance(S.EDGE.oracle(), o, d, ns, bl, S.SEED)
    for sb in (0, 5):
        TRA.same(TRA.radiance(eng, o, d, ns, bl, seed=S.SEED, sort_bits=sb), w, ("edge", sb))


def test_gather_radiance_on_sphere_and_plane_points(eng):
    S.EDGE.upload(eng)
    p, n = S.points()
    ns, bl = S.PATHS
    w = GRR.gather_radiance(S.EDGE.oracle(), p, n, ns, bl, S.SEED)
    for sb in (0, 5):
        TGR.same(TGR.gather(eng, p, n, ns, bl, seed=S.SEED, sort_bits=sb), w, ("edge", sb))


# ---- 4. the renders ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ALL)
@pytest.mark.parametrize("name", ["edge", "edge_model_tree", "edge_model_bf", "many_spheres"])
def test_renders_match_the_oracle(eng, name, variant):
    """The app's eye, an eye inside sphere 3, one inside the radius-50 sphere and one on the plane y = 0."""
    sc = S.SCENES[name]
    sc.upload(eng)
    for cam in S.CAMERAS.values():
        for spp, bounces in RENDERS:
            same_render(run(eng, E.camera(S.RW, S.RH, spp, bounces, **cam), variant=variant),
                        ref(sc, S.RW, S.RH, spp, bounces, **cam), (name, variant, spp, bounces, cam))


# ---- 5. the scene box ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(S.BOXES))
def test_scene_boxes_of_degenerate_sphere_lists(eng, name):
    """The queue sort's origin cells span the box atr_scene_upload builds from the spheres' bounds: a
    sorted query and the renders (PATHS sorts its queues) on a zero-extent box, on a scene with
    nothing bounded, on bounds that overflow to inf and on EDGE's NaN and 1e30 centres."""
    sc = S.BOXES[name]
    sc.upload(eng)
    o, d = S.batch("edge", "second")
    w = A.closest(sc.spheres, sc.planes, o, d)
    want = sc.oracle().trace(o, d)[:3]
    assert np.array_equal(bits(w["t"]), bits(want[1]))
    for sb in (2, 5, 7):
        res = TR.query(eng, o, d, E.ATR_KERNEL_AUTO, sb)
        TR.assert_parity(res, want, (name, sb))
        for k in ("kind", "material"):
            assert np.array_equal(res[k], w[k]), (name, sb, k)
        assert np.array_equal(bits(res["normal"]), bits(w["normal"])), (name, sb)
    if name == "edge":
        return  # rendered above
    for variant in ALL:
        for cam in S.CAMERAS.values():
            for spp, bounces in RENDERS:
                same_render(run(eng, E.camera(S.RW, S.RH, spp, bounces, **cam), variant=variant),
                            ref(sc, S.RW, S.RH, spp, bounces, **cam), (name, variant, spp, bounces, cam))
