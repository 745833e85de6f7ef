"""The sphere-and-plane edge tests without a GPU: the numpy-float32 reference of
tests/analytic_ref.py against the unchanged oracle, in the bits of t, on every scene and batch of
tests/test_gpu_analytic.py (tests/analytic_scenes.py), and the coverage conditions of those inputs,
asserted on the reference alone, so that no GPU comparison can pass vacuously: which primitive wins
and which never does, a plane accepted after a farther sphere, origins inside spheres, the tangent
and denominator families on both sides of their edges, the exact ties, sky rays, the occlusion
bound one ulp either side of the closest hit, and what the renders' cameras see."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import analytic_ref as A  # noqa: E402
from tests import analytic_scenes as S  # noqa: E402
from tests import gather_radiance_ref as GRR  # noqa: E402
from tests import gather_ref as GR  # noqa: E402
from tests import occlusion_ref as OR  # noqa: E402
from tests import radiance_ref as RR  # noqa: E402
from tests import ray_sets as R  # noqa: E402

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def wins(w, kind, index):
    return int(((w["kind"] == kind) & (w["index"] == index)).sum())


# ---- the reference against the oracle ---------------------------------------------------------------

def test_constants_are_the_engines():
    assert (A.SKY, A.TRI, A.SPHERE, A.PLANE) == (E.ATR_RAY_SKY, E.ATR_RAY_TRI, E.ATR_RAY_SPHERE, E.ATR_RAY_PLANE)
    assert bits(A.MAX_FLOAT) == bits(R.MAX_FLOAT) and A.TOL == F(1e-4)
    assert len(S.MATS10) >= 8 and len({m[0] for m in S.MATS10}) == len(S.MATS10)  # distinct emissions
    assert len(S.EDGE_SPHERES) == 11 and len(S.EDGE_PLANES) == 8
    assert len(S.MANY_SPHERES.spheres) == 70 and len(S.MANY_PLANES.planes) == 40
    stats = S.EDGE_MODEL["tree"].parts()[0].tree_stats()
    assert stats["inner"] == 1 and stats["max_leaf"] == 2 and S.EDGE_MODEL["bf"].parts()[0].tree is None
    sizes = [len(S.batch(n, k)[0]) for n, k in S.BATCHES]
    assert max(sizes) <= 4100 and any(s % 64 for s in sizes)


@pytest.mark.parametrize("name,kind", S.BATCHES)
def test_reference_equals_the_oracle(name, kind):
    o, d = S.batch(name, kind)
    w = S.reference(name, kind)
    face, t, uv, _ = S.SCENES[name].oracle().trace(o, d)
    bad = np.flatnonzero(bits(t) != bits(w["t"]))
    assert len(bad) == 0, (len(bad), bad[:5].tolist(), t[bad[:5]], w["t"][bad[:5]])
    analytic = (w["kind"] == A.SPHERE) | (w["kind"] == A.PLANE)
    assert (face[analytic] == R.MISS).all()
    assert np.array_equal(face, w["face"]) and np.array_equal(bits(uv), bits(w["uv"]))
    assert np.array_equal(w["kind"] == A.SKY, t == R.MAX_FLOAT)
    assert not np.isnan(w["t"]).any() and not np.isnan(w["normal"]).any()  # no degenerate primitive wins


@pytest.mark.parametrize("cam", list(S.CAMERAS))
def test_reference_equals_the_oracles_primary_hits(cam):
    """The renders' primary rays (E.camera_rays, host code) through the reference: the oracle's hit_t."""
    co, cd = E.camera_rays(E.camera(S.RW, S.RH, **S.CAMERAS[cam]))
    w = A.closest(S.EDGE_SPHERES, S.EDGE_PLANES, co, cd)
    _, t, _ = S.EDGE.oracle().primary_hits(O.Camera(S.RW, S.RH, **S.CAMERAS[cam]))
    assert np.array_equal(bits(w["t"]), bits(t.reshape(-1)))
    sph = np.bincount(w["index"][w["kind"] == A.SPHERE], minlength=11)
    pl = np.bincount(w["index"][w["kind"] == A.PLANE], minlength=8)
    if cam == "in_sphere":  # the eye is inside sphere 3: it, the nested sphere 2 and the floor through it
        assert A.inside(S.CAMERAS[cam]["eye"], *S.EDGE_SPHERES[3][:2]) and sph[3] >= 500 and sph[2] >= 50
    elif cam == "in_big":
        assert A.inside(S.CAMERAS[cam]["eye"], *S.EDGE_SPHERES[S.BIG][:2]) and sph[S.BIG] >= 500
    elif cam == "on_plane":  # the eye's own plane y = 0 is never hit from it: the floor below shows
        assert S.CAMERAS[cam]["eye"][1] == 0.0 and pl[2] == 0 and pl[0] >= 500
    else:
        assert (sph[[0, 3, 4, 6, S.BIG]] >= 20).all() and pl[2] >= 500


# ---- the coverage conditions ---------------------------------------------------------------------------

def test_every_sound_primitive_wins_and_no_other_does():
    w = S.reference("edge", "aimed")
    for i in S.SPHERE_WINS:
        assert wins(w, A.SPHERE, i) >= 20, (i, wins(w, A.SPHERE, i))
    for i in S.PLANE_WINS:
        assert wins(w, A.PLANE, i) >= 20, (i, wins(w, A.PLANE, i))
    for name, kind in S.BATCHES[:12]:  # EDGE and both model scenes
        w = S.reference(name, kind)
        for i in S.SPHERE_NEVER:
            assert wins(w, A.SPHERE, i) == 0 and not (w["ns"] == i).any(), (name, kind, i)
        for i in S.PLANE_NEVER:
            assert wins(w, A.PLANE, i) == 0 and not (w["np"] == i).any(), (name, kind, i)
    assert S.EDGE_SPHERES[0][:2] == S.EDGE_SPHERES[1][:2] and S.EDGE_SPHERES[0][2] != S.EDGE_SPHERES[1][2]
    assert S.EDGE_PLANES[0][:2] == S.EDGE_PLANES[1][:2] and S.EDGE_PLANES[0][2] != S.EDGE_PLANES[1][2]


def test_a_plane_takes_the_hit_from_an_accepted_sphere():
    w = S.reference("edge", "aimed")
    both = (w["ns"] >= 0) & (w["np"] >= 0)
    assert int(both.sum()) >= 200 and (w["kind"][both] == A.PLANE).all()
    wm = S.reference("edge_model_tree", "aimed")
    tri = wm["kind"] == A.TRI
    hidden = (wm["model_t"] < R.MAX_FLOAT) & ~tri  # a model hit that a sphere or plane takes over
    assert int(tri.sum()) >= 100 and int(hidden.sum()) >= 20


def test_origins_inside_spheres_take_the_far_root():
    o, d = S.batch("edge", "inside")
    w = S.reference("edge", "inside")
    n = 0
    for i in S.SPHERE_WINS:
        c, r, _ = S.EDGE_SPHERES[i]
        won = (w["kind"] == A.SPHERE) & (w["index"] == i) & A.inside(o, c, r)
        _, ta, tb = A.sphere_t64(o[won], d[won], c, r)
        assert (tb < 0).all() and (ta > 0).all()
        n += int(won.sum())
    assert n >= 100, n
    # bounce rays start on the surface: the near root is within rounding of 0 and is not taken
    o, d = S.batch("edge", "second")
    w = S.reference("edge", "second")
    on = np.zeros(len(o), bool)
    for i in S.SPHERE_WINS:
        c, r, _ = S.EDGE_SPHERES[i]
        _, ta, tb = A.sphere_t64(o, d, c, r)
        on |= (np.abs(tb) < 1e-4 * abs(r)) & (ta > 1e-3)
    assert int(on.sum()) >= 100, int(on.sum())


def test_tangent_family_hits_and_misses():
    o, d = S.batch("edge", "special")
    w = S.reference("edge", "special")
    c, r, _ = S.EDGE_SPHERES[S.TANGENT_SPHERE]
    hit = (w["kind"][S.TANGENT] == A.SPHERE) & (w["index"][S.TANGENT] == S.TANGENT_SPHERE)
    assert 5 <= int(hit.sum()) <= 60, int(hit.sum())
    dmt, _, _ = A.sphere_t64(o[S.TANGENT], d[S.TANGENT], c, r)
    assert (dmt > 0).any() and (dmt < 0).any() and (np.abs(dmt) < 1e-4).all()  # grazing, either side
    assert hit[dmt >= 0].all()  # the f32 discriminant rounds a few of the outer ones to a hit as well
    assert (w["kind"][S.TANGENT][~hit] == A.SPHERE).all()  # the others go on to spheres 4 and 3


def test_denominator_family_straddles_the_tolerance():
    o, d = S.batch("edge", "special")
    w = S.reference("edge", "special")
    n, dist, _ = S.EDGE_PLANES[S.DENOM_PLANE]
    hit = (w["kind"][S.DENOM] == A.PLANE) & (w["index"][S.DENOM] == S.DENOM_PLANE)
    assert (w["kind"][S.DENOM][~hit] == A.SKY).all()  # nothing else is in the way
    denom = A.dot(np.broadcast_to(np.asarray(n, F), (130, 3)), d[S.DENOM])
    assert np.array_equal(denom, d[S.DENOM][:, 0])  # exactly d.x
    for side, rows in ((1.0, slice(0, 65)), (-1.0, slice(65, 130))):
        den, h = denom[rows] * F(side), hit[rows]
        assert int((den < A.TOL).sum()) == 32 and int((den == A.TOL).sum()) == 1 and int((den > A.TOL).sum()) == 32
        assert not h[den < A.TOL].any() and h[den >= A.TOL].all()  # the bound itself is outside the open interval


def test_exact_ties():
    o, d = (a[S.TIES] for a in S.batch("edge", "special"))
    two = bits(F(2.0))
    ts = A.sphere_t(o, d, *S.EDGE_SPHERES[0][:2])
    tp = A.plane_t(o, d, *S.EDGE_PLANES[0][:2])
    w = S.reference("edge", "special")
    kind, index, t = w["kind"][S.TIES], w["index"][S.TIES], w["t"][S.TIES]
    # ray 0: sphere 0 and planes 0, 1 at t = 2: the sphere, found first, keeps the hit
    assert bits(ts[0]) == two and bits(tp[0]) == two and (kind[0], index[0]) == (A.SPHERE, 0)
    # rays 1 .. 3: the duplicate planes alone: the first
    assert (bits(tp[1:4]) == two).all() and (kind[1:4] == A.PLANE).all() and (index[1:4] == 0).all()
    # ray 4: sphere 4 against the planes
    assert bits(A.sphere_t(o, d, *S.EDGE_SPHERES[4][:2])[4]) == two and bits(tp[4]) == two
    assert (kind[4], index[4]) == (A.SPHERE, 4)
    # ray 6 enters sphere 0 at its contact point with sphere 4: the duplicate pair from inside, the first
    assert (kind[6], index[6]) == (A.SPHERE, 0) and bits(t[6]) == two
    for name in ("edge_model_tree", "edge_model_bf"):
        wm = S.reference(name, "special")
        # rays 0 .. 2: the quad at t = 2 as well: the model, found first, keeps the hit
        assert (bits(wm["model_t"][S.TIES][:3]) == two).all() and (bits(wm["t"][S.TIES][:3]) == two).all()
        assert (wm["kind"][S.TIES][:3] == A.TRI).all() and (wm["kind"][S.TIES][3] == A.PLANE)
        assert wm["model_t"][S.TIES][3] == R.MAX_FLOAT


def test_sky_rays_remain():
    assert int((S.reference("edge", "special")["kind"] == A.SKY).sum()) >= 20
    assert int((S.reference("edge", "second")["kind"] == A.SKY).sum()) >= 20
    assert int((S.reference("many_spheres", "aimed")["kind"] == A.SKY).sum()) >= 20


def test_long_loops_are_used():
    w = S.reference("many_spheres", "aimed")
    assert int((w["index"] >= 64).sum()) >= 10 and len(np.unique(w["index"])) >= 50
    w = S.reference("many_planes", "aimed")
    assert len(np.unique(w["index"])) >= 30 and int((w["index"] >= 32).sum()) >= 50


# ---- the occlusion bound -------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["edge", "edge_model_tree", "edge_model_bf"])
@pytest.mark.parametrize("kind", S.EDGE_KINDS)
def test_occlusion_bound_around_the_closest_hit(name, kind):
    """kTol < t < T: at T = t no ray is occluded, its own closest hit included; one ulp above every ray
    that hits is; one ulp below none is."""
    o, d = S.batch(name, kind)
    t = S.reference(name, kind)["t"]
    s = S.SCENES[name].oracle()
    hit = t < R.MAX_FLOAT
    assert not OR.occluded(s, o, d, np.array(t, F)).any()
    assert np.array_equal(OR.occluded(s, o, d, S.tmax(t, "up")), hit.astype(np.uint8))
    assert not OR.occluded(s, o, d, S.tmax(t, "down")).any()
    assert np.array_equal(OR.occluded(s, o, d), hit.astype(np.uint8))


# ---- the gathers and the paths ---------------------------------------------------------------------------

def test_points_are_on_every_surface_and_the_references_see_both_answers():
    p, n = S.points()
    assert len(p) == 256
    c, r, _ = S.EDGE_SPHERES[S.BIG]
    on_big = np.abs(np.sqrt(((p.astype(np.float64) - np.asarray(c)) ** 2).sum(axis=1)) - r) < 1e-3
    assert int(on_big.sum()) == 32
    out = ((p.astype(np.float64) - np.asarray(c)) * n).sum(axis=1)[on_big]
    assert (out > 0).any() and (out < 0).any()  # outward and inward normals
    s = S.EDGE.oracle()
    for tm in (None, S.GATHER_TMAX):
        g = GR.gather(s, p, n, S.GATHER_NS, None if tm is None else np.full(len(p), tm, F), *S.GATHER_ARGS)
        assert g["visible"].sum() >= 100 and g["occluded"].sum() >= 100 and (g["flags"] == 0).any()
    ro, rd = (a[:256] for a in S.batch("edge", "second"))
    casts = RR.radiance(s, ro, rd, *S.PATHS, S.SEED)["sample_casts"]
    lengths = set(np.unique(casts).tolist())  # paths that leave at once, paths in between, paths that reach the limit
    assert {0, 1, S.PATHS[1]} <= lengths and len(lengths) >= 4, lengths
    gr = GRR.gather_radiance(s, p, n, *S.PATHS, S.SEED)
    traced = gr["sample_casts"][gr["flags"] == 1]
    lengths = set(np.unique(traced).tolist())
    assert {0, 1, S.PATHS[1]} <= lengths and len(lengths) >= 4 and (gr["flags"] == 0).any(), lengths
