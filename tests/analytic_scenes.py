"""The scenes, ray batches and point sets of the sphere-and-plane edge tests, shared by
tests/test_analytic_cpu.py (which pins the reference and asserts what the inputs cover) and
tests/test_gpu_analytic.py: numpy float32 throughout, fixed seeds, everything cached and read-only.

EDGE's primitives, by index.
  Spheres: 0 the unit sphere at (0, 0, -4); 1 its exact duplicate with another material; 2 a sphere
  nested in 3 (same centre); 4 touches 0 at (1, 0, -4) and overlaps 3; 5 has r = 0; 6 has r = -0.8
  (only r * r is used); 7 has its centre at 1e30 (dmt = inf - inf = NaN); 8 has a NaN centre; 9 has
  r = 1e-3; 10 has r = 50 and holds many origins.
  Planes: 0 the floor y = -1, tangent to sphere 0 at its lowest point; 1 its exact duplicate with
  another material; 2 y = 0, through the centres of spheres 0, 2, 3, 4 and 6; 3 y = -5 with the
  normal (0, 3, 0); 4 a zero normal; 5 a NaN normal; 6 a wall tilted 1e-4 off x = -8; 7 the wall
  x = 30, which the denominator family has to itself.
EDGE_MODEL adds two exactly representable quads: one in the floor y = -1 facing down, so that the
ray from (0, -3, -4) along +y meets the quad, sphere 0 and planes 0 and 1 at t = 2 exactly; one at
z = -7 facing the app camera."""
import zlib

import numpy as np

from tests import analytic_ref as A
from tests import ray_sets as R
from tests.test_gpu_scenes import MATS, Sc
from atray_amd import engine as E
from oracle import oracle as O

F = np.float32
NAN = float("nan")
MATS10 = MATS + [((0.25, 0.0, 0.3), (0.9, 0.4, 0.8), 0.0), ((0.15, 0.25, 0.05), (0.3, 0.9, 0.5), 1.0),
                 ((0.3, 0.15, 0.1), (0.85, 0.85, 0.6), 0.5)]

BIG = 10  # the radius-50 sphere
EDGE_SPHERES = [((0.0, 0.0, -4.0), 1.0, 1), ((0.0, 0.0, -4.0), 1.0, 2), ((4.0, 0.0, -4.0), 0.5, 3),
                ((4.0, 0.0, -4.0), 1.5, 4), ((2.0, 0.0, -4.0), 1.0, 5), ((0.0, 3.0, -4.0), 0.0, 6),
                ((-3.0, 0.0, -4.0), -0.8, 7), ((1e30, 0.0, 0.0), 1.0, 8), ((NAN, 0.0, -4.0), 1.0, 9),
                ((0.0, 2.5, -4.0), 1e-3, 3), ((0.0, 10.0, -80.0), 50.0, 6)]
EDGE_PLANES = [((0.0, 1.0, 0.0), -1.0, 2), ((0.0, 1.0, 0.0), -1.0, 5), ((0.0, 1.0, 0.0), 0.0, 7),
               ((0.0, 3.0, 0.0), -15.0, 8), ((0.0, 0.0, 0.0), 1.0, 9), ((NAN, 0.0, 1.0), -2.0, 1),
               ((1.0, 1e-4, 0.0), -8.0, 4), ((1.0, 0.0, 0.0), 30.0, 9)]
SPHERE_WINS = (0, 2, 3, 4, 6, 9, BIG)   # finite and non-degenerate, not a second duplicate
SPHERE_NEVER = (1, 5, 7, 8)             # the second duplicate, r = 0, the 1e30 centre, the NaN centre
PLANE_WINS = (0, 2, 3, 6, 7)
PLANE_NEVER = (1, 4, 5)                 # the second duplicate, the zero normal, the NaN normal
DENOM_PLANE, TANGENT_SPHERE = 7, 0

QUADS = """v -2.25 -1 -6.5
v 1.75 -1 -6.5
v 1.75 -1 -2.5
v -2.25 -1 -2.5
v -3 3.5 -7
v 1 3.5 -7
v 1 7.5 -7
v -3 7.5 -7
f 1 2 3
f 1 3 4
f 5 6 7
f 5 7 8
"""
MODEL_MAT = 9


class TextSc(Sc):
    """A scene whose one model comes from inline OBJ text, as it stands (no translation)."""
    _o, _e = {}, {}

    def __init__(self, text, tree, leaf, material, materials, spheres=(), planes=()):
        Sc.__init__(self, ["text:%08x:%d:%d" % (zlib.crc32(text.encode()), tree, leaf)], [material], materials, spheres,
                    planes)
        self.text, self.tree, self.leaf = text, bool(tree), int(leaf)

    def parts(self):
        key = (self.names[0], self.model_mats[0])
        if key not in self._o:
            self._o[key] = O.Scene(obj_text=self.text, center=None, max_faces=self.leaf, use_tree=self.tree,
                                   model_material=self.model_mats[0])
        return [self._o[key]]

    def models(self):
        key = self.names[0]
        if key not in self._e:
            m = E.Mesh.parse_obj(self.text)
            self._e[key] = (m, E.Octree.build(m, self.leaf) if self.tree else None, m.aabb())
        return [self._e[key] + (self.model_mats[0],)]

    def alone(self):
        """The model without the spheres and planes."""
        return TextSc(self.text, self.tree, self.leaf, self.model_mats[0], self.materials)


def _many_spheres():
    """70 small spheres on a 10 x 7 grid, in a depth order that is not the index order."""
    rng = np.random.default_rng(3)
    depth = rng.permutation(70)
    return [((-4.5 + (k % 10), -3.0 + (k // 10), -6.0 - 0.25 * float(depth[k])), 0.45, 1 + k % 9) for k in range(70)]


def _many_planes():
    """40 planes in four orientations, ten distances each, in shuffled order."""
    rng = np.random.default_rng(4)
    normals = [(0.0, 1.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.6, 0.8, 0.0)]
    order = rng.permutation(40)
    return [(normals[int(k) % 4], -2.0 - 1.5 * float(int(k) // 4), 1 + j % 9) for j, k in enumerate(order)]


EDGE = Sc([], [], MATS10, EDGE_SPHERES, EDGE_PLANES)
EDGE_MODEL = {"tree": TextSc(QUADS, True, 2, MODEL_MAT, MATS10, EDGE_SPHERES, EDGE_PLANES),
              "bf": TextSc(QUADS, False, 2, MODEL_MAT, MATS10, EDGE_SPHERES, EDGE_PLANES)}
MANY_SPHERES = Sc([], [], MATS10, _many_spheres(), [])
MANY_PLANES = Sc([], [], MATS10, [], _many_planes())
SCENES = {"edge": EDGE, "edge_model_tree": EDGE_MODEL["tree"], "edge_model_bf": EDGE_MODEL["bf"],
          "many_spheres": MANY_SPHERES, "many_planes": MANY_PLANES}
# what atr_scene_upload makes the queue sort's scene box from: zero extent (every scale 0); nothing
# bounded (the unit box); bounds that overflow to inf (the unit box); EDGE itself (a NaN centre, which
# the bounds skip, and one at 1e30, which they take)
BOXES = {"point": Sc([], [], MATS10, [((0.0, 0.0, -4.0), 0.0, 1)], []),
         "planes_only": Sc([], [], MATS10, [], EDGE_PLANES[:4]),
         "overflow": Sc([], [], MATS10, [((0.0, 0.0, -4.0), 1.0, 1), ((3e38, 0.0, 0.0), 3e38, 2)], EDGE_PLANES[:1]),
         "edge": EDGE}

# the renders' eyes: the app's; inside sphere 3 (outside sphere 2); inside the radius-50 sphere; on
# plane 2 (y = 0), looking along it
CAMERAS = {"app": {}, "in_sphere": dict(eye=(4.0, 0.25, -3.0), facing=(-1.0, -0.1, -0.4)),
           "in_big": dict(eye=(5.0, 20.0, -70.0), facing=(-0.1, -0.3, 1.0)),
           "on_plane": dict(eye=(0.5, 0.0, 1.0), facing=(0.0, 0.0, -1.0))}
RW, RH = 64, 48
SEED = 0x853C49E6748FEA9B
GATHER_NS, GATHER_TMAX, GATHER_ARGS = 16, 0.75, (3, 1000, SEED)  # samples, a radius, (first_sample, point_base, seed)
PATHS = (4, 5)  # (nsamples, bounce_limit) of the radiance queries

_rays, _refs, _points = {}, {}, {}


def sphere_box(s):
    (cx, cy, cz), r, _ = s
    r = abs(r)
    return np.array([cx - r, cy - r, cz - r, cx + r, cy + r, cz + r], F)


def edge_boxes():
    return [sphere_box(EDGE_SPHERES[i]) for i in SPHERE_WINS]


def ulps(x, k):
    """x moved by k units in the last place (float32, k of either sign)."""
    x = np.asarray(x, F)
    b = x.view(np.int32).astype(np.int64)
    b = np.where(b < 0, -(b & 0x7FFFFFFF), b) + k  # a monotone integer line through +-0
    return np.where(b < 0, (-b) | 0x80000000, b).astype(np.uint32).view(F)


def _tie_rays():
    """Exact axis rays: 0 meets the quad, sphere 0 and planes 0 and 1 at t = 2; 1 and 2 meet the quad
    and the planes there, beside the sphere; 3 meets the planes alone, beside the quad; 4 meets sphere
    4 at t = 2 in the floor plane from below as well (no quad there); 5 and 6 start on the contact
    point of spheres 0 and 4 and leave along +-x."""
    o = np.array([[0, -3, -4], [1.5, -3, -5], [-1.5, -3, -3], [3.5, -3, -8], [2, -3, -4], [1, 0, -4], [1, 0, -4]], F)
    d = np.array([[0, 1, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0], [0, 1, 0], [1, 0, 0], [-1, 0, 0]], F)
    return o, d


def _tangent_rays():
    """Along +x at z = -4, at heights r +- k ulp over the centre of sphere 0, k = 0 .. 32: 65 rays."""
    k = np.arange(-32, 33)
    o = np.zeros((len(k), 3), F)
    o[:, 0], o[:, 1], o[:, 2] = F(-5.0), ulps(np.full(len(k), 1.0, F), k), F(-4.0)
    return o, np.tile(np.array([1, 0, 0], F), (len(k), 1))


def _denominator_rays():
    """Against plane 7 (x = 30, normal (1, 0, 0), so dot(n, d) = d.x exactly): d = (+-kTol +- k ulp, 1,
    0) for k = 0 .. 32, from 1e-3 in front of the plane on the side the ray leaves towards it. 130 rays;
    the first 65 step across +kTol, the last 65 across -kTol."""
    k = np.arange(-32, 33)
    dx = np.concatenate([ulps(np.full(len(k), A.TOL, F), k), ulps(np.full(len(k), -A.TOL, F), k)])
    o = np.zeros((len(dx), 3), F)
    o[:, 0] = np.where(dx > 0, F(30.0) - F(1e-3), F(30.0) + F(1e-3))
    o[:, 1], o[:, 2] = F(5.0), F(-4.0)
    d = np.stack([dx, np.ones(len(dx), F), np.zeros(len(dx), F)], axis=1).astype(F)
    return o, d


def _sky_rays(n, seed):
    """From beyond every sphere, leaving every plane behind."""
    rng = np.random.default_rng(seed)
    o = (np.array([40.0, 70.0, 30.0], F) + rng.uniform(0.0, 5.0, (n, 3)).astype(F)).astype(F)
    return o, R.unit(rng.uniform(0.2, 1.0, (n, 3)).astype(F))


def rays(name, kind):
    """A named batch (cached, read-only): (orig, dirs). `name` is "edge" (which the model scenes share),
    "many_spheres" or "many_planes"."""
    if (name, kind) in _rays:
        return _rays[name, kind]
    if name == "many_spheres":
        o, d = R.aimed(np.array([-5.0, -3.5, -24.0, 5.0, 3.5, -5.5], F), 1031, 51)
    elif name == "many_planes":
        o, d = R.aimed(np.array([-18.0, -18.0, -18.0, 0.0, 0.0, 0.0], F), 1031, 52)
    elif kind == "aimed":  # 4095 = 7 boxes x 585
        o, d = R.aimed(edge_boxes(), 4095, 53)
    elif kind == "inside":  # origins well inside spheres 0, 2 (hence 3), 3 beside 2, 4, 6 and the big one
        rng = np.random.default_rng(54)
        parts = []
        for i, shift in ((0, 0.0), (2, 0.0), (3, 0.9), (4, 0.0), (6, 0.0), (BIG, 0.0)):
            c, r, _ = EDGE_SPHERES[i]
            u = rng.uniform(-1.0, 1.0, (128, 3)).astype(F) * F(0.25 * abs(r))
            u[:, 1] += F(shift)
            parts.append((np.asarray(c, F) + u).astype(F))
        o = np.concatenate(parts)
        d = R.random_dirs(len(o), rng)
    elif kind == "second":
        ao, ad = rays("edge", "aimed")
        o, d = R.second_generation(ao, ad, reference("edge", "aimed")["t"], 55, 2049)
    elif kind == "special":  # ties, the tangent family, the denominator family, the sky: 7 + 65 + 130 + 63
        parts = [_tie_rays(), _tangent_rays(), _denominator_rays(), _sky_rays(63, 56)]
        o, d = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    else:
        raise KeyError(kind)
    o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
    assert R.passes(o, d).all(), (name, kind)
    o.setflags(write=False)
    d.setflags(write=False)
    _rays[name, kind] = (o, d)
    return o, d


TIES, TANGENT, DENOM, SKYR = slice(0, 7), slice(7, 72), slice(72, 202), slice(202, 265)  # rows of "special"
EDGE_KINDS = ("aimed", "inside", "second", "special")
BATCHES = [("edge", k) for k in EDGE_KINDS] + [("edge_model_tree", k) for k in EDGE_KINDS] + [
    ("edge_model_bf", k) for k in EDGE_KINDS] + [("many_spheres", "aimed"), ("many_planes", "aimed")]


def tmax(t, which):
    """The occlusion bounds around a closest-hit trace: one ulp above ("up") or below ("down") each hit's
    t; MAX_FLOAT for the misses."""
    hit = t < R.MAX_FLOAT
    near = np.nextafter(np.where(hit, t, F(1.0)), F(np.inf) if which == "up" else F(0.0)).astype(F)
    return np.where(hit, near, R.MAX_FLOAT).astype(F)


def batch(name, kind):
    return rays("edge" if name.startswith("edge") else name, kind)


def reference(name, kind):
    """analytic_ref.closest of a batch on a scene (cached, read-only). On a model scene the selection is
    seeded with the oracle's trace of the model alone, and model, face, uv, material and the flat normal
    of its triangles are filled in from it."""
    if (name, kind) in _refs:
        return _refs[name, kind]
    sc = SCENES[name]
    o, d = batch(name, kind)
    if sc.names:
        part = sc.parts()[0]
        face, tm, uv, _ = sc.alone().oracle().trace(o, d)
        hit = face != R.MISS
        w = A.closest(sc.spheres, sc.planes, o, d, tm, np.where(hit, 0, -1))
        tri = w["kind"] == A.TRI
        w["model"] = np.where(tri, 0, -1).astype(np.int32)
        w["face"] = np.where(tri, face, R.MISS).astype(np.uint32)
        w["uv"] = np.where(hit[:, None], uv, F(0.0)).astype(F)  # the model's, whatever hides it later
        w["material"][tri] = sc.model_mats[0]
        V, N, FV, _ = part.mesh_arrays()
        assert len(N) == 0  # flat: cross(v0 - v1, v0 - v2), shade.h
        v0, v1, v2 = (V[FV[face[tri].astype(np.int64), k]] for k in range(3))
        a, b = v0 - v1, v0 - v2
        w["normal"][tri] = A.unit(np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                                            a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1).astype(F))
        w["model_t"] = tm
    else:
        w = A.closest(sc.spheres, sc.planes, o, d)
        w["model"] = np.full(len(o), -1, np.int32)
        w["face"] = np.full(len(o), R.MISS, np.uint32)
        w["uv"] = np.zeros((len(o), 2), F)
    for a in w.values():
        a.setflags(write=False)
    _refs[name, kind] = w
    return w


def points():
    """256 surface points of EDGE with unit normals (cached, read-only): hits of the aimed batch, 32 on
    each winning sphere (normals outward and, every other one, inward) and 16 on each of planes 0 and 2
    (the normal, every other one negated). (p, n)."""
    if "edge" not in _points:
        o, d = rays("edge", "aimed")
        w = reference("edge", "aimed")
        rows = []
        for kind, idx, cnt in [(A.SPHERE, i, 32) for i in SPHERE_WINS] + [(A.PLANE, i, 16) for i in (0, 2)]:
            r = np.flatnonzero((w["kind"] == kind) & (w["index"] == idx))
            assert len(r) >= cnt, (kind, idx, len(r))
            rows.append(r[:cnt])
        rows = np.concatenate(rows)
        assert len(rows) == 256
        p = (o[rows] + (d[rows] * w["t"][rows][:, None]).astype(F)).astype(F)
        n = np.array(w["normal"][rows], F)
        n[1::2] = -n[1::2]
        assert R.passes(p, n).all()
        p.setflags(write=False)
        n.setflags(write=False)
        _points["edge"] = (np.ascontiguousarray(p), np.ascontiguousarray(n))
    return _points["edge"]
