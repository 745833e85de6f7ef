"""Geometry far from unit scale and from the origin, shared by tests/test_scale_cpu.py (which pins
the regimes on the oracle) and tests/test_gpu_scale.py: numpy only, fixed seeds, everything cached
and read-only.

An asset's vertices are centred on the origin (its box centre subtracted in float32) and then placed
as v' = fl32(fl32(v * s) + p) with p = fl32(s * CENTERS[asset] + c); the result is written as OBJ text
with %.9g, so that the oracle and the engine parse identical floats (the TextSc pattern of
tests/analytic_scenes.py). Normals and faces are the asset's own.

Families (DESIGN.md section 2 has the hit counts the oracle gives on them):
  SCALE        the Monkey at s = 2^k, k in -5, -4, -3, -2, 6, 12, 20: from |ab x ac| around the tolerance
               kTol = 1e-4 (most faces can never be hit) to P and q twelve orders above the assets'.
  OFFSET       the Monkey at s = 1, moved by 2^12 .. 2^20: vertices on a coarse lattice, a tree whose
               split degenerates, quantised primary directions. Offsets of 2^22 and more make the
               reference's build run away (tests/test_build_runaway_cpu.py) and are not built here.
  OVERFLOW     the Cube at s = 2^34 .. 2^63 and the Monkey at 2^41 and 2^60: det >= 2^64 (the IEEE
               branch of recip_det), then products that overflow until no ray hits.
  FAR          the Monkey as the assets have it, the aimed batch's origins moved back along their own
               directions by 2^k box diagonals: the exact test's rounding picks the face.
  MIXED_SIZES  one OBJ of the Monkey, a copy at 2^-3 inside it and the Cube at 2^10 around both.
"""
import numpy as np

from atray_amd.assets import CENTERS, asset_path
from tests import ray_sets as R
from tests.analytic_scenes import TextSc
from tests.test_gpu_scenes import MATS

F = np.float32
APP_EYE, APP_FACING = (0.1, 2.0, 0.0), (-0.1, -0.5, -1.0)
LEAF = {"Monkey": 64, "Cube": 300}
MODEL_MAT = 2  # scatter 0.3: bounce rays both diffuse and mirrored
RW, RH = 64, 48
N_AIMED, N_SMALL = 2048, 1025
MIXED_LEAF = 300  # three leaves then hold faces of two pieces (tests/test_scale_cpu.py); at 8 the build runs away

SCALE_K = (-5, -4, -3, -2, 6, 12, 20)
OFFSETS = {"2^12": (2.0 ** 12, -2.0 ** 12, 2.0 ** 13), "2^17": (2.0 ** 17, 2.0 ** 17, -2.0 ** 17),
           "2^20": (2.0 ** 20, 0.0, 0.0)}
OVERFLOW_CUBE_K = (34, 41, 42, 43, 50, 62, 63)
OVERFLOW_MONKEY_K = (41, 60)
FAR_K = (8, 14, 17, 20, 23)

_assets, _scenes, _batches, _traces = {}, {}, {}, {}


def asset(name):
    """(vertices centred on the origin, normals, face vertex indices, face normal indices), 0-based."""
    if name not in _assets:
        v, vn, fv, fn = [], [], [], []
        for line in open(asset_path(name)):
            p = line.split()
            if not p:
                continue
            if p[0] == "v":
                v.append([float(x) for x in p[1:4]])
            elif p[0] == "vn":
                vn.append([float(x) for x in p[1:4]])
            elif p[0] == "f":
                assert len(p) == 4, line
                idx = [q.split("/") for q in p[1:]]
                fv.append([int(q[0]) - 1 for q in idx])
                fn.append([int(q[2]) - 1 for q in idx])
        v = np.array(v, F)
        lo, hi = v.min(axis=0), v.max(axis=0)
        v = (v - (lo + (hi - lo) / F(2.0))).astype(F)
        _assets[name] = (v, np.array(vn, F), np.array(fv, np.int64), np.array(fn, np.int64))
        for a in _assets[name]:
            a.setflags(write=False)
    return _assets[name]


def place(name, s, c=(0.0, 0.0, 0.0)):
    """The asset's vertices at scale s around fl32(s * CENTERS[name] + c)."""
    v = asset(name)[0]
    p = (np.float64(s) * np.asarray(CENTERS[name], np.float64) + np.asarray(c, np.float64)).astype(F)
    with np.errstate(over="ignore", invalid="ignore"):
        return ((v * F(s)).astype(F) + p).astype(F)


def obj_text(pieces):
    """OBJ text of pieces [(asset name, placed vertices)]: v, vn, f a//n lines, floats as %.9g."""
    out, faces, v0, n0 = [], [], 0, 0
    for name, v in pieces:
        _, vn, fv, fn = asset(name)
        out += ["v %.9g %.9g %.9g" % tuple(float(x) for x in r) for r in v]
        out += ["vn %.9g %.9g %.9g" % tuple(float(x) for x in r) for r in vn]
        faces += ["f " + " ".join("%d//%d" % (a + 1 + v0, b + 1 + n0) for a, b in zip(ra, rb)) for ra, rb in zip(fv, fn)]
        v0 += len(v)
        n0 += len(vn)
    return "\n".join(out + faces) + "\n"


class ScaleSc(TextSc):
    """A TextSc with its family, its member's name and the camera the renders use."""

    def __init__(self, family, member, text, leaf, eye=APP_EYE, facing=APP_FACING):
        TextSc.__init__(self, text, True, leaf, MODEL_MAT, MATS)
        self.family, self.member = family, member
        self.cam = dict(eye=tuple(float(F(x)) for x in eye), facing=facing)

    @property
    def id(self):
        return "%s-%s" % (self.family, self.member)

    def box(self):
        return np.array(self.parts()[0].surrounding_aabb, F)


def _make(key):
    family, member = key
    if family == "SCALE":
        s = 2.0 ** member
        return ScaleSc(family, member, obj_text([("Monkey", place("Monkey", s))]), LEAF["Monkey"],
                       eye=[s * x for x in APP_EYE])
    if family == "OFFSET":
        c = OFFSETS[member]
        return ScaleSc(family, member, obj_text([("Monkey", place("Monkey", 1.0, c))]), LEAF["Monkey"],
                       eye=[x + y for x, y in zip(APP_EYE, c)])
    if family == "OVERFLOW":
        name, k = member
        s = 2.0 ** k
        return ScaleSc(family, member, obj_text([(name, place(name, s))]), LEAF[name], eye=[s * x for x in APP_EYE])
    if family == "FAR":
        return ScaleSc(family, member, obj_text([("Monkey", place("Monkey", 1.0))]), LEAF["Monkey"])
    assert family == "MIXED_SIZES"
    mid = np.asarray(CENTERS["Monkey"], np.float64)
    pieces = [("Monkey", place("Monkey", 1.0)), ("Monkey", place("Monkey", 2.0 ** -3)),
              ("Cube", ((asset("Cube")[0] * F(2.0 ** 10)).astype(F) + mid.astype(F)).astype(F))]
    return ScaleSc(family, member, obj_text(pieces), MIXED_LEAF)


def scene(family, member):
    key = (family, member)
    if key not in _scenes:
        _scenes[key] = _make(key)
    return _scenes[key]


MIXED_PIECES = (3936, 3936, 12)  # faces of MIXED_SIZES' pieces, in face order
FAMILIES = {"SCALE": SCALE_K, "OFFSET": tuple(OFFSETS),
            "OVERFLOW": tuple(("Cube", k) for k in OVERFLOW_CUBE_K) + tuple(("Monkey", k) for k in OVERFLOW_MONKEY_K),
            "FAR": ("near",), "MIXED_SIZES": ("three",)}
KEYS = [(f, m) for f, ms in FAMILIES.items() for m in ms]
RENDERED = [(f, m) for f, m in KEYS if f in ("SCALE", "OFFSET", "MIXED_SIZES")] + [("OVERFLOW", ("Cube", 34))]
# the scenes of the two-context comparisons, of the table-row check and (with MIXED_SIZES) of the gathers
SWITCHED = [("SCALE", -3), ("SCALE", 20), ("OFFSET", "2^17")]
GATHERED = SWITCHED + [("MIXED_SIZES", "three")]


def key_id(key):
    f, m = key
    return "%s-%s" % (f, "%s2^%d" % m if isinstance(m, tuple) else "2^%d" % m if isinstance(m, int) else m)


def trace(sc, kind, o, d):
    """The oracle's trace of a batch (cached, read-only): (face, t, uv)."""
    k = (sc.family, sc.member, kind)
    if k not in _traces:
        face, t, uv, _ = sc.oracle().trace(o, d)
        for a in (face, t, uv):
            a.setflags(write=False)
        _traces[k] = (face, t, uv)
    return _traces[k]


def _freeze(o, d):
    o, d = np.ascontiguousarray(o, F), np.ascontiguousarray(d, F)
    o.setflags(write=False)
    d.setflags(write=False)
    return o, d


def raw_batch(sc, kind):
    """A batch as its generator gives it, rows that fail the validity test included."""
    k = (sc.family, sc.member, kind, "raw")
    if k not in _batches:
        box = sc.box()
        with np.errstate(over="ignore", invalid="ignore"):
            if kind == "aimed":
                o, d = R.aimed(box, N_AIMED, 11)
            elif kind == "second":
                ao, ad = batch(sc, "aimed")
                o, d = R.second_generation(ao, ad, trace(sc, "aimed", ao, ad)[1], 22, N_SMALL)
            elif kind == "axis":
                o, d = R.axis(box, N_SMALL, 23)
            elif kind == "inner":  # MIXED_SIZES: from inside the Cube, aimed at the Monkey's own box
                v = place("Monkey", 1.0)
                o, d = R.aimed(np.concatenate([v.min(axis=0), v.max(axis=0)]).astype(F), N_AIMED, 12)
            else:
                assert kind[0] == "far" and sc.family == "FAR"
                ao, ad = R.aimed(box, N_AIMED, 11)
                diag = np.sqrt(((box[3:].astype(np.float64) - box[:3].astype(np.float64)) ** 2).sum())
                o = (ao.astype(np.float64) - ad.astype(np.float64) * (2.0 ** kind[1] * diag)).astype(F)
                d = ad
        _batches[k] = _freeze(o, d)
    return _batches[k]


def batch(sc, kind):
    """The rows of a batch that pass atr_trace_rays' validity test."""
    k = (sc.family, sc.member, kind)
    if k not in _batches:
        o, d = raw_batch(sc, kind)
        ok = R.passes(o, d)
        _batches[k] = _freeze(o[ok], d[ok])
    return _batches[k]


def invalid_batch(sc, kind):
    """The rows that fail it (origins that overflowed at the largest scales): possibly empty."""
    o, d = raw_batch(sc, kind)
    bad = ~R.passes(o, d)
    return _freeze(o[bad], d[bad])


def kinds(sc):
    """The batch kinds of a scene: the three of every scene, FAR's moved-back origins, and MIXED_SIZES'
    batch from inside the Cube (the aimed one starts outside it and meets its outer faces alone)."""
    return ("aimed", "second", "axis") + (tuple(("far", k) for k in FAR_K) if sc.family == "FAR" else ()) + (
        ("inner",) if sc.family == "MIXED_SIZES" else ())


def hit_rays(sc, n=256):
    """The first n rays that hit, of the aimed batch (MIXED_SIZES: of the inner one, on the Monkeys)."""
    kind = "inner" if sc.family == "MIXED_SIZES" else "aimed"
    o, d = batch(sc, kind)
    face, t, _ = trace(sc, kind, o, d)
    rows = np.flatnonzero(face != R.MISS)[:n]
    assert len(rows) == n, (sc.id, len(rows))
    return np.ascontiguousarray(o[rows]), np.ascontiguousarray(d[rows]), t[rows]


def frame_hits(sc, W=RW, H=RH):
    """(face, t) of the oracle's primary rays from the scene's camera."""
    from oracle import oracle as O
    face, t, _ = sc.oracle().primary_hits(O.Camera(W, H, **sc.cam))
    return face, t


def points(sc, n=256):
    """n surface points from hit_rays: the positions o + d * t, and as the hemisphere's axis the negated
    ray direction (a unit vector on the side the ray came from), every other one turned into the
    surface (in MIXED_SIZES: into the Monkey's head, where the copy at 2^-3 sits)."""
    o, d, t = hit_rays(sc, n)
    p = (o + (d * t[:, None]).astype(F)).astype(F)
    nrm = (-d).astype(F)
    nrm[1::2] = -nrm[1::2]
    return np.ascontiguousarray(p), np.ascontiguousarray(nrm)
