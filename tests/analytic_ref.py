"""The analytic part of get_intersection_data restated in numpy float32, operation for operation as
shade.h (sphere_t, plane_t, scene_finish) and oracle/atr_oracle.c (sphere_hit, plane_hit,
intersect_scene) write it: the t of a ray with a sphere and with a plane, and the selection among a
scene's spheres and planes, optionally seeded with a model's closest hit. Every operation is a
separately rounded f32 one (no fused multiply-add; the square root through f64, which rounds
correctly). The float64 twins at the end only classify inputs (inside or outside, tangent,
parallel); they never supply an expected value. Pinned against the oracle in
tests/test_analytic_cpu.py."""
import numpy as np

F = np.float32
TOL = F(0.0001)  # engine.h kTol, ray.h:5
MAX_FLOAT = F(3.402823466e38)
SKY, TRI, SPHERE, PLANE = 0, 1, 2, 3  # ATR_RAY_SKY, _TRI, _SPHERE, _PLANE


def dot(a, b):
    """engine.h:50."""
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def sqrt(x):
    """The correctly rounded f32 square root (NaN for a negative or NaN argument)."""
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.asarray(x, F).astype(np.float64)).astype(F)


def unit(v):
    """engine.h unit(): v * (1 / sqrt(len2(v)))."""
    v = np.asarray(v, F)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = F(1.0) / sqrt(dot(v, v))
        return (v * inv[..., None]).astype(F)


def sphere_t(o, d, centre, r):
    """shade.h sphere_t: 0 for no hit; NaN where the discriminant is NaN (which no caller accepts)."""
    o, d = np.asarray(o, F), np.asarray(d, F)
    r = F(r)
    with np.errstate(invalid="ignore", over="ignore"):
        pc = o - np.asarray(centre, F)
        pcs = dot(pc, pc)
        b = F(2.0) * dot(d, pc)
        bs = b * b
        c = pcs - r * r
        dmt = bs - F(4.0) * c
        root = sqrt(dmt)
        ta = (-b + root) * F(0.5)
        tb = (-b - root) * F(0.5)
        t = np.where((ta <= 0) & (tb <= 0), F(0.0), np.where(tb > 0, tb, ta))
        return np.where(dmt < 0, F(0.0), t).astype(F)


def plane_t(o, d, normal, dist):
    """shade.h plane_t: 0 where the denominator is strictly inside (-kTol, kTol)."""
    o, d, n = np.asarray(o, F), np.asarray(d, F), np.asarray(normal, F)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        denom = dot(np.broadcast_to(n, d.shape), d)
        t = (F(dist) - dot(o, np.broadcast_to(n, o.shape))) / denom
        return np.where((denom > -TOL) & (denom < TOL), F(0.0), t).astype(F)


def closest(spheres, planes, o, d, best=None, nm=None):
    """scene_finish on a batch: spheres in order, then planes in order, each accepted where
    kTol < t < best. best, nm: the models' closest hit per ray (nm = -1: none); default none.
    Returns a dict: t; kind (SKY, TRI, SPHERE, PLANE); index (the winning sphere or plane, -1 for a
    triangle or the sky); material (0 where kind is TRI or SKY: the model's is the caller's);
    normal (unit; zeros where kind is TRI or SKY); ns, np (the accepted sphere and plane, -1: none:
    both can be set, and then the plane holds the hit)."""
    o, d = np.asarray(o, F), np.asarray(d, F)
    n = len(o)
    best = np.full(n, MAX_FLOAT, F) if best is None else np.array(best, F)
    nm = np.full(n, -1, np.int32) if nm is None else np.asarray(nm, np.int32)
    ns, npl = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    with np.errstate(invalid="ignore"):
        for i, (c, r, _) in enumerate(spheres):
            t = sphere_t(o, d, c, r)
            win = (t > TOL) & (t < best)
            best[win], ns[win] = t[win], i
        for i, (nrm, dist, _) in enumerate(planes):
            t = plane_t(o, d, nrm, dist)
            win = (t > TOL) & (t < best)
            best[win], npl[win] = t[win], i
    pl, sp = npl >= 0, (npl < 0) & (ns >= 0)
    kind = np.where(pl, PLANE, np.where(sp, SPHERE, np.where(nm >= 0, TRI, SKY))).astype(np.int32)
    index = np.where(pl, npl, np.where(sp, ns, -1)).astype(np.int32)
    material = np.zeros(n, np.int32)
    normal = np.zeros((n, 3), F)
    if pl.any():
        material[pl] = np.asarray([p[2] for p in planes], np.int32)[npl[pl]]
        normal[pl] = unit(np.asarray([p[0] for p in planes], F)[npl[pl]])
    if sp.any():
        material[sp] = np.asarray([s[2] for s in spheres], np.int32)[ns[sp]]
        at = o[sp] + d[sp] * best[sp][:, None]  # Ray::at, then minus the centre
        normal[sp] = unit(at - np.asarray([s[0] for s in spheres], F)[ns[sp]])
    return {"t": best, "kind": kind, "index": index, "material": material, "normal": normal, "ns": ns, "np": npl}


# ---- float64, to classify inputs only ---------------------------------------------------------------

def sphere_t64(o, d, centre, r):
    """(discriminant, ta, tb) in float64."""
    o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        pc = o - np.asarray(centre, np.float64)
        b = 2.0 * (pc * d).sum(axis=-1)
        dmt = b * b - 4.0 * ((pc * pc).sum(axis=-1) - float(r) * float(r))
        root = np.sqrt(dmt)
        return dmt, (-b + root) * 0.5, (-b - root) * 0.5


def inside(o, centre, r):
    """Origins strictly inside a sphere (float64)."""
    pc = np.asarray(o, np.float64) - np.asarray(centre, np.float64)
    return (pc * pc).sum(axis=-1) < float(r) * float(r)


def plane_t64(o, d, normal, dist):
    """(denominator, t) in float64."""
    o, d, n = np.asarray(o, np.float64), np.asarray(d, np.float64), np.asarray(normal, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        denom = (d * n).sum(axis=-1)
        return denom, (float(dist) - (o * n).sum(axis=-1)) / denom
