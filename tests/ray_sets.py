"""Ray batches for the atr_trace_rays tests (tests/test_trace_rays_cpu.py, tests/test_gpu_trace_rays.py):
numpy float32 throughout, fixed seeds, directions normalised the way engine.h unit() does."""
import numpy as np

F = np.float32
MISS = 0xFFFFFFFF
MAX_FLOAT = np.float32(3.402823466e38)
LEN2_TOL = np.float32(2.0 ** -20)  # atr_trace_rays' validity bound on |len2(d) - 1|


def len2(v):
    """engine.h:52, in its order."""
    v = np.asarray(v, F)
    return (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]


def unit(v):
    """engine.h unit(): v * (1 / sqrt(len2(v))), every operation a separately rounded f32 one."""
    v = np.asarray(v, F)
    inv = F(1.0) / np.sqrt(len2(v))
    return v * inv[:, None]


def passes(orig, dirs):
    """The validity test of atr_trace_rays, restated: six finite inputs, |len2(d) - 1| <= 2^-20."""
    fin = np.isfinite(orig).all(axis=1) & np.isfinite(dirs).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        return fin & (np.abs(len2(dirs) - F(1.0)) <= LEN2_TOL)


def _box(box):
    box = np.asarray(box, F)
    lo, hi = box[:3], box[3:]
    return lo, hi, hi - lo, (lo + hi) * F(0.5)


def aimed(boxes, n, seed):
    """Ray i belongs to boxes[i % len(boxes)]: its origin is centre + extent * U(-1.5, 1.5) of that
    box, its direction points at lo + extent * U(0.2, 0.8)."""
    if np.ndim(boxes) == 1:
        boxes = [boxes]
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1.5, 1.5, (n, 3)).astype(F)
    b = rng.uniform(0.2, 0.8, (n, 3)).astype(F)
    orig, tgt = np.empty((n, 3), F), np.empty((n, 3), F)
    for k, box in enumerate(boxes):
        lo, _, ext, ctr = _box(box)
        sl = slice(k, n, len(boxes))
        orig[sl] = ctr + ext * a[sl]
        tgt[sl] = lo + ext * b[sl]
    return orig, unit(tgt - orig)


def random_dirs(n, rng):
    return unit(rng.normal(size=(n, 3)).astype(F) + F(1e-3))


def second_generation(orig, dirs, t, seed, n=None):
    """From the hits (t < MAX_FLOAT) of a batch: origins o + d * t on the surfaces, random unit
    directions."""
    hit = t < MAX_FLOAT
    o = orig[hit] + dirs[hit] * t[hit][:, None]
    if n is not None:
        o = o[:n]
    return np.ascontiguousarray(o, F), random_dirs(len(o), np.random.default_rng(seed))


def axis(boxes, n, seed):
    """Directions with one or two components exactly +0.0 or -0.0 (an infinite reciprocal), cast back
    from a target inside the box so that many of them hit."""
    if np.ndim(boxes) == 1:
        boxes = [boxes]
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3)).astype(F) + F(1e-3)
    zero_sets = [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2)]
    for i in range(n):
        for ax in zero_sets[i % 6]:
            d[i, ax] = F(-0.0) if (i // 6) % 2 else F(0.0)
    d = unit(d)
    b = rng.uniform(0.2, 0.8, (n, 3)).astype(F)
    back = rng.uniform(0.5, 2.0, n).astype(F)
    orig = np.empty((n, 3), F)
    for k, box in enumerate(boxes):
        lo, _, ext, _ = _box(box)
        sl = slice(k, n, len(boxes))
        orig[sl] = (lo + ext * b[sl]) - d[sl] * (back[sl] * np.sqrt(len2(ext[None, :])))[:, None]
    return orig, d


def inside(box, n, seed):
    """Origins around the centre of the box (inside the Monkey for its box), random directions."""
    rng = np.random.default_rng(seed)
    _, _, ext, ctr = _box(box)
    orig = ctr + ext * rng.uniform(-0.1, 0.1, (n, 3)).astype(F)
    return orig.astype(F), random_dirs(n, rng)


def away(box, n, seed):
    """Origins outside the box, directions radially away from its centre."""
    rng = np.random.default_rng(seed)
    _, _, ext, ctr = _box(box)
    sign = np.where(rng.uniform(size=(n, 3)) < 0.5, F(-1.0), F(1.0)).astype(F)
    orig = (ctr + ext * (rng.uniform(1.0, 1.5, (n, 3)).astype(F) * sign)).astype(F)
    return orig, unit(orig - ctr)
