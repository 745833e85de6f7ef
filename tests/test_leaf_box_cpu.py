"""The primary kernels' leaf boxes on the CPU: an operation-for-operation float32
restatement, in numpy, of the box construction (cluster.h leaf_box_add / leaf_box_entry), of the
lane's leaf test (trace.h leaf_box_miss) and of the loose test of cluster_pads (cluster.h). What the
kernels rely on is one implication, for the f32 operations as executed: a ray that fails the leaf test
fails the loose test of every cluster of that leaf, whatever the best so far. It is checked with zero
exceptions on random and adversarial inputs: leaves of 1 to 75 clusters, growths from 1e-9 to 1e6,
geometry at the magnitudes of tests/scale_scenes.py (2^-5 .. 2^20, up to 2^20 from the origin), rays
aimed within a few ulps of the faces, edges and corners of the leaf box and of the grown cluster
boxes, from outside, from inside and from a face, directions with a component down to 1e-30 (1 / d
up to 1e30) and directions scaled by 2^-20 .. 2^20 (tiny 1 / d). And the construction is compared
with float64 containment: every cluster box grown by its growth lies inside [LO, HI]. No GPU."""
import numpy as np
import pytest

F = np.float32
INF = F(np.inf)
TEST, EMPTY, KEEP = 0, 1, 2


def below(x):
    """cluster.h f32_below on finite values (a zero steps to the smallest negative subnormal)."""
    return np.nextafter(x, -INF, dtype=F)


def above(x):
    return np.nextafter(x, INF, dtype=F)


def leaf_box(eye, lo, hi, gl):
    """leaf_box_init / leaf_box_add over the clusters (lo, hi: (K, 3), gl: (K,)) / leaf_box_entry:
    (LO, HI, flag), every operation a float32 one in the kernel's order."""
    eye, lo, hi, gl = (np.asarray(a, F) for a in (eye, lo, hi, gl))
    if len(gl) == 0:
        return np.zeros(3, F), np.zeros(3, F), EMPTY
    with np.errstate(all="ignore"):
        g = gl * F(1.0009765625)
        Fd = np.fmax(np.abs(lo - eye), np.abs(hi - eye))           # (K, 3)
        slack = g[:, None] + F(9.5367432e-7) * Fd
        x0, x1 = below(lo - slack), above(hi + slack)
        bad = bool((~(slack < INF) | ~(np.abs(x0) < INF) | ~(np.abs(x1) < INF)).any())
        LO, HI = np.full(3, INF, F), np.full(3, -INF, F)
        for k in range(len(gl)):                                   # fminf / fmaxf drop a NaN
            LO, HI = np.fmin(LO, x0[k]), np.fmax(HI, x1[k])
        bad = bad or bool((~(np.abs(LO - eye) < INF) | ~(np.abs(HI - eye) < INF)).any())
    if bad:
        return np.zeros(3, F), np.zeros(3, F), KEEP
    return LO, HI, TEST


def leaf_miss(o, inv, LO, HI, flag):
    """trace.h leaf_box_miss for rays (R, 3): True where the pass leaves the leaf out."""
    if flag != TEST:
        return np.full(len(inv), flag == EMPTY)
    with np.errstate(all="ignore"):
        a, b = (LO - o) * inv, (HI - o) * inv
        n, f = np.fmin(a, b), np.fmax(a, b)
        tn = np.fmax(np.fmax(n[:, 0], n[:, 1]), n[:, 2])
        tf = np.fmin(np.fmin(f[:, 0], f[:, 1]), f[:, 2])
        return (tn > tf) | (tf < F(0.0))


def loose_pass(o, inv, lo, hi, gl):
    """cluster_pads' loose test with best = +inf, rays (R, 3) x clusters (K, 3): True where it passes."""
    with np.errstate(all="ignore"):
        s = np.abs(inv)[:, None, :]                                # (R, 1, 3)
        a = (lo[None] - o) * inv[:, None, :]                       # (R, K, 3)
        b = (hi[None] - o) * inv[:, None, :]
        n, f = np.fmin(a, b), np.fmax(a, b)
        gs = gl[None, :, None] * s
        nn, ff = n - gs, f + gs
        tn = np.fmax(np.fmax(nn[..., 0], nn[..., 1]), nn[..., 2])
        tf = np.fmin(np.fmin(ff[..., 0], ff[..., 1]), ff[..., 2])
        return ~((tn > tf) | (tf < F(0.0)))


def unit(v):
    """engine.h unit(): 1 / sqrt(len2), then three products, in float32."""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        l2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        return v * (F(1.0) / np.sqrt(l2))[:, None]


def nudge(p, k):
    """p moved k floats (k may be negative) per component."""
    p = np.array(p, F)
    for _ in range(abs(int(k))):
        p = np.nextafter(p, INF if k > 0 else -INF, dtype=F)
    return p


def leaf_case(rng, scale, offset, K, gmag, where):
    """One leaf: K cluster boxes inside an octant of size ~scale around offset + scale * (0, 1, -2.2),
    growths around gmag (log-uniform over two decades), and an eye: 'out' the app's distance away, 'in'
    inside the leaf's content, 'face' on a cluster box face, 'near' a fraction of the octant away."""
    c = np.asarray(offset, np.float64) + scale * np.array([0.0, 1.0, -2.2])
    ext = scale * 0.25
    a = c + ext * rng.uniform(-1, 1, (K, 3))
    b = a + ext * rng.uniform(0, 0.5, (K, 3)) * rng.choice([0.0, 1.0], (K, 3), p=[0.1, 0.9])  # flat boxes too
    lo, hi = a.astype(F), np.maximum(a.astype(F), b.astype(F))
    gl = (gmag * 10.0 ** rng.uniform(-1, 1, K)).astype(F)
    if where == "out":
        eye = np.asarray(offset, np.float64) + scale * np.array([0.1, 2.0, 0.0])
    elif where == "in":
        eye = (lo[0].astype(np.float64) + hi[0]) / 2
    elif where == "face":
        eye = (lo[0].astype(np.float64) + hi[0]) / 2
        eye[rng.integers(3)] = lo[0][rng.integers(3)]
    else:
        eye = c + ext * rng.uniform(1.0, 1.5, 3) * rng.choice([-1, 1], 3)
    return eye.astype(F), lo, hi, gl


def rays_for(rng, eye, lo, hi, gl, LO, HI, flag, n_random=96):
    """Directions (float32, as the kernel's unit() leaves them, plus scaled copies) from the eye: random
    ones, ones with a tiny component, and ones aimed a few floats either side of the faces, edges and
    corners of the leaf box and of the first clusters' grown boxes."""
    targets = []
    boxes = []
    if flag == TEST:
        boxes.append((LO, HI))
    with np.errstate(all="ignore"):
        for k in range(min(len(gl), 3)):
            boxes.append((lo[k] - gl[k], hi[k] + gl[k]))
    for l, h in boxes:
        if not (np.isfinite(l).all() and np.isfinite(h).all()):
            continue
        for corner in range(8):
            p = np.array([h[a] if (corner >> a) & 1 else l[a] for a in range(3)], F)
            for k in (-3, -1, 0, 1, 3):
                targets.append(nudge(p, k))
            for a in range(3):  # an edge and a face point next to this corner
                q = p.copy()
                q[a] = F((np.float64(l[a]) + h[a]) / 2)
                targets += [nudge(q, -2), q, nudge(q, 2)]
                r = q.copy()
                r[(a + 1) % 3] = F((np.float64(l[(a + 1) % 3]) + h[(a + 1) % 3]) / 2)
                targets += [nudge(r, -2), r, nudge(r, 2)]
    d = [rng.normal(size=(n_random, 3))]
    tiny = rng.normal(size=(24, 3))
    tiny[np.arange(24), rng.integers(0, 3, 24)] *= 10.0 ** rng.uniform(-30, -6, 24)
    d.append(tiny)
    if targets:
        with np.errstate(all="ignore"):
            d.append(np.array(targets, F) - eye)
    d = np.concatenate([np.asarray(x, F) for x in d])
    d = d[np.isfinite(d).all(axis=1) & (np.abs(d).max(axis=1) > 0)]
    u = unit(d)
    u = u[np.isfinite(u).all(axis=1)]
    scaled = [u] + [u[:: 7] * F(2.0 ** k) for k in (-20, -7, 9, 20)]
    return np.concatenate(scaled).astype(F)


def check_leaf(eye, lo, hi, gl, d):
    LO, HI, flag = leaf_box(eye, lo, hi, gl)
    with np.errstate(all="ignore"):
        inv = (F(1.0) / d).astype(F)
    inv = inv[np.isfinite(inv).all(axis=1)]  # the lanes that may skip: 1 / d finite on every axis
    miss = leaf_miss(eye, inv, LO, HI, flag)
    if len(gl) and miss.any():
        ok = loose_pass(eye, inv[miss], lo, hi, gl)
        assert not ok.any(), ("a skipped leaf with a cluster that passes", eye, int(ok.sum()), np.argwhere(ok)[:3])
    if flag == TEST:  # float64 containment of every grown cluster box
        g = gl.astype(np.float64)[:, None]
        assert (LO.astype(np.float64) <= lo.astype(np.float64) - g).all()
        assert (HI.astype(np.float64) >= hi.astype(np.float64) + g).all()
    return flag, int(miss.sum()), len(inv)


SCALES = [2.0 ** k for k in (-5, -3, 0, 6, 12, 20)]
OFFSETS = [(0.0, 0.0, 0.0), (2.0 ** 12, -2.0 ** 12, 2.0 ** 13), (2.0 ** 17, 2.0 ** 17, -2.0 ** 17), (2.0 ** 20, 0.0, 0.0)]
GROWTHS = [1e-9, 1e-6, 1e-3, 0.063, 2.0, 1e3, 1e6]


@pytest.mark.parametrize("where", ["out", "near", "in", "face"])
def test_leaf_test_culls_only_what_every_cluster_rejects(where):
    rng = np.random.default_rng({"out": 1, "near": 2, "in": 3, "face": 4}[where])
    skipped = rays = leaves = 0
    for scale in SCALES:
        for offset in (OFFSETS if scale == 1.0 else OFFSETS[:1]):
            for gmag in GROWTHS:
                for K in (1, 2, int(rng.integers(3, 20)), 75):
                    eye, lo, hi, gl = leaf_case(rng, scale, offset, K, gmag * min(scale, 1.0) if gmag < 1.0 else gmag, where)
                    LO, HI, flag = leaf_box(eye, lo, hi, gl)
                    d = rays_for(rng, eye, lo, hi, gl, LO, HI, flag)
                    _, m, n = check_leaf(eye, lo, hi, gl, d)
                    skipped, rays, leaves = skipped + m, rays + n, leaves + 1
    print(where, "leaves", leaves, "rays", rays, "skipped", skipped)
    assert rays > 20000
    if where in ("out", "near"):
        assert skipped > rays // 20  # the test does cull from outside


def test_the_test_separates_within_a_few_floats_of_the_box():
    """Aimed at the middle of the leaf box: kept; aimed past the +x edge of its near face by a fiftieth of
    the box, so that the ray leaves sideways: culled. (The implication above is empty if the leaf test
    never culls.)"""
    eye = np.array([0.1, 2.0, 0.0], F)
    lo, hi, gl = np.array([[-1.0, 0.0, -3.0]], F), np.array([[1.0, 1.5, -2.0]], F), np.array([0.05], F)
    LO, HI, flag = leaf_box(eye, lo, hi, gl)
    assert flag == TEST
    mid = ((LO.astype(np.float64) + HI) / 2).astype(F)
    past = np.array([HI[0] + F(0.02) * (HI[0] - LO[0]), mid[1], HI[2]], F)
    d = unit(np.array([mid - eye, past - eye], F))
    inv = (F(1.0) / d).astype(F)
    assert leaf_miss(eye, inv, LO, HI, flag).tolist() == [False, True]
    assert loose_pass(eye, inv, lo, hi, gl)[:, 0].tolist() == [True, False]


def test_flags():
    eye = np.array([0.1, 2.0, 0.0], F)
    lo, hi = np.array([[-1.0, 0.0, -3.0]], F), np.array([[1.0, 1.5, -2.0]], F)
    d = unit(np.random.default_rng(7).normal(size=(64, 3)).astype(F))
    inv = (F(1.0) / d).astype(F)
    # a leaf without clusters is always left out: LO = +inf, HI = -inf would not fail the slab test
    LO, HI, flag = leaf_box(eye, np.zeros((0, 3), F), np.zeros((0, 3), F), np.zeros(0, F))
    assert flag == EMPTY and leaf_miss(eye, inv, LO, HI, flag).all()
    with np.errstate(all="ignore"):
        a, b = (np.full(3, INF, F) - eye) * inv, (np.full(3, -INF, F) - eye) * inv
        n, f = np.fmin(a, b), np.fmax(a, b)
        assert not ((n.max(axis=1) > f.min(axis=1)) | (f.min(axis=1) < 0)).any()
    # a non-finite operand or an overflowing growth: never left out
    for bad_gl in (np.inf, np.nan, 3.4e38):  # the last overflows in g (1 + 2^-10)
        assert leaf_box(eye, lo, hi, np.array([bad_gl], F))[2] == KEEP
    for bad in (np.nan, np.inf, -np.inf):
        l2 = lo.copy()
        l2[0, 1] = bad
        assert leaf_box(eye, l2, hi, np.array([0.05], F))[2] == KEEP
        e2 = eye.copy()
        e2[2] = bad
        assert leaf_box(e2, lo, hi, np.array([0.05], F))[2] == KEEP
    far = np.array([3e38, 0.0, 0.0], F)  # finite bounds whose difference from the eye overflows
    assert leaf_box(-far, lo + far, hi + far, np.array([0.05], F))[2] == KEEP
    LO, HI, flag = leaf_box(eye, lo, hi, np.array([np.inf], F))
    assert not leaf_miss(eye, inv, LO, HI, flag).any()
    # one bad cluster among good ones spoils the leaf
    lo2, hi2 = np.concatenate([lo, lo]), np.concatenate([hi, hi])
    assert leaf_box(eye, lo2, hi2, np.array([0.05, np.nan], F))[2] == KEEP
    assert leaf_box(eye, lo2, hi2, np.array([0.05, 0.05], F))[2] == TEST
