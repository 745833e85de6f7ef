"""The facing fold of the per-camera table of box growths (ATR_FACING_FOLD): the table's
loose growth of a cluster is sized for the camera's det floor delta of that cluster -- the smallest
det the culled test can compute for any primitive of the cluster it does not reject anyway, over
every ray from the eye that reaches the cluster's loose box -- instead of the tolerance kTol. A ray
that misses the folded box accepts nothing inside, so nothing may change: two contexts in one
process, one created with ATR_FACING_FOLD=0, must agree bit for bit on every output and both must
equal the oracle; the COUNT kernel's new counters show that the fold does remove work; and the row
read back with atr_camera_pads_row -- built by the table kernel a launch runs -- is checked against
the bound on densely sampled boxes in float64, against an operation-for-operation restatement of the
kernel's arithmetic (which pins the margin and the rounding direction), and, entry by entry, against
cluster_grow's pair. Needs an MI355X (-m gpu)."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from atray_amd.assets import CENTERS, asset_path  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests.goldens import SEED  # noqa: E402
from tests.test_gpu_camera_pads import frames_of, run_cameras  # noqa: E402
from tests.test_gpu_cluster import grazing_soup  # noqa: E402
from tests.test_gpu_parity import MODEL, SKY, run  # noqa: E402

pytestmark = pytest.mark.gpu
K_TOL, K_TAU, EPS = float(np.float32(1e-4)), float(np.float32(3e-3)), 2.0 ** -24
OUT_KEYS = ("fb", "face", "casts")


def _engine(switch):
    """A context created with ATR_FACING_FOLD = switch (None: unset); the variable is read at creation."""
    old = os.environ.get("ATR_FACING_FOLD")
    try:
        if switch is None:
            os.environ.pop("ATR_FACING_FOLD", None)
        else:
            os.environ["ATR_FACING_FOLD"] = switch
        return E.Engine(0)
    finally:
        if old is None:
            os.environ.pop("ATR_FACING_FOLD", None)
        else:
            os.environ["ATR_FACING_FOLD"] = old


@pytest.fixture(scope="module")
def pair():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    off, on = _engine("0"), _engine(None)
    yield off, on
    off.close()
    on.close()


@pytest.fixture(autouse=True)
def _restore_tuning(pair):
    yield
    for e in pair:
        e.set_tuning(cluster_size=16)


def same(a, b, what=""):
    for k in OUT_KEYS:
        assert np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))
    assert np.array_equal(a["t"].view(np.uint32), b["t"].view(np.uint32)), (what, "t")


APP_EYE, APP_FACING = (0.1, 2.0, 0.0), (-0.1, -0.5, -1.0)
MONKEY_C = CENTERS["Monkey"]
# name -> (asset or None for the soup, leaf size, cluster size, W, H, eye, facing)
SCENES = {
    "cube": ("Cube", 300, 16, 64, 48, APP_EYE, APP_FACING),
    "monkey": ("Monkey", 300, 16, 256, 192, APP_EYE, APP_FACING),
    "soup": (None, 300, 16, 256, 192, APP_EYE, APP_FACING),
    # the same soup from an eye moved 0.5 units: another row of the table
    "soup_moved": (None, 300, 16, 256, 192, (0.6, 2.0, 0.0), APP_FACING),
    "monkey_minus_z": ("Monkey", 300, 16, 72, 56, (MONKEY_C[0], MONKEY_C[1], MONKEY_C[2] + 3.0), (0.0, 0.0, -1.0)),
    "monkey_cluster4": ("Monkey", 300, 4, 64, 48, APP_EYE, APP_FACING),  # up to 75 clusters per leaf
}
_txt, _built, _refs = {}, {}, {}


def soup_text():
    """8,000 triangles (and their exact duplicates) tilted so that det is 0.5-60 x kTol from the app
    eye -- the band between kTol and kTau where the fold decides -- half of them back-facing."""
    if not _txt:
        _txt["soup"] = grazing_soup(8000, 7, (0.5, 60.0))
    return _txt["soup"]


def built(asset, leaf):
    """(engine model tuple, oracle scene) of a one-model scene, built once."""
    key = (asset, leaf)
    if key not in _built:
        if asset is None:
            m = E.Mesh.parse_obj(soup_text())
            box = m.aabb()
            s = O.Scene(obj_text=soup_text(), center=None, max_faces=leaf)
        else:
            m = E.Mesh.load_obj(asset_path(asset))
            box = m.translate_to(m.aabb(), CENTERS[asset])
            s = O.Scene(asset_path(asset), center=CENTERS[asset], max_faces=leaf)
        _built[key] = ((m, E.Octree.build(m, leaf), box, 1), s)
    return _built[key]


def oracle_frame(s, key, W, H, eye, facing):
    """The oracle's framebuffer, hit face, hit t and ray_casts of one frame (computed once)."""
    key = (key, W, H, tuple(eye), tuple(facing))
    if key not in _refs:
        face, t, _ = s.primary_hits(O.Camera(W, H, eye=eye, facing=facing))
        _, fb, casts, _ = s.render(O.Camera(W, H, eye=eye, facing=facing), SEED)
        for a in (face, t, fb, casts):
            a.setflags(write=False)
        _refs[key] = {"fb": fb, "face": face, "casts": casts, "t": t}
    return _refs[key]


def upload(pair, asset, leaf, cs=16):
    md, s = built(asset, leaf)
    for e in pair:
        e.set_tuning(cluster_size=cs)
        e.upload([SKY, MODEL], [md])
    return s


def both_equal_the_oracle(pair, want, cam, what):
    """Both contexts, HYBRID and FLAT (which sends primary-only frames to HYBRID's 6-wave kernel), the
    whole frame and a PACKED render of its two halves: equal to each other and to the oracle."""
    off, on = pair
    W, H = cam.width, cam.height
    halves = [[0, 0, W // 2 - 1, H - 1], [W // 2, 0, W - 1, H - 1]]
    pix = E.packed_pixel_map(halves, W, H)
    for variant in (E.ATR_KERNEL_HYBRID, E.ATR_KERNEL_FLAT):
        x, y = run(off, cam, variant=variant), run(on, cam, variant=variant)
        same(x, y, (what, variant))
        same(y, want, (what, variant, "oracle"))
        px = run(off, cam, tiles=halves, layout=E.ATR_LAYOUT_PACKED, variant=variant)
        py = run(on, cam, tiles=halves, layout=E.ATR_LAYOUT_PACKED, variant=variant)
        same(px, py, (what, variant, "PACKED"))
        same(py, {k: np.asarray(v).reshape(-1)[pix] for k, v in want.items()}, (what, variant, "PACKED oracle"))


@pytest.mark.parametrize("name", list(SCENES))
def test_fold_on_equals_fold_off_and_the_oracle(pair, name):
    off, on = pair
    asset, leaf, cs, W, H, eye, facing = SCENES[name]
    s = upload(pair, asset, leaf, cs)
    want = oracle_frame(s, (asset, leaf), W, H, eye, facing)
    assert int((want["face"] != E.MISS).sum()) > 50  # the model is in view
    cam = E.camera(W, H, eye=eye, facing=facing)
    both_equal_the_oracle(pair, want, cam, name)
    whole = [[0, 0, W - 1, H - 1]]
    # the COUNT build counts the unfolded work, in both contexts
    assert off.counters(cam, whole, SEED, E.ATR_KERNEL_HYBRID) == on.counters(cam, whole, SEED, E.ATR_KERNEL_HYBRID)
    assert off.cull_counters(cam, whole, SEED, E.ATR_KERNEL_HYBRID) == on.cull_counters(cam, whole, SEED, E.ATR_KERNEL_HYBRID)
    f_on, f_off = on.fold_counters(cam, whole, SEED, E.ATR_KERNEL_HYBRID), off.fold_counters(cam, whole, SEED, E.ATR_KERNEL_HYBRID)
    print(name, "fold counters", f_on, "of", on.counters(cam, whole, SEED, E.ATR_KERNEL_HYBRID))
    assert f_off == {"loose_passes_removed": 0, "screened_removed": 0}
    if name in ("monkey", "soup", "soup_moved"):  # the fold is engaged, not silently off
        assert f_on["loose_passes_removed"] > 0 and f_on["screened_removed"] >= f_on["loose_passes_removed"], f_on


def test_moved_eye_reads_another_row(pair):
    off, on = pair
    upload(pair, None, 300)
    a, _, _ = on.camera_pads_row(SCENES["soup"][5])
    b, _, _ = on.camera_pads_row(SCENES["soup_moved"][5])
    assert len(a) == len(b) > 100
    assert (a[:, 2] != b[:, 2]).any() and (a[:, 0] != b[:, 0]).any()
    assert np.array_equal(a, on.camera_pads_row(SCENES["soup"][5])[0])  # and a row is a function of its eye


def test_eye_inside_a_cluster_box(pair):
    """The eye at the centre of the Monkey's largest cluster box (so inside the root box too): that
    cluster, and every other whose loose box holds the eye, reads back delta = kTol."""
    off, on = pair
    s = upload(pair, "Monkey", 300)
    _, boxes, _ = on.camera_pads_row(APP_EYE)
    lo, hi = boxes[:, 0:3].astype(np.float64), boxes[:, 4:7].astype(np.float64)
    k = int(np.argmax(np.prod(hi - lo, axis=1)))
    eye = tuple(float(x) for x in np.float32((lo[k] + hi[k]) / 2))
    root = built("Monkey", 300)[0][2]
    assert all(root[i] < eye[i] < root[3 + i] for i in range(3)), (root, eye)
    row, boxes, _ = on.camera_pads_row(eye)
    g = boxes[:, 8].astype(np.float64)[:, None]
    inside = ((lo - g <= np.array(eye)) & (np.array(eye) <= hi + g)).all(axis=1)
    assert inside[k] and inside.sum() >= 1
    assert (row[inside, 2] == np.float32(K_TOL)).all() and np.array_equal(row[inside, 0], boxes[inside, 8])
    assert (row[inside, 3].view(np.uint32) == 0).all()
    facing = tuple(MONKEY_C[i] - eye[i] for i in range(3))
    if sum(f * f for f in facing) < 1e-6:
        facing = (0.0, 0.0, -1.0)
    W, H = 64, 48
    want = oracle_frame(s, ("Monkey", 300), W, H, eye, facing)
    both_equal_the_oracle(pair, want, E.camera(W, H, eye=eye, facing=facing), "inside")


@pytest.mark.parametrize("layout", [E.ATR_LAYOUT_IMAGE, E.ATR_LAYOUT_PACKED])
def test_three_cameras_in_one_launch(pair, layout):
    """Three eyes in one launch: each frame equals its own one-camera render, in both contexts."""
    off, on = pair
    upload(pair, None, 300)
    W, H = 128, 96
    tiles = [[0, 0, W - 1, H - 1]] if layout == E.ATR_LAYOUT_IMAGE else [[0, 0, 55, H - 1], [56, 0, W - 1, H - 1]]
    cams = [E.camera(W, H, eye=e) for e in (APP_EYE, (0.6, 2.0, 0.0), (0.1, 1.7, 0.4))]
    got = []
    for e in (off, on):
        n, bufs = run_cameras(e, cams, tiles, layout)
        rc, _ = e.wait()
        assert rc == 0
        torch.cuda.synchronize()
        got.append(frames_of(n, len(cams), bufs))
    for f, cam in enumerate(cams):
        same(got[0][f], got[1][f], f)
        one = run(on, cam, tiles=tiles, layout=layout, variant=E.ATR_KERNEL_HYBRID)
        same(got[1][f], {k: np.asarray(v).reshape(-1) for k, v in one.items() if k != "rgb" and k != "traced"}, (f, "one"))
    assert not np.array_equal(got[1][0]["face"], got[1][1]["face"])  # the cameras do differ


def test_two_tree_models_index_their_own_rows(pair):
    """Monkey and Deer in one scene (the second model's clusters start at its cl_base)."""
    from tests.test_gpu_scenes import MATS, Sc, ref  # noqa: E402
    from tests.test_gpu_scenes import same as same_oracle  # noqa: E402
    off, on = pair
    W, H = 96, 72
    for names in (["monkey", "deer"], ["deer", "monkey"]):
        sc = Sc(names, [1, 2], MATS)
        for e in pair:
            sc.upload(e)
        row, boxes, _ = on.camera_pads_row(APP_EYE)
        assert len(row) == len(boxes) > 2 and (boxes[:, 8] > 0).all()  # every cluster of both models has its entry
        cam = E.camera(W, H)
        r = ref(sc, W, H)
        x, y = run(off, cam, variant=E.ATR_KERNEL_HYBRID), run(on, cam, variant=E.ATR_KERNEL_HYBRID)
        same(x, y, names)
        same_oracle(y, r, names)
        whole = [[0, 0, W - 1, H - 1]]
        assert off.counters(cam, whole, SEED, E.ATR_KERNEL_HYBRID) == on.counters(cam, whole, SEED, E.ATR_KERNEL_HYBRID)


# ---------------------------------------------------------------- the bound itself, in float64
def _restated(eye, boxes, edges):
    """cluster.h fold_box / fold_prim / fold_delta restated operation for operation in float64 (IEEE
    on both sides, so the same bits up to the device's f64 square root and quotient): per cluster the
    det floor as f32, the mask of the rejected primitives, whether the cluster may fold, and the
    smallest lower bound it was rounded from."""
    e = np.asarray(np.float32(eye), np.float64)
    lo, hi = boxes[:, 0:3].astype(np.float64), boxes[:, 4:7].astype(np.float64)
    P, q, gl = boxes[:, 3].astype(np.float64), boxes[:, 7], boxes[:, 8].astype(np.float64)
    cnt = (boxes[:, 3].view(np.uint32) & 31) + 1
    g = gl * (1.0 + 2.0 ** -10)
    x0, x1 = np.empty_like(lo), np.empty_like(lo)
    n2, f2 = np.zeros(len(lo)), np.zeros(len(lo))
    for a in range(3):
        F = np.maximum(np.abs(lo[:, a] - e[a]), np.abs(hi[:, a] - e[a]))
        slack = g + 2.0 ** -20 * F
        x0[:, a] = lo[:, a] - e[a] - slack
        x1[:, a] = hi[:, a] - e[a] + slack
        nr = np.maximum(np.maximum(x0[:, a], -x1[:, a]), 0.0)
        fr = np.maximum(np.abs(x0[:, a]), np.abs(x1[:, a]))
        n2 += nr * nr
        f2 += fr * fr
    rmin, rmax = np.sqrt(n2), np.sqrt(f2)
    ok = np.isfinite(f2) & (rmin > rmax * 2.0 ** -10) & (q >= np.float32(1.1754944e-38))
    ab, ac = edges[:, :, 0:3].astype(np.float64), edges[:, :, 3:6].astype(np.float64)
    N = np.stack([ab[:, :, 1] * ac[:, :, 2] - ab[:, :, 2] * ac[:, :, 1], ab[:, :, 2] * ac[:, :, 0] - ab[:, :, 0] * ac[:, :, 2],
                  ab[:, :, 0] * ac[:, :, 1] - ab[:, :, 1] * ac[:, :, 0]], axis=2)
    smin, smax = np.zeros(N.shape[:2]), np.zeros(N.shape[:2])
    for a in range(3):
        u, v = -x0[:, a][:, None] * N[:, :, a], -x1[:, a][:, None] * N[:, :, a]
        smin += np.minimum(u, v)
        smax += np.maximum(u, v)
    m = (32.0 * EPS * P)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        L = smin / np.where(smin >= 0.0, rmax[:, None], rmin[:, None])
        U = smax / np.where(smax >= 0.0, rmin[:, None], rmax[:, None])
    have = np.arange(16)[None, :] < cnt[:, None]
    rejected = have & (U < K_TOL - m) & ok[:, None]
    lower = np.where(have & ~(U < K_TOL - m), L - m, np.inf).min(axis=1)
    d = lower.astype(np.float32)
    above = d.astype(np.float64) > lower
    d = np.where(above, (d.view(np.uint32) - above.astype(np.uint32)).view(np.float32), d)  # the float below
    d = np.maximum(d, np.float32(K_TOL))
    d = np.where(lower >= K_TAU, np.float32(K_TAU), np.where(lower > K_TOL, d, np.float32(K_TOL)))
    d = np.where(ok, d, np.float32(K_TOL)).astype(np.float32)
    mask = (rejected.astype(np.uint32) << np.arange(16, dtype=np.uint32)[None, :]).sum(axis=1).astype(np.uint32)
    return d, mask, ok, lower


def _det_range(eye, lo, hi, g, N, steps=16):
    """Per (cluster, primitive): the smallest and the largest -(u . N) over the unit directions u from
    the eye to steps x steps points on each face of the cluster's box grown by g (corners included)."""
    eye = np.asarray(eye, np.float64)
    a, b = lo - g[:, None], hi + g[:, None]                 # (n, 3)
    s = np.linspace(0.0, 1.0, steps)
    uu, vv = (x.reshape(-1) for x in np.meshgrid(s, s, indexing="ij"))
    pts = []
    for axis in range(3):
        o1, o2 = (axis + 1) % 3, (axis + 2) % 3
        for end in (a, b):
            p = np.empty((len(lo), len(uu), 3))
            p[:, :, axis] = end[:, axis][:, None]
            p[:, :, o1] = a[:, o1][:, None] + (b[:, o1] - a[:, o1])[:, None] * uu[None]
            p[:, :, o2] = a[:, o2][:, None] + (b[:, o2] - a[:, o2])[:, None] * vv[None]
            pts.append(p)
    p = np.concatenate(pts, axis=1) - eye                   # (n, 6 steps^2, 3)
    u = p / np.linalg.norm(p, axis=2, keepdims=True)
    det = -np.einsum("npk,njk->njp", u, N)                  # (n, 16, points)
    return det.min(axis=2), det.max(axis=2)


@pytest.mark.parametrize("name", ["cube", "monkey", "soup", "soup_moved"])
def test_row_obeys_the_bound(pair, name):
    """delta against the float64 restatement. For every cluster with delta > kTol and every primitive of
    it that the row did not treat as rejected: delta <= (sampled minimum of -(d . n)) - m, m = 32 eps P
    the documented margin (a delta of kTol is what the kernels assumed before and claims nothing). Every
    primitive treated as rejected has a sampled det below kTol everywhere."""
    asset, leaf, cs, W, H, eye, facing = SCENES[name]
    upload(pair, asset, leaf, cs)
    row_obeys_the_bound(pair, name, eye, must_fold=name != "cube")


def row_obeys_the_bound(pair, name, eye, must_fold):
    """The checks of test_row_obeys_the_bound on the scene both contexts hold, from `eye`; must_fold:
    some cluster has to fold (the fold is engaged, not silently off)."""
    off, on = pair
    row, boxes, edges = on.camera_pads_row(eye)
    n = len(row)
    assert n > 0
    P = boxes[:, 3].astype(np.float64)
    cnt = (boxes[:, 3].view(np.uint32) & 31) + 1
    lo, hi, gl = boxes[:, 0:3].astype(np.float64), boxes[:, 4:7].astype(np.float64), boxes[:, 8].astype(np.float64)
    gf, gt, delta = (row[:, i].astype(np.float64) for i in range(3))
    rej = row[:, 3].view(np.uint32)
    ab, ac = edges[:, :, 0:3].astype(np.float64), edges[:, :, 3:6].astype(np.float64)
    N = np.cross(ab, ac)
    assert (np.linalg.norm(N, axis=2) <= P[:, None] * (1 + 1e-6)).all()  # P bounds |ab||ac| >= |n|
    assert ((delta >= K_TOL) & (delta <= K_TAU)).all()
    assert ((gt <= gf) & (gf <= gl)).all()
    assert np.array_equal(row[delta == K_TOL, 0], boxes[delta == K_TOL, 8])  # nothing folded: today's bits
    # g_f is cluster_grow's expression with delta in kTol's place: W from the unfolded pair
    kl, ka = 36 * EPS / (float(np.float32(0.9)) * K_TOL), 12 * EPS
    Wd = gl / (P * kl + ka)
    expect = np.clip(Wd * (P * (36 * EPS / (float(np.float32(0.9)) * delta)) + ka), gt, gl)
    assert np.allclose(gf, expect, rtol=1e-5, atol=0.0)
    dmin, dmax = np.empty((n, 16)), np.empty((n, 16))
    for c0 in range(0, n, 256):
        c1 = min(n, c0 + 256)
        dmin[c0:c1], dmax[c0:c1] = _det_range(eye, lo[c0:c1], hi[c0:c1], gl[c0:c1], N[c0:c1])
    have = np.arange(16)[None, :] < cnt[:, None]
    rejected = ((rej[:, None] >> np.arange(16)[None, :]) & 1).astype(bool)
    assert not (rejected & ~have).any()
    m = 32 * EPS * P
    folded = delta > K_TOL
    claim = have & ~rejected & folded[:, None]
    bad = claim & ~(delta[:, None] <= dmin - m[:, None])
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    bad = rejected & ~(dmax < K_TOL)
    assert not bad.any(), (name, int(bad.sum()), np.argwhere(bad)[:5].tolist())
    # The sampling cannot see an error of the margin's size. The restatement can: delta is the f32
    # just below (min L - m) with m = 32 eps P -- half the margin would move it by hundreds of ulp
    d_want, mask_want, ok, lower = _restated(eye, boxes, edges)
    ulps = np.abs(row[:, 2].view(np.uint32).astype(np.int64) - d_want.view(np.uint32).astype(np.int64))
    print(name, "delta equal to the restatement in", int((ulps == 0).sum()), "of", n, "clusters, largest difference", int(ulps.max()), "ulp")
    assert ulps.max() <= 1, (name, int(ulps.max()), np.argwhere(ulps > 1)[:5].tolist())
    assert np.array_equal(rej, mask_want), (name, np.argwhere(rej != mask_want)[:5].tolist())
    between = folded & (delta < K_TAU)
    assert (delta[between] <= lower[between] * (1 + 1e-12)).all()  # rounded down, never up
    assert (lower[between] - delta[between] <= 2.0 ** -23 * delta[between]).all()  # and by less than an ulp
    # the entry's tight growth is cluster_grow's, from the unfolded pair: g_t / g_l = (P k_t + k_a) / (P k_l + k_a)
    kt = 36 * EPS / (float(np.float32(0.9)) * K_TAU)
    assert np.allclose(gt, gl * (P * kt + ka) / (P * kl + ka), rtol=1e-5, atol=0.0)
    print(name, "clusters", n, "folded", int(folded.sum()), "at kTau", int((delta == K_TAU).sum()),
          "primitives rejected", int(rejected.sum()), "of", int(have.sum()))
    if must_fold:
        assert folded.sum() > 0  # the fold is engaged
    # The other context's table is today's, built by today's kernel: its entries are, bit for bit, the
    # pair that cluster_grow returns in the folding kernel (boxes[:, 8], this context's tight growth)
    r0, b0, _ = off.camera_pads_row(eye)
    assert np.array_equal(b0, boxes) and np.array_equal(r0[:, 0], boxes[:, 8]) and np.array_equal(r0[:, 1], row[:, 1])
    assert (r0[:, 2] == np.float32(K_TOL)).all() and (r0[:, 3].view(np.uint32) == 0).all()
