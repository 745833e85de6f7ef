"""atr_occluded_rays without a GPU: the symbol, its binding and constants, the NULL-context answer,
segment_rays, and the reference of the GPU tests (tests/occlusion_ref.py: the oracle's walk with its
closest distance started at t_max) validated against the unchanged oracle alone, on the batches of
tests/test_gpu_trace_rays.py."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from atray_amd import engine as E  # noqa: E402
from atray_amd.assets import asset_path  # noqa: E402
from oracle import oracle as O  # noqa: E402
from tests import occlusion_ref as OR  # noqa: E402
from tests import ray_sets as R  # noqa: E402
from tests import test_gpu_scenes as TS  # noqa: E402
from tests import test_gpu_trace_rays as TR  # noqa: E402

F = np.float32
SCENES = ("mixed", "ties", "nomodel")
KINDS = ("aimed", "second", "axis", "inside", "away")
BATCHES = [(s, k) for s in SCENES for k in KINDS]


# ---- the entry point ---------------------------------------------------------------------------------

def test_library_exports_occluded_rays():
    assert "atr_occluded_rays" in E.EXPORTS
    assert hasattr(E.lib(), "atr_occluded_rays")


def test_binding_and_constants():
    args, res = E.signatures()["atr_occluded_rays"]
    assert len(args) == 10 and res is C.c_int
    assert args[4] is C.c_int64 and args[7] is C.c_int32 and args[8] is C.c_int32
    assert (E.ATR_OCCL_VISIBLE, E.ATR_OCCL_OCCLUDED, E.ATR_OCCL_INVALID) == (0, 1, 2)


def test_null_context_is_invalid_without_a_device():
    f = E.lib().atr_occluded_rays
    assert f(None, None, None, None, 0, None, None, E.ATR_KERNEL_AUTO, 0, None) == -1
    assert f(None, None, None, None, 5, None, None, E.ATR_KERNEL_AUTO, -1, None) == -1


# ---- segment_rays --------------------------------------------------------------------------------------

def test_segment_rays():
    rng = np.random.default_rng(41)
    p = rng.uniform(-50, 50, (1025, 3)).astype(F)
    q = (p + rng.normal(size=(1025, 3)).astype(F) * rng.choice([1e-3, 1.0, 300.0], (1025, 1)).astype(F)).astype(F)
    assert (p != q).any(axis=1).all()
    q[7] = p[7]  # a degenerate segment
    for margin in (1e-3, 0.25):
        o, d, tm = (a.numpy() for a in E.segment_rays(torch.from_numpy(p), torch.from_numpy(q), margin))
        assert o.dtype == d.dtype == tm.dtype == np.float32 and d.shape == (1025, 3) and tm.shape == (1025,)
        ok = np.arange(1025) != 7
        assert np.array_equal(o, p)
        assert R.passes(o[ok], d[ok]).all()  # every non-degenerate segment passes the 2^-20 test
        v = q - p
        length = np.sqrt(R.len2(v))
        assert np.array_equal(d[ok].view(np.uint32), R.unit(v[ok]).view(np.uint32))
        assert np.array_equal(tm.view(np.uint32), (length * (F(1.0) - F(margin))).astype(F).view(np.uint32))
        assert np.isnan(d[7]).all() and tm[7] == 0  # NaN direction: ATR_OCCL_INVALID
    with pytest.raises(ValueError):
        E.segment_rays(torch.from_numpy(p).double(), torch.from_numpy(q))


# ---- the reference against the oracle ----------------------------------------------------------------

_bf = {}


def brute_force_t(name, kind):
    """The oracle's closest t on the same scene composed from use_tree=False parts: every triangle
    of every model is tested, no leaf rule."""
    if (name, kind) not in _bf:
        sc = TR.SCENES[name]
        if name not in _bf:
            parts = []
            for n, m in zip(sc.names, sc.model_mats):
                asset, center, leaf, _ = TS.PARTS[n]
                parts.append(O.Scene(asset_path(asset), center=center, max_faces=leaf, use_tree=False, model_material=m))
            _bf[name] = (parts, O.Scene.compose(parts, sc.materials, sc.spheres, sc.planes))
        t = _bf[name][1].trace(*TR.rays(name, kind))[1]
        t.setflags(write=False)
        _bf[name, kind] = t
    return _bf[name, kind]


def batch(name, kind):
    orig, dirs = TR.rays(name, kind)
    return TR.SCENES[name].oracle(), orig, dirs, TR.trace(name, orig, dirs, kind)[1]


@pytest.mark.parametrize("name,kind", BATCHES)
def test_unbounded_is_the_oracles_hit_mask(name, kind):
    """(a) t_max = MAX (and NULL): occluded == (oracle t < MAX)."""
    s, orig, dirs, t_ref = batch(name, kind)
    want = (t_ref < R.MAX_FLOAT).astype(np.uint8)
    assert np.array_equal(OR.occluded(s, orig, dirs), want)
    assert np.array_equal(OR.occluded(s, orig, dirs, np.full(len(orig), R.MAX_FLOAT, F)), want)
    assert np.array_equal(OR.occluded(s, orig, dirs, np.full(len(orig), np.inf, F)), want)


@pytest.mark.parametrize("name,kind", BATCHES)
def test_just_past_the_closest_hit_is_occluded(name, kind):
    """(b) t_max = nextafter(t_ref, +inf): every ray the oracle hits is occluded, with t_ref itself
    or something nearer as the witness."""
    s, orig, dirs, t_ref = batch(name, kind)
    hit = t_ref < R.MAX_FLOAT
    tm = np.nextafter(np.where(hit, t_ref, F(1.0)), F(np.inf)).astype(F)
    tm[~hit] = R.MAX_FLOAT
    out, found = OR.occluded(s, orig, dirs, tm, found=True)
    assert (out[hit] == 1).all() and (out[~hit] == 0).all()
    assert (found[hit] <= t_ref[hit]).all() and (found[hit] > F(1e-4)).all()


@pytest.mark.parametrize("name,kind", BATCHES)
def test_sandwich_between_tree_and_brute_force_oracle(name, kind):
    """(c) t_ref < t_max => occluded and t_bf >= t_max => visible, without exception; the rays
    between (t_bf < t_max <= t_ref: the first-hit-leaf rule kept a farther hit) are at most 3 % of
    the batch."""
    s, orig, dirs, t_ref = batch(name, kind)
    t_bf = brute_force_t(name, kind)
    assert (t_bf <= t_ref).all()
    tm = OR.random_tmax(t_ref)
    out, found = OR.occluded(s, orig, dirs, tm, found=True)
    assert set(np.unique(out).tolist()) <= {0, 1}
    assert (out[t_ref < tm] == 1).all()
    assert (out[t_bf >= tm] == 0).all()
    occ = out == 1
    assert (found[occ] < tm[occ]).all() and (found[occ] >= t_bf[occ]).all() and (found[~occ] == R.MAX_FLOAT).all()
    between = (t_bf < tm) & (tm <= t_ref)
    print(name, kind, "undetermined", int(between.sum()), "of", len(tm), "occluded share", float(occ.mean()))
    assert between.mean() <= 0.03, int(between.sum())
    if name == "mixed" and kind in ("aimed", "second", "axis"):
        assert 0.15 <= occ.mean() <= 0.85, float(occ.mean())  # both classes are there


def test_walk_goes_on_past_a_leaf_that_does_not_improve():
    """(d) t_max = t_ref exactly: the closest-hit walk stopped at t_ref's leaf; a ray occluded here has
    a nearer hit in a later leaf, so the batch tells this query from 'closest t < t_max'."""
    counts = {}
    for name, kind in (("mixed", "aimed"), ("ties", "aimed"), ("ties", "second")):
        s, orig, dirs, t_ref = batch(name, kind)
        out, found = OR.occluded(s, orig, dirs, t_ref, found=True)
        occ = out == 1
        assert (found[occ] < t_ref[occ]).all()
        assert (found[occ] >= brute_force_t(name, kind)[occ]).all()
        counts[name, kind] = int(occ.sum())
    print(counts)
    assert counts["mixed", "aimed"] >= 1, counts


def test_bad_t_max_rows():
    s, orig, dirs, t_ref = batch("mixed", "aimed")
    n = 8
    tm = np.array([np.nan, 0.0, -1.0, -np.inf, np.inf, 1e-5, 1e-40, R.MAX_FLOAT], F)
    out = OR.occluded(s, orig[:n], dirs[:n], tm)
    free = OR.occluded(s, orig[:n], dirs[:n])
    assert out[:4].tolist() == [2, 2, 2, 2]
    assert out[4] == free[4] and out[7] == free[7]  # +inf counts as MAX
    assert out[5] == 0 and out[6] == 0  # nothing is accepted below the tolerance
