"""atr_trace_rays without a GPU: the symbol, its binding, the hit record's size, the NULL-context
answer, and the test ray generators' own conditions, measured on the oracle alone (so that the GPU
tests of tests/test_gpu_trace_rays.py compare batches that do hit something)."""
import ctypes as C

import numpy as np
import pytest

from atray_amd import engine as E
from atray_amd.assets import CENTERS, asset_path
from oracle import oracle as O
from tests import ray_sets as R

N = 4097


def test_library_exports_trace_rays():
    assert "atr_trace_rays" in E.EXPORTS
    assert hasattr(E.lib(), "atr_trace_rays")


def test_binding_lists_trace_rays():
    args, res = E.signatures()["atr_trace_rays"]
    assert len(args) == 8 and res is C.c_int
    assert args[3] is C.c_int64 and args[5] is C.c_int32 and args[6] is C.c_int32
    assert (E.ATR_RAY_SKY, E.ATR_RAY_TRI, E.ATR_RAY_SPHERE, E.ATR_RAY_PLANE, E.ATR_RAY_INVALID) == (0, 1, 2, 3, 4)


def test_ray_hits_is_eight_pointers():
    assert C.sizeof(E.atr_ray_hits) == 8 * C.sizeof(C.c_void_p)
    assert [f[0] for f in E.atr_ray_hits._fields_] == ["t", "face", "model", "uv", "kind", "material", "normal",
                                                       "traced_rays"]


def test_null_context_is_invalid_without_a_device():
    hits = E.atr_ray_hits()
    assert E.lib().atr_trace_rays(None, None, None, 0, C.byref(hits), E.ATR_KERNEL_AUTO, 0, None) == -1
    assert E.lib().atr_trace_rays(None, None, None, 5, None, E.ATR_KERNEL_AUTO, -1, None) == -1


_scenes = {}


def scene(asset, leaf):
    if (asset, leaf) not in _scenes:
        _scenes[asset, leaf] = O.Scene(asset_path(asset), center=CENTERS[asset], max_faces=leaf)
    return _scenes[asset, leaf]


@pytest.mark.parametrize("asset,leaf", [("Monkey", 64), ("Deer", 300), ("Cube", 300)])
def test_aimed_rays_hit(asset, leaf):
    s = scene(asset, leaf)
    orig, dirs = R.aimed(s.surrounding_aabb, N, 11)
    assert R.passes(orig, dirs).all()
    face, t, _, _ = s.trace(orig, dirs)
    share = float((face != R.MISS).mean())
    print(asset, "aimed hit share", share)
    assert share >= 0.5, share


def test_second_generation_rays_hit_again():
    s = scene("Monkey", 64)
    orig, dirs = R.aimed(s.surrounding_aabb, N, 11)
    _, t, _, _ = s.trace(orig, dirs)
    o2, d2 = R.second_generation(orig, dirs, t, 12)
    assert len(o2) >= N // 2 and R.passes(o2, d2).all()
    face, _, _, _ = s.trace(o2, d2)
    share = float((face != R.MISS).mean())
    print("Monkey second-generation hit share", share)
    assert share >= 0.05, share


def test_generators_are_normalised_and_axis_rays_have_zeros():
    box = scene("Monkey", 64).surrounding_aabb
    for o, d in (R.axis(box, 1025, 13), R.inside(box, 1025, 14), R.away(box, 1025, 15)):
        assert o.dtype == np.float32 and d.dtype == np.float32 and R.passes(o, d).all()
    _, d = R.axis(box, 1025, 13)
    zeros = (d == 0).sum(axis=1)
    assert set(zeros.tolist()) == {1, 2}
    assert np.signbit(d[d == 0]).any() and (~np.signbit(d[d == 0])).any()  # +0.0 and -0.0
    # the validity bound's two sides: len2 - 1 = +-2^-20 passes, +-2^-19 does not
    for s, ok in ((1 + 2.0 ** -21, True), (1 - 2.0 ** -21, True), (1 + 2.0 ** -20, False), (1 - 2.0 ** -20, False)):
        d = np.array([[s, 0.0, 0.0]], np.float32)
        assert abs(float(R.len2(d)[0]) - 1.0) == (2.0 ** -20 if ok else 2.0 ** -19)
        assert bool(R.passes(np.zeros((1, 3), np.float32), d)[0]) is ok
