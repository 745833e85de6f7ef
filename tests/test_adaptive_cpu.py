"""Adaptive sampling, host side (no GPU): the exported entry points, their signatures and the
argument checks that come before any device or context is touched."""
import ctypes as C

import pytest

from atray_amd import engine as E
from atray_amd import renderer as R


def test_library_exports_adaptive_entry_points():
    L = E.lib()
    sig = E.signatures()
    for name, nargs in (("atr_render_start_adaptive", 12), ("atr_render_adaptive_info", 2)):
        assert hasattr(L, name)
        assert name in E.EXPORTS
        args, res = sig[name]
        assert len(args) == nargs and res is C.c_int
    assert E.ATR_SAMPLES_CONVERGED == 0x80000000
    assert hasattr(E.Engine, "render_start_adaptive") and hasattr(E.Engine, "adaptive_info")


def test_adaptive_pass_rejects_bad_arguments_without_a_device():
    """ATR_E_INVALID for a NULL context, camera or frame, a NULL count and a NaN tolerance, before
    anything is dereferenced: the context handed in is 64 bytes of nothing."""
    L = E.lib()
    cam = E.atr_camera()
    cam.width, cam.height, cam.samples_per_pixel, cam.bounce_limit = 16, 16, 1, 1
    dummy = C.create_string_buffer(64)
    ptr = C.cast(dummy, C.c_void_p)
    fr = E.atr_frame(E.ATR_LAYOUT_IMAGE, ptr, None, None, None, None, None)
    fake_ctx = C.cast(C.create_string_buffer(64), C.c_void_p)
    tiles = (E.atr_tile * 1)(E.atr_tile(0, 0, 15, 15))
    t = C.cast(tiles, C.c_void_p)
    f = L.atr_render_start_adaptive
    assert f(None, C.byref(cam), t, 1, C.byref(fr), 0, None, 0, 0, ptr, ptr, 0.01) == -1
    assert f(fake_ctx, None, t, 1, C.byref(fr), 0, None, 0, 0, ptr, ptr, 0.01) == -1
    assert f(fake_ctx, C.byref(cam), t, 1, None, 0, None, 0, 0, ptr, ptr, 0.01) == -1
    assert f(fake_ctx, C.byref(cam), t, 1, C.byref(fr), 0, None, 0, 0, ptr, None, 0.01) == -1
    assert f(fake_ctx, C.byref(cam), t, 1, C.byref(fr), 0, None, 0, 0, None, ptr, 0.01) == -1
    for tol in (float("nan"), float("inf"), -1.0):
        assert f(fake_ctx, C.byref(cam), t, 1, C.byref(fr), 0, None, 0, 0, ptr, ptr, tol) == -1
    for variant in (E.ATR_KERNEL_FLAT, E.ATR_KERNEL_LANE, E.ATR_KERNEL_HYBRID, 5):
        assert f(fake_ctx, C.byref(cam), t, 1, C.byref(fr), 0, None, variant, 0, ptr, ptr, 0.01) == -1
    assert L.atr_render_adaptive_info(None, (C.c_int64 * 4)()) == -1


def test_renderer_adaptive_tolerance_needs_sample_passes():
    """The argument check comes before any tile, buffer or engine call."""
    rs = R.RenderSettings(resolution=(32, 16), samples_per_pixel=4, bounce_limit=2)
    info = R.RenderInfo(camera=R.Camera(rs, None), scene=None)
    with pytest.raises(ValueError, match="adaptive_tolerance"):
        R.start_render_from_camera(info, None, adaptive_tolerance=0.01)
    for tol in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="adaptive_tolerance"):
            R.start_render_from_camera(info, None, sample_passes=[2, 2], adaptive_tolerance=tol)
