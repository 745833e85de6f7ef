"""atr_camera_rays_host without a GPU: the library's ray generator -- the one function the device
kernels of atr_camera_rays and atr_camera_guides call -- equals numpy camera_rays in every bit, for
cameras whose last 8 x 8 cell is partial in x, in y and in both, three eyes and fields of view, ranges
that start and end mid-row; the argument errors."""
import ctypes as C

import numpy as np
import pytest

from atray_amd import engine as E

SIZES = [(1, 1), (8, 8), (13, 7), (65, 9), (72, 40)]
VIEWS = [dict(), dict(eye=(4.0, 0.25, -3.0), facing=(-1.0, -0.1, -0.4), h_fov=0.35),
         dict(eye=(-250.5, 1e-3, 7.75), facing=(0.3, 0.9, 0.2), h_fov=2.5)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("view", range(len(VIEWS)))
@pytest.mark.parametrize("w,h", SIZES)
def test_host_rays_equal_numpy_camera_rays(w, h, view):
    cam = E.camera(w, h, **VIEWS[view])
    want_o, want_d = E.camera_rays(cam)
    got_o, got_d = E.camera_rays_host(cam)
    assert got_o.shape == got_d.shape == (w * h, 3)
    assert np.array_equal(bits(got_o), bits(want_o))
    assert np.array_equal(bits(got_d), bits(want_d))
    assert np.isfinite(got_d).all()


@pytest.mark.parametrize("w,h", SIZES[2:])
def test_ranges_that_start_and_end_mid_row(w, h):
    cam = E.camera(w, h, **VIEWS[1])
    want_o, want_d = E.camera_rays(cam)
    n = w * h
    for first, count in [(0, 1), (3, w), (w - 1, 2), (w + 5, 2 * w + 1), (n - 3, 3), (n, 0), (5, 0)]:
        got_o, got_d = E.camera_rays_host(cam, first, count)
        assert got_d.shape == (count, 3)
        assert np.array_equal(bits(got_o), bits(want_o[first:first + count])), (first, count)
        assert np.array_equal(bits(got_d), bits(want_d[first:first + count])), (first, count)


def test_anti_aliasing_and_samples_are_not_read():
    a = E.camera(13, 7, **VIEWS[1])
    b = E.camera(13, 7, spp=4, bounces=5, aa=True, **VIEWS[1])
    assert b.anti_aliasing == 1
    for x, y in zip(E.camera_rays_host(a), E.camera_rays_host(b)):
        assert np.array_equal(bits(x), bits(y))


def test_only_the_range_is_written():
    cam = E.camera(13, 7)
    o = np.full((12, 3), 7.5, np.float32)
    d = np.full((12, 3), 7.5, np.float32)
    rc = E.lib().atr_camera_rays_host(C.byref(cam), 20, 10, o[1:].ctypes.data, d[1:].ctypes.data)
    assert rc == 0
    want_o, want_d = E.camera_rays(cam)
    assert np.array_equal(bits(o[1:11]), bits(want_o[20:30])) and np.array_equal(bits(d[1:11]), bits(want_d[20:30]))
    for a in (o, d):
        assert (a[0] == 7.5).all() and (a[11] == 7.5).all()


def test_argument_errors():
    L = E.lib()
    cam = E.camera(13, 7)
    n = 13 * 7
    o, d = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.float32)
    po, pd = o.ctypes.data, d.ctypes.data
    call = lambda c, first, cnt, a=po, b=pd: L.atr_camera_rays_host(C.byref(c) if c is not None else None, first, cnt, a, b)  # noqa: E731
    assert call(cam, 0, n) == 0
    assert call(cam, n, 0) == 0 and call(cam, 0, 0, None, None) == 0
    assert call(None, 0, 1) == E.lib().atr_camera_rays_host(None, 0, 1, po, pd) == -1
    for first, cnt in [(-1, 1), (0, -1), (0, n + 1), (n, 1), (n + 1, 0), (1, n), (2**62, 2**62)]:
        assert call(cam, first, cnt) == -1, (first, cnt)
    assert call(cam, 0, 1, None, pd) == -1 and call(cam, 0, 1, po, None) == -1
    for field, value in [("width", 0), ("height", 0), ("width", -3), ("h_fov", float("nan")),
                         ("aspect_ratio", float("inf")), ("half_pixel_width", float("nan")),
                         ("half_pixel_height", float("-inf"))]:
        bad = E.atr_camera.from_buffer_copy(cam)
        setattr(bad, field, value)
        assert call(bad, 0, 0) == -1, field
    for vec in ("eye", "frame_center", "camera_x", "camera_y", "camera_z"):
        for axis in "xyz":
            bad = E.atr_camera.from_buffer_copy(cam)
            setattr(getattr(bad, vec), axis, float("nan"))
            assert call(bad, 0, 1) == -1, (vec, axis)
    with pytest.raises(E.AtrError):
        E.camera_rays_host(cam, 5, n)


def test_binding_declares_the_calls():
    sig = E.signatures()
    for name in ("atr_camera_rays_host", "atr_camera_rays", "atr_camera_guides"):
        assert name in E.EXPORTS and name in sig
    assert [f for f, _ in E.atr_guides_out._fields_] == ["normal", "position", "ident", "depth", "material"]
    assert callable(E.Engine.camera_guides) and callable(E.Engine.camera_rays)
