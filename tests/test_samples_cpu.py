"""Sample-progressive rendering, host side (no GPU): the default refinement schedule, the exported
entry point and its argument check before any device is touched."""
import ctypes as C

import pytest

from atray_amd import engine as E
from atray_amd import renderer as R


@pytest.mark.parametrize("spp", [1, 2, 3, 64, 100, 256])
def test_sample_schedule_sums_to_spp(spp):
    passes = R.sample_schedule(spp)
    assert sum(passes) == spp
    assert all(isinstance(n, int) and n >= 1 for n in passes)
    # doubling: every pass but the trimmed last one equals the samples done before it (1 first)
    done = 0
    for n in passes[:-1]:
        assert n == max(done, 1)
        done += n
    assert passes[-1] <= max(done, 1)


def test_sample_schedule_examples():
    assert R.sample_schedule(64) == [1, 1, 2, 4, 8, 16, 32]
    assert R.sample_schedule(100) == [1, 1, 2, 4, 8, 16, 32, 36]
    assert R.sample_schedule(1) == [1]
    with pytest.raises(ValueError):
        R.sample_schedule(0)


def test_library_exports_sample_pass_entry_point():
    L = E.lib()
    assert hasattr(L, "atr_render_start_samples")
    assert "atr_render_start_samples" in E.EXPORTS
    args, res = E.signatures()["atr_render_start_samples"]
    assert len(args) == 10 and res is C.c_int


def test_sample_pass_rejects_null_context_without_a_device():
    """ATR_E_INVALID for a NULL context (and NULL camera / frame) before anything is dereferenced."""
    L = E.lib()
    cam = E.atr_camera()
    fr = E.atr_frame()
    dummy = C.create_string_buffer(64)
    sum_ptr = C.cast(dummy, C.c_void_p)
    assert L.atr_render_start_samples(None, C.byref(cam), None, 0, C.byref(fr), 0, None, 0, 0, sum_ptr) == -1
    fake_ctx = C.cast(C.create_string_buffer(64), C.c_void_p)  # never dereferenced: validation fails first
    assert L.atr_render_start_samples(fake_ctx, None, None, 0, C.byref(fr), 0, None, 0, 0, sum_ptr) == -1
    assert L.atr_render_start_samples(fake_ctx, C.byref(cam), None, 0, None, 0, None, 0, 0, sum_ptr) == -1
    # a frame without a framebuffer
    assert L.atr_render_start_samples(fake_ctx, C.byref(cam), None, 0, C.byref(fr), 0, None, 0, 0, sum_ptr) == -1
