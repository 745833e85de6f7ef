"""The variance-guided denoiser's reference for the tests (tests/c/denoise_variance_ref.c):
atr_denoise_variance's contract of include/atray.h as a plain loop; built with gcc into atray_amd/_lib/
and bound with ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.denoise_ref import same_bits  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "denoise_variance_ref.c")
LIB_PATH = os.path.join(ROOT, "atray_amd", "_lib", "libdenoise_variance_ref.so")
FLAGS = ["-O2", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-fopenmp"]
F = np.float32
EMPTY = 0xFFFFFFFF
# atr_default_denoise_variance_params and Engine.denoise_variance's defaults
DEFAULTS = dict(passes=3, sigma_luminance=8.0, luminance_floor=1e-4, sigma_position=0.0, normal_power_log2=5,
                spatial_below=4)

_lib = None


def build():
    if os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= os.path.getmtime(SRC):
        return LIB_PATH
    os.makedirs(os.path.dirname(LIB_PATH), exist_ok=True)
    tmp = f"{LIB_PATH}.{os.getpid()}.tmp"
    subprocess.run(["gcc"] + FLAGS + ["-shared", "-o", tmp, SRC, "-lm"], check=True)
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        vp, i32, f32 = C.c_void_p, C.c_int32, C.c_float
        L.ref_denoise_variance.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, f32, f32, f32, i32, i32, vp, vp, vp]
        L.ref_denoise_variance.restype = C.c_int
        L.ref_denoise_variance_constants.argtypes = [i32, f32, C.c_int, vp]
        L.ref_denoise_variance_constants.restype = C.c_int
        _lib = L
    return _lib


def constants(passes, sigma_position, position_given=True):
    """(rc, kp[passes]); rc -1: the call is ATR_E_INVALID by the kp rule."""
    kp = np.zeros(passes, F)
    rc = lib().ref_denoise_variance_constants(passes, sigma_position, 1 if position_given else 0, kp.ctypes.data)
    return rc, kp


def denoise_variance(color, variance, normal=None, position=None, ident=None, moments=None, length=None, **params):
    """The reference's (out (H, W, 3) float32, variance_out (H, W) float32, framebuffer (H, W) uint32) for
    (H, W, 3) float32 images, an (H, W) float32 variance, an (H, W) ident and length of 32-bit integers
    and (H, W, 2) float32 moments; None where the kp rule rejects the call. The other arguments are taken
    as valid (atray.h's rules are the entry point's)."""
    kw = dict(DEFAULTS, **params)
    assert set(kw) == set(DEFAULTS), sorted(set(kw) - set(DEFAULTS))
    c = np.ascontiguousarray(color, F)
    h, w = c.shape[:2]
    assert c.shape == (h, w, 3)
    v = np.ascontiguousarray(variance, F)
    assert v.shape == (h, w)
    g = [None if a is None else np.ascontiguousarray(a, F) for a in (normal, position)]
    for a in g:
        assert a is None or a.shape == (h, w, 3)
    idt = None if ident is None else np.ascontiguousarray(ident).view(np.uint32)
    assert idt is None or idt.shape == (h, w)
    assert (moments is None) == (length is None)
    mom = None if moments is None else np.ascontiguousarray(moments, F)
    ln = None if length is None else np.ascontiguousarray(length).view(np.uint32)
    assert mom is None or (mom.shape == (h, w, 2) and ln.shape == (h, w))
    out, vout, fb = np.full((h, w, 3), np.nan, F), np.full((h, w), np.nan, F), np.zeros((h, w), np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = lib().ref_denoise_variance(c.ctypes.data, v.ctypes.data, ptr(g[0]), ptr(g[1]), ptr(idt), ptr(mom), ptr(ln), w, h,
                                    kw["passes"], kw["sigma_luminance"], kw["luminance_floor"], kw["sigma_position"],
                                    kw["normal_power_log2"], kw["spatial_below"], out.ctypes.data, vout.ctypes.data,
                                    fb.ctypes.data)
    return (out, vout, fb) if rc == 0 else None
