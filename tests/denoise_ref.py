"""The denoiser's reference for the tests (tests/c/denoise_ref.c): atr_denoise's contract of
include/atray.h as a plain loop; built with gcc into atray_amd/_lib/ and bound with ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "denoise_ref.c")
LIB_PATH = os.path.join(ROOT, "atray_amd", "_lib", "libdenoise_ref.so")
FLAGS = ["-O2", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-fopenmp"]
F = np.float32
EMPTY = 0xFFFFFFFF

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
        L.ref_denoise.argtypes = [vp, vp, vp, vp, i32, i32, i32, f32, f32, i32, vp, vp]
        L.ref_denoise.restype = C.c_int
        L.ref_denoise_constants.argtypes = [i32, f32, f32, C.c_int, vp, vp]
        L.ref_denoise_constants.restype = C.c_int
        _lib = L
    return _lib


def constants(passes, sigma_color, sigma_position, position_given=True):
    """(rc, kc[passes], kp[passes]); rc -1: the call is ATR_E_INVALID by the kc/kp rule."""
    kc, kp = np.zeros(passes, F), np.zeros(passes, F)
    rc = lib().ref_denoise_constants(passes, sigma_color, sigma_position, 1 if position_given else 0, kc.ctypes.data,
                                     kp.ctypes.data)
    return rc, kc, kp


def denoise(color, normal=None, position=None, ident=None, passes=5, sigma_color=0.01, sigma_position=0.0,
            normal_power_log2=5):
    """The reference's (out (H, W, 3) float32, framebuffer (H, W) uint32) for (H, W, 3) float32 images and
    an (H, W) ident of 32-bit integers; None where the kc/kp rule rejects the call."""
    c = np.ascontiguousarray(color, F)
    h, w = c.shape[:2]
    assert c.shape == (h, w, 3)
    g = [None if a is None else np.ascontiguousarray(a, F) for a in (normal, position)]
    for a in g:
        assert a is None or a.shape == (h, w, 3)
    idt = None if ident is None else np.ascontiguousarray(ident).view(np.uint32)
    assert idt is None or idt.shape == (h, w)
    out, fb = np.full((h, w, 3), np.nan, F), np.zeros((h, w), np.uint32)
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = lib().ref_denoise(c.ctypes.data, ptr(g[0]), ptr(g[1]), ptr(idt), w, h, passes, sigma_color, sigma_position,
                           normal_power_log2, out.ctypes.data, fb.ctypes.data)
    return (out, fb) if rc == 0 else None


def same_bits(a, b):
    """Bit equality of two arrays; a NaN equals a NaN (the sign and payload of a generated NaN are the
    processor's, not the contract's)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f":
        ua, ub = a.view(np.uint32), b.view(np.uint32)
        return bool(np.all((ua == ub) | (np.isnan(a) & np.isnan(b))))
    return bool(np.array_equal(a.astype(np.int64), b.astype(np.int64)))
