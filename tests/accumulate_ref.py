"""The temporal accumulator's reference for the tests (tests/c/accumulate_ref.c): atr_accumulate's
contract of include/atray.h as a plain loop; built with gcc into atray_amd/_lib/ and bound with ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.denoise_ref import same_bits  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "accumulate_ref.c")
LIB_PATH = os.path.join(ROOT, "atray_amd", "_lib", "libaccumulate_ref.so")
FLAGS = ["-O2", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-fopenmp"]
F = np.float32
EMPTY = 0xFFFFFFFF
DEFAULTS = dict(alpha=0.0, alpha_moments=0.0, max_length=64, plane_tolerance=0.02, min_normal_dot=0.9)

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
        L.ref_accumulate.argtypes = [vp, vp, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp, vp, i32, i32, f32, f32, i32, f32,
                                     f32, vp, vp, vp, vp, vp]
        L.ref_accumulate.restype = None
        _lib = L
    return _lib


def cam_floats(cam):
    """An atr_camera (or anything with its fields) as the reference's 13 floats: eye, camera_x, camera_y,
    camera_z and k = h_fov * aspect_ratio, the product rounded to f32."""
    v = lambda a: [a.x, a.y, a.z]  # noqa: E731
    k = F(cam.h_fov) * F(cam.aspect_ratio)
    return np.array(v(cam.eye) + v(cam.camera_x) + v(cam.camera_y) + v(cam.camera_z) + [k], F)


def accumulate(color, guides=(None, None, None), prev=None, moments=True, **params):
    """The reference's result for (H, W, 3) float32 colour, guides = (normal, position, ident) arrays or
    None each, and prev = None or a dict with "cam" (13 floats, or an atr_camera), "guides" (the previous
    frame's triple), "color", "moments" (or None), "length". Returns a dict of color (H, W, 3), moments
    (H, W, 2) or None, length (H, W) uint32, variance (H, W) or None, framebuffer (H, W) uint32. The
    arguments are taken as valid (atray.h's rules are the entry point's)."""
    kw = dict(DEFAULTS, **params)
    c = np.ascontiguousarray(color, F)
    h, w = c.shape[:2]
    assert c.shape == (h, w, 3)

    def f3(a):
        a = None if a is None else np.ascontiguousarray(a, F)
        assert a is None or a.shape == (h, w, 3)
        return a

    def u1(a):
        a = None if a is None else np.ascontiguousarray(a).view(np.uint32)
        assert a is None or a.shape == (h, w)
        return a

    nrm, pos, idt = f3(guides[0]), f3(guides[1]), u1(guides[2])
    cam = pn = pp = pi = pc = pm = pl = None
    if prev is not None:
        cam = prev["cam"]
        cam = np.ascontiguousarray(cam, F) if isinstance(cam, np.ndarray) else cam_floats(cam)
        assert cam.shape == (13,)
        pn, pp, pi = f3(prev["guides"][0]), f3(prev["guides"][1]), u1(prev["guides"][2])
        pc, pl = f3(prev["color"]), u1(prev["length"])
        pm = prev.get("moments")
        if pm is not None:
            pm = np.ascontiguousarray(pm, F)
            assert pm.shape == (h, w, 2)
        assert pos is not None and pp is not None and (pm is not None) == bool(moments)
        assert (nrm is None) == (pn is None) and (idt is None) == (pi is None)
    out = {"color": np.full((h, w, 3), np.nan, F), "moments": np.full((h, w, 2), np.nan, F) if moments else None,
           "length": np.full((h, w), 0xABABABAB, np.uint32), "variance": np.full((h, w), np.nan, F) if moments else None,
           "framebuffer": np.zeros((h, w), np.uint32)}
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    lib().ref_accumulate(ptr(c), ptr(nrm), ptr(pos), ptr(idt), 0 if prev is None else 1, ptr(cam), ptr(pn), ptr(pp),
                         ptr(pi), ptr(pc), ptr(pm), ptr(pl), w, h, kw["alpha"], kw["alpha_moments"], kw["max_length"],
                         kw["plane_tolerance"], kw["min_normal_dot"], ptr(out["color"]), ptr(out["moments"]),
                         ptr(out["length"]), ptr(out["variance"]), ptr(out["framebuffer"]))
    return out


def history(out, cam, guides):
    """The `prev` of the next call: a result, the camera it was rendered from and its guides."""
    return {"cam": cam, "guides": guides, "color": out["color"], "moments": out["moments"], "length": out["length"]}
