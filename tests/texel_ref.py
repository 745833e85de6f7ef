"""The lightmap texels' reference for the tests (tests/c/texel_ref.c): a plain loop over the faces in
ascending order and over all texels with the formulas of include/atray.h, and the dilation of
atr_texels_to_image; built with gcc into atray_amd/_lib/ and bound with ctypes. Takes the mesh as
Mesh.arrays() returns it."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "texel_ref.c")
LIB_PATH = os.path.join(ROOT, "atray_amd", "_lib", "libtexel_ref.so")
FLAGS = ["-O2", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-fopenmp"]
F = np.float32
KEYS = ("slot", "texel", "face", "bary", "point", "normal")

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
        vp, i64, i32, u32 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32
        L.ref_mesh_texels.argtypes = [vp, u32, vp, u32, vp, u32, vp, vp, vp, u32, i32, i32, i32] + [vp] * 6
        L.ref_mesh_texels.restype = i64
        L.ref_texels_to_image.argtypes = [vp, vp, i64, i32, i32, i32, vp, vp]
        L.ref_texels_to_image.restype = None
        _lib = L
    return _lib


def mesh_texels(arrays, width, height, flip=False):
    """The reference's outputs for the mesh `arrays` (Mesh.arrays()) as a dict: slot (height * width,)
    int32; per covered k texel (n,) int32, face (n,) uint32, bary (n, 2), point (n, 3), normal (n, 3)
    float32."""
    V, N, T, FV, FT, FN = (np.ascontiguousarray(a) for a in arrays)
    n = width * height
    slot, texel, face = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.uint32)
    bary, point, normal = np.zeros((n, 2), F), np.zeros((n, 3), F), np.zeros((n, 3), F)
    cnt = lib().ref_mesh_texels(V.ctypes.data, len(V), N.ctypes.data, len(N), T.ctypes.data, len(T), FV.ctypes.data,
                                FT.ctypes.data, FN.ctypes.data, len(FV), width, height, 1 if flip else 0,
                                slot.ctypes.data, texel.ctypes.data, face.ctypes.data, bary.ctypes.data,
                                point.ctypes.data, normal.ctypes.data)
    return {"slot": slot, "texel": texel[:cnt].copy(), "face": face[:cnt].copy(), "bary": bary[:cnt].copy(),
            "point": point[:cnt].copy(), "normal": normal[:cnt].copy()}


def texels_to_image(values, texel, width, height, passes=2, fill=(0, 0, 0)):
    """The reference's (height, width, 3) float32 image."""
    v, t = np.ascontiguousarray(values, F).reshape(-1, 3), np.ascontiguousarray(texel, np.int32)
    assert len(v) == len(t)
    f = np.array(fill, F)
    img = np.full((height, width, 3), np.nan, F)
    lib().ref_texels_to_image(v.ctypes.data, t.ctypes.data, len(t), width, height, passes, f.ctypes.data,
                              img.ctypes.data)
    return img


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
