"""The occlusion query's reference for the tests (tests/c/occlusion_ref.c): the oracle's traversal
with its closest distance started at each ray's t_max, built with gcc and the oracle Makefile's
flags into atray_amd/_lib/ and bound with ctypes. Takes an oracle.Scene."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "occlusion_ref.c")
DEPS = [SRC, os.path.join(ROOT, "oracle", "atr_oracle.c"), os.path.join(ROOT, "oracle", "atr_oracle.h")]
LIB_PATH = os.path.join(ROOT, "atray_amd", "_lib", "libocclusion_ref.so")
FLAGS = ["-O2", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fPIC"]
F = np.float32
MAX_FLOAT = np.float32(3.402823466e38)

_lib = None


def build():
    if os.path.exists(LIB_PATH) and all(os.path.getmtime(LIB_PATH) >= os.path.getmtime(d) for d in DEPS):
        return LIB_PATH
    os.makedirs(os.path.dirname(LIB_PATH), exist_ok=True)
    tmp = f"{LIB_PATH}.{os.getpid()}.tmp"
    subprocess.run(["gcc"] + FLAGS + ["-shared", "-pthread", "-o", tmp, SRC, "-lm"], check=True)
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.ref_occluded.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        L.ref_occluded.restype = None
        _lib = L
    return _lib


def random_tmax(t_ref, seed=7):
    """The tests' random bounds around a closest-hit trace: t_ref x U(0.25, 1.75) for the rays that
    hit, 10 x U(0.1, 3) for the misses (float32)."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.25, 1.75, len(t_ref)).astype(F)
    b = rng.uniform(0.1, 3.0, len(t_ref)).astype(F)
    hit = t_ref < MAX_FLOAT
    return np.where(hit, np.where(hit, t_ref, F(1.0)) * a, F(10.0) * b).astype(F)


def occluded(scene, orig, dirs, t_max=None, found=False):
    """ref_occluded on an oracle.Scene: the byte per ray (0 visible, 1 occluded, 2 bad t_max) and,
    with found, a witness t below t_max for each occluded ray (MAX_FLOAT otherwise). The rays must
    pass the query's validity test; t_max None means unbounded."""
    orig, dirs = np.ascontiguousarray(orig, F), np.ascontiguousarray(dirs, F)
    n = len(orig)
    assert orig.shape == (n, 3) and dirs.shape == (n, 3)
    tm = None
    if t_max is not None:
        tm = np.ascontiguousarray(t_max, F)
        assert tm.shape == (n,)
    out = np.full(n, 255, np.uint8)
    tf = np.empty(n, F)
    lib().ref_occluded(C.addressof(scene.s), orig.ctypes.data, dirs.ctypes.data,
                       tm.ctypes.data if tm is not None else None, n, out.ctypes.data, tf.ctypes.data)
    return (out, tf) if found else out
