"""The hemisphere gather's reference for the tests (tests/c/gather_ref.c): the sampler restated with the
oracle's RNG in C f32 and the occlusion reference's walk per traced sample, built with gcc and the
oracle Makefile's flags into atray_amd/_lib/ and bound with ctypes. Takes an oracle.Scene."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "gather_ref.c")
DEPS = [SRC, os.path.join(ROOT, "tests", "c", "occlusion_ref.c"), os.path.join(ROOT, "oracle", "atr_oracle.c"),
        os.path.join(ROOT, "oracle", "atr_oracle.h")]
LIB_PATH = os.path.join(ROOT, "atray_amd", "_lib", "libgather_ref.so")
FLAGS = ["-O2", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fPIC"]
F = np.float32

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
        vp, i64, i32, u32, u64 = C.c_void_p, C.c_int64, C.c_int32, C.c_uint32, C.c_uint64
        L.ref_gather_directions.argtypes = [vp, i64, i32, u32, i64, u64, vp, vp]
        L.ref_gather_directions.restype = None
        L.ref_gather.argtypes = [vp, vp, vp, vp, i64, i32, u32, i64, u64, vp, vp, vp, vp, vp]
        L.ref_gather.restype = i64
        _lib = L
    return _lib


def directions(normals, nsamples, first_sample=0, point_base=0, seed=0):
    """(dirs (n, nsamples, 3) float32, traced (n, nsamples) uint8) of the reference's sampler."""
    nrm = np.ascontiguousarray(normals, F)
    n = len(nrm)
    assert nrm.shape == (n, 3)
    dirs = np.full((n, nsamples, 3), np.nan, F)
    traced = np.full((n, nsamples), 255, np.uint8)
    lib().ref_gather_directions(nrm.ctypes.data, n, nsamples, first_sample, point_base, seed, dirs.ctypes.data,
                                traced.ctypes.data)
    return dirs, traced


def gather(scene, points, normals, nsamples, t_max=None, first_sample=0, point_base=0, seed=0):
    """The reference's five outputs on an oracle.Scene, as a dict: visible, occluded (n,) uint32, mask
    (n, ceil(nsamples / 32)) uint32, dirs (n, nsamples, 3) float32, traced (the count), and the
    per-sample traced flags as `flags`."""
    p, nrm = np.ascontiguousarray(points, F), np.ascontiguousarray(normals, F)
    n = len(p)
    assert p.shape == (n, 3) and nrm.shape == (n, 3)
    tm = None
    if t_max is not None:
        tm = np.ascontiguousarray(t_max, F)
        assert tm.shape == (n,)
    words = (nsamples + 31) // 32
    dirs = np.full((n, nsamples, 3), np.nan, F)
    flags = np.full((n, nsamples), 255, np.uint8)
    vis, occ = np.full(n, 0xFFFFFFFF, np.uint32), np.full(n, 0xFFFFFFFF, np.uint32)
    mask = np.full((n, words), 0xFFFFFFFF, np.uint32)
    traced = lib().ref_gather(C.addressof(scene.s), p.ctypes.data, nrm.ctypes.data,
                              tm.ctypes.data if tm is not None else None, n, nsamples, first_sample, point_base,
                              seed, dirs.ctypes.data, flags.ctypes.data, vis.ctypes.data, occ.ctypes.data,
                              mask.ctypes.data)
    return {"visible": vis, "occluded": occ, "mask": mask, "dirs": dirs, "traced": int(traced), "flags": flags}
