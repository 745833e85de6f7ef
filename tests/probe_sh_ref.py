"""The light probes' reference for the tests (tests/c/probe_sh_ref.c): the sphere sampler on the oracle's
own stream, then the oracle's own cast_ray from the probe on that same state, projected per probe on
the nine basis functions in sample order; built with gcc and the oracle Makefile's flags into
atray_amd/_lib/ and bound with ctypes. Takes an oracle.Scene. Also a numpy float32 restatement of the
basis and of the ordered sums."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "probe_sh_ref.c")
DEPS = [SRC] + [os.path.join(ROOT, "tests", "c", f) for f in ("radiance_ref.c", "gather_ref.c", "occlusion_ref.c")] + [
    os.path.join(ROOT, "oracle", "atr_oracle.c"), os.path.join(ROOT, "oracle", "atr_oracle.h")]
LIB_PATH = os.path.join(ROOT, "atray_amd", "_lib", "libprobe_sh_ref.so")
FLAGS = ["-O2", "-std=c11", "-ffp-contract=off", "-fno-fast-math", "-fPIC"]
F = np.float32
SENTINEL = 0xABABABAB  # what the reference leaves where it writes nothing (an invalid probe, first > 0)
UNTRACED = 0xFFFFFFFF  # sample_casts of a sample of an invalid probe
MAX_TRIES = 32         # the library's (engine.h kProbeTries)
TRI, SPHERE, PLANE, SKY = 1, 2, 3, 4  # first_kind: the oracle's OT_*

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
        L.ref_probe_sh.argtypes = [vp, vp, i64, i32, u32, i64, i32, u64, i32] + [vp] * 9
        L.ref_probe_sh.restype = i64
        L.ref_probe_directions.argtypes = [i64, i32, u32, i64, u64, i32, vp, vp]
        L.ref_probe_directions.restype = None
        _lib = L
    return _lib


def directions(npoints, nsamples, first_sample=0, point_base=0, seed=0, max_tries=MAX_TRIES):
    """The sampler alone: (dirs (n, nsamples, 3) float32, tries (n, nsamples) uint8)."""
    d = np.full((npoints, nsamples, 3), np.nan, F)
    t = np.full((npoints, nsamples), 255, np.uint8)
    lib().ref_probe_directions(npoints, nsamples, first_sample, point_base, seed, max_tries, d.ctypes.data, t.ctypes.data)
    return d, t


def probe_sh(scene, points, nsamples, bounces, seed=0, first_sample=0, point_base=0, start=None, max_tries=MAX_TRIES):
    """The reference's outputs on an oracle.Scene, as a dict: sh, sum (n, 27) float32 (index 3 k + c);
    ray_casts (n,) uint32; invalid (n,) uint8; sample_rgb, dirs (n, nsamples, 3) float32; tries (n,
    nsamples) uint8; sample_casts (n, nsamples) uint32 (cast_ray's count, UNTRACED for an invalid probe);
    first_kind (n, nsamples) uint8 (TRI, SPHERE, PLANE, SKY; 0 for an invalid probe); traced (what
    atr_probe_sh adds to traced_rays: the oracle's n_rays). start: the earlier range's sum and ray_casts
    when first_sample > 0 (copied, not changed). Where the reference writes nothing the per-probe arrays
    hold SENTINEL bits."""
    p = np.ascontiguousarray(points, F)
    n = len(p)
    assert p.shape == (n, 3)
    start = start or {}
    if first_sample > 0:
        assert "sum" in start
    s = np.array(start["sum"], F).reshape(n, 27) if "sum" in start else np.full((n, 27), SENTINEL, np.uint32).view(F)
    c = (np.array(start["ray_casts"], np.uint32).reshape(n) if "ray_casts" in start
         else np.full(n, 0 if first_sample > 0 else SENTINEL, np.uint32))
    sh = np.full((n, 27), SENTINEL, np.uint32).view(F)
    inv = np.full(n, 0xAB, np.uint8)
    srgb = np.full((n, nsamples, 3), np.nan, F)
    dirs = np.full((n, nsamples, 3), np.nan, F)
    tries = np.full((n, nsamples), 255, np.uint8)
    sc = np.full((n, nsamples), 0xFFFFFFFE, np.uint32)
    kind = np.full((n, nsamples), 255, np.uint8)
    n_rays = lib().ref_probe_sh(C.addressof(scene.s), p.ctypes.data, n, nsamples, first_sample, point_base, bounces,
                                seed, max_tries, s.ctypes.data, c.ctypes.data, sh.ctypes.data, inv.ctypes.data,
                                srgb.ctypes.data, dirs.ctypes.data, tries.ctypes.data, sc.ctypes.data, kind.ctypes.data)
    return {"sh": sh, "sum": s, "ray_casts": c, "invalid": inv, "sample_rgb": srgb, "dirs": dirs, "tries": tries,
            "sample_casts": sc, "first_kind": kind, "traced": int(n_rays)}


# ---- numpy float32 restatements ---------------------------------------------------------------------------

def np_basis(dirs):
    """Y0..Y8 of (..., 3) float32 directions, every product rounded to float32 on its own: (..., 9)."""
    d = np.asarray(dirs, F)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    c1, c2, c6, c8 = F(0.488602512), F(1.092548431), F(0.315391565), F(0.546274215)
    out = np.empty(d.shape[:-1] + (9,), F)
    out[..., 0] = F(0.282094792)
    out[..., 1] = c1 * y
    out[..., 2] = c1 * z
    out[..., 3] = c1 * x
    out[..., 4] = c2 * (x * y)
    out[..., 5] = c2 * (y * z)
    out[..., 6] = c6 * ((F(3.0) * (z * z)) - F(1.0))
    out[..., 7] = c2 * (x * z)
    out[..., 8] = c8 * ((x * x) - (y * y))
    return out


def np_sums(sample_rgb, dirs, start=None):
    """The 27 ordered sums of (n, ns, 3) colours on (n, ns, 3) directions, (n, 27) float32 at index
    3 k + c: for each sample in order sum = sum + (colour.c * Yk), vectorised over probes only."""
    rgb, y = np.asarray(sample_rgb, F), np_basis(dirs)
    n, ns = rgb.shape[:2]
    acc = np.zeros((n, 9, 3), F) if start is None else np.array(start, F).reshape(n, 9, 3)
    for s in range(ns):
        acc = (acc + (y[:, s, :, None] * rgb[:, s, None, :]).astype(F)).astype(F)
    return acc.reshape(n, 27)


def np_sh(sums, total):
    """sh from the sums: (sum * 12.566370614f) / float(total)."""
    return ((np.asarray(sums, F) * F(12.566370614)).astype(F) / F(total)).astype(F)
