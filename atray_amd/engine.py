"""ctypes binding of the C-ABI in ``include/atray.h`` (``atray_amd/_lib/libatray_hip.so``).

The HIP library is the product path: there is no CPU fallback. Loading fails loudly if the
library was not built (``__graft_entry__.build()`` / ``make -C atray_amd/csrc``).

torch is imported before the library is loaded so that both bind the same HIP runtime
(torch's bundled ``libamdhip64.so`` carries the SONAME ``libamdhip64.so.7`` that the library
needs); torch then provides device memory, streams and ``torch.distributed`` (RCCL).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ATRAY_LIB") or os.path.join(HERE, "_lib", "libatray_hip.so")  # ATRAY_LIB: experiment builds only

ATR_LAYOUT_IMAGE = 0
ATR_LAYOUT_PACKED = 1
ATR_PLAN_PRIO = 0x80  # cell plan: raised issue priority (atr_set_cell_plan)


def plan_class(c):
    """Cell plan dispatch class (ATR_PLAN_CLASS): class 7 cells are dispatched first, class 0 last."""
    return (int(c) & 7) << 4
ATR_KERNEL_AUTO, ATR_KERNEL_LANE = 0, 1
ATR_KERNEL_FLAT = 8
ATR_KERNEL_HYBRID = 9
ATR_KERNEL_PATHS = 10
# the kernel variants of the shipping library (atray.h); AUTO picks HYBRID or PATHS
VARIANTS = (ATR_KERNEL_LANE, ATR_KERNEL_FLAT, ATR_KERNEL_HYBRID, ATR_KERNEL_PATHS)
MISS = 0xFFFFFFFF
ATR_SAMPLES_CONVERGED = 0x80000000  # sample_count bit 31: the pixel has stopped (atr_render_start_adaptive)
MAX_FLOAT = np.float32(3.402823466e38)
# atr_trace_rays: what a ray met (atr_ray_hits.kind)
ATR_RAY_SKY, ATR_RAY_TRI, ATR_RAY_SPHERE, ATR_RAY_PLANE, ATR_RAY_INVALID = 0, 1, 2, 3, 4
# atr_occluded_rays: the byte of a ray
ATR_OCCL_VISIBLE, ATR_OCCL_OCCLUDED, ATR_OCCL_INVALID = 0, 1, 2
ATR_TEXELS_FLIP = 1  # atr_mesh_texels: negate every normal
ATR_DENOISE_EMPTY = 0xFFFFFFFF  # atr_denoise_guides.ident: an inert pixel (-1 in an int32 tensor)

ERRORS = {-1: "ATR_E_INVALID", -2: "ATR_E_IO", -3: "ATR_E_NOMEM", -4: "ATR_E_NOSCENE",
          -5: "ATR_E_TREE_DEPTH", -6: "ATR_E_TREE_LAYOUT"}


class AtrError(RuntimeError):
    pass


def check(rc, what=""):
    if rc < 0:
        name = ERRORS.get(rc) or (f"hipError {-rc - 1000}" if rc <= -1000 else str(rc))
        raise AtrError(f"{what}: {name}")
    return rc


class atr_vec3(C.Structure):
    _fields_ = [("x", C.c_float), ("y", C.c_float), ("z", C.c_float)]


class atr_material(C.Structure):
    _fields_ = [("emission", atr_vec3), ("reflection", atr_vec3), ("scatter", C.c_float)]


class atr_model(C.Structure):
    _fields_ = [("mesh", C.c_void_p), ("tree", C.c_void_p), ("surrounding_aabb", C.c_float * 6),
                ("material", C.c_int32)]


class atr_sphere(C.Structure):
    _fields_ = [("center", atr_vec3), ("radius", C.c_float), ("material", C.c_int32)]


class atr_plane(C.Structure):
    _fields_ = [("normal", atr_vec3), ("distance", C.c_float), ("material", C.c_int32)]


class atr_camera(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("anti_aliasing", C.c_int32),
                ("samples_per_pixel", C.c_uint32), ("bounce_limit", C.c_int32),
                ("aspect_ratio", C.c_float), ("camera_z", atr_vec3), ("camera_x", atr_vec3),
                ("camera_y", atr_vec3), ("eye", atr_vec3), ("frame_center", atr_vec3),
                ("h_fov", C.c_float), ("half_pixel_width", C.c_float),
                ("half_pixel_height", C.c_float)]


class atr_tile(C.Structure):
    _fields_ = [("min_x", C.c_int32), ("min_y", C.c_int32), ("max_x", C.c_int32),
                ("max_y", C.c_int32)]


class atr_frame(C.Structure):
    _fields_ = [("layout", C.c_int32), ("framebuffer", C.c_void_p), ("hit_face", C.c_void_p),
                ("hit_t", C.c_void_p), ("rgb", C.c_void_p), ("ray_casts", C.c_void_p),
                ("traced_rays", C.c_void_p)]


class atr_ray_hits(C.Structure):
    _fields_ = [("t", C.c_void_p), ("face", C.c_void_p), ("model", C.c_void_p), ("uv", C.c_void_p),
                ("kind", C.c_void_p), ("material", C.c_void_p), ("normal", C.c_void_p),
                ("traced_rays", C.c_void_p)]


class atr_gather_out(C.Structure):
    _fields_ = [("visible", C.c_void_p), ("occluded", C.c_void_p), ("mask", C.c_void_p), ("dirs", C.c_void_p),
                ("traced_rays", C.c_void_p)]


class atr_radiance_out(C.Structure):
    _fields_ = [("rgb", C.c_void_p), ("sum", C.c_void_p), ("ray_casts", C.c_void_p), ("invalid", C.c_void_p),
                ("traced_rays", C.c_void_p)]


class atr_gather_radiance_out(C.Structure):
    _fields_ = [("rgb", C.c_void_p), ("sum", C.c_void_p), ("samples", C.c_void_p), ("ray_casts", C.c_void_p),
                ("invalid", C.c_void_p), ("sample_rgb", C.c_void_p), ("dirs", C.c_void_p),
                ("traced_rays", C.c_void_p)]


class atr_probe_sh_out(C.Structure):
    _fields_ = [("sh", C.c_void_p), ("sum", C.c_void_p), ("ray_casts", C.c_void_p), ("invalid", C.c_void_p),
                ("sample_rgb", C.c_void_p), ("dirs", C.c_void_p), ("traced_rays", C.c_void_p)]


class atr_texels_out(C.Structure):
    _fields_ = [("slot", C.c_void_p), ("texel", C.c_void_p), ("face", C.c_void_p), ("bary", C.c_void_p),
                ("point", C.c_void_p), ("normal", C.c_void_p)]


class atr_denoise_params(C.Structure):
    _fields_ = [("passes", C.c_int32), ("sigma_color", C.c_float), ("sigma_position", C.c_float),
                ("normal_power_log2", C.c_int32), ("reserved", C.c_int32 * 4)]


class atr_denoise_guides(C.Structure):
    _fields_ = [("normal", C.c_void_p), ("position", C.c_void_p), ("ident", C.c_void_p)]


class atr_guides_out(C.Structure):
    _fields_ = [("normal", C.c_void_p), ("position", C.c_void_p), ("ident", C.c_void_p), ("depth", C.c_void_p),
                ("material", C.c_void_p)]


class atr_history(C.Structure):
    _fields_ = [("color", C.c_void_p), ("moments", C.c_void_p), ("length", C.c_void_p)]


class atr_accumulate_params(C.Structure):
    _fields_ = [("alpha", C.c_float), ("alpha_moments", C.c_float), ("max_length", C.c_int32),
                ("plane_tolerance", C.c_float), ("min_normal_dot", C.c_float), ("reserved", C.c_int32 * 3)]


class atr_denoise_variance_params(C.Structure):
    _fields_ = [("passes", C.c_int32), ("sigma_luminance", C.c_float), ("luminance_floor", C.c_float),
                ("sigma_position", C.c_float), ("normal_power_log2", C.c_int32), ("spatial_below", C.c_int32),
                ("reserved", C.c_int32 * 2)]


class atr_tuning(C.Structure):
    _fields_ = [("xcd_chunk", C.c_int32), ("frame_rotate", C.c_int32), ("hybrid_a", C.c_int32),
                ("hybrid_b", C.c_int32), ("path_batch_log2", C.c_int32), ("cluster_size", C.c_int32),
                ("frame_plan", C.c_int32), ("path_camera_occ", C.c_int32), ("path_bounce_occ", C.c_int32),
                ("primary_occ", C.c_int32), ("path_sort_bits", C.c_int32), ("path_split", C.c_int32),
                ("reserved", C.c_int32 * 4)]


# every symbol include/atray.h declares (checked by tests/test_capi_symbols.py)
EXPORTS = [
    "atr_mesh_load_obj", "atr_mesh_parse_obj", "atr_mesh_from_arrays", "atr_mesh_free",
    "atr_mesh_info", "atr_mesh_aabb", "atr_mesh_translate_to", "atr_octree_build", "atr_octree_build_device",
    "atr_octree_from_nodes", "atr_octree_free", "atr_octree_export", "atr_octree_stats", "atr_camera_set",
    "atr_make_tiles", "atr_make_shard_tiles", "atr_create", "atr_destroy", "atr_version",
    "atr_scene_upload", "atr_scene_info", "atr_render_start", "atr_render_start_ex",
    "atr_render_counters", "atr_render_tile_costs", "atr_balance_shard_tiles",
    "atr_render_packed_size", "atr_packed_pixel_map", "atr_unpack", "atr_tile_ray_casts", "atr_render_wait",
    "atr_last_kernel_ms", "atr_device_alloc", "atr_device_free", "atr_memcpy_d2h", "atr_memcpy_h2d",
    "atr_memset_d", "atr_render_start_progressive", "atr_write_bmp", "atr_render_start_frames",
    "atr_render_start_cameras", "atr_mesh_load_obj_threaded", "atr_mesh_parse_obj_threaded",
    "atr_mesh_export", "atr_packed_tile_ray_casts", "atr_set_cell_plan", "atr_render_cell_costs",
    "atr_default_tuning", "atr_set_tuning", "atr_get_tuning", "atr_pack_bgr", "atr_scatter_bgr",
    "atr_pack_bgr_masked_bound", "atr_pack_bgr_masked", "atr_scatter_bgr_masked", "atr_unpack_masked",
    "atr_unpack_masked_ranks",
    "atr_render_plan_info", "atr_workspace_info", "atr_render_start_samples",
    "atr_render_start_adaptive", "atr_render_adaptive_info", "atr_render_cull_counters",
    "atr_trace_rays", "atr_occluded_rays", "atr_gather_occlusion", "atr_gather_directions",
    "atr_radiance_rays", "atr_gather_radiance", "atr_mesh_texels", "atr_texels_to_image",
    "atr_render_fold_counters", "atr_camera_pads_row", "atr_default_denoise_params", "atr_denoise",
    "atr_render_leaf_box_counters", "atr_camera_leaf_boxes_row",
    "atr_render_sky_cells", "atr_scene_sky_record", "atr_sky_record_host",
    "atr_default_accumulate_params", "atr_accumulate_check", "atr_accumulate",
    "atr_default_denoise_variance_params", "atr_denoise_variance_check", "atr_denoise_variance",
    "atr_camera_rays_host", "atr_camera_rays", "atr_camera_guides",
    "atr_probe_sh", "atr_probe_directions", "atr_sh_basis",
]
# the diagnostic build's extra symbols (include/atray_diag.h; make -C atray_amd/csrc DIAG=1)
DIAG_EXPORTS = ["atr_render_wave_trace", "atr_render_phase_clocks", "atr_render_path_counters",
                "atr_render_simd_counters"]

_lib = None


def lib():
    """Load the HIP engine library (torch first: shared HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (binds libamdhip64.so.7 before our library needs it)
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"atray HIP engine not built: {LIB_PATH} missing "
                          "(run __graft_entry__.build())")
    L = C.CDLL(LIB_PATH)
    P, vp, i32, u32, i64 = C.POINTER, C.c_void_p, C.c_int32, C.c_uint32, C.c_int64
    sig = {
        "atr_mesh_load_obj": ([C.c_char_p, P(vp)], C.c_int),
        "atr_mesh_parse_obj": ([C.c_char_p, C.c_size_t, P(vp)], C.c_int),
        "atr_mesh_load_obj_threaded": ([C.c_char_p, i32, P(vp)], C.c_int),
        "atr_mesh_parse_obj_threaded": ([C.c_char_p, C.c_size_t, i32, P(vp)], C.c_int),
        "atr_mesh_from_arrays": ([vp, u32, vp, u32, vp, u32, vp, P(vp)], C.c_int),
        "atr_mesh_free": ([vp], None),
        "atr_mesh_info": ([vp, P(u32), P(u32), P(u32)], C.c_int),
        "atr_mesh_export": ([vp, vp, vp, vp, P(u32), vp, vp, vp], C.c_int),
        "atr_mesh_aabb": ([vp, C.c_float * 6], C.c_int),
        "atr_mesh_translate_to": ([vp, C.c_float * 6, atr_vec3], C.c_int),
        "atr_octree_build": ([vp, u32, P(vp)], C.c_int),
        "atr_octree_build_device": ([vp, u32, i32, P(vp), vp], C.c_int),
        "atr_octree_from_nodes": ([i32, vp, vp, vp, vp, u32, vp, vp, P(vp)], C.c_int),
        "atr_octree_free": ([vp], None),
        "atr_octree_export": ([vp, vp, vp, vp, vp, vp, vp], C.c_int),
        "atr_octree_stats": ([vp, i64 * 7], C.c_int),
        "atr_camera_set": ([P(atr_camera), atr_vec3, atr_vec3, i32, i32, i32, u32, i32, C.c_float], C.c_int),
        "atr_make_tiles": ([i32, i32, i32, vp, i32], i32),
        "atr_make_shard_tiles": ([i32, i32, i32, i32, i32, vp, i32], i32),
        "atr_balance_shard_tiles": ([i32, i32, i32, i32, vp, i64, vp], i32),
        "atr_create": ([C.c_int, P(vp)], C.c_int),
        "atr_destroy": ([vp], C.c_int),
        "atr_version": ([], C.c_char_p),
        "atr_scene_upload": ([vp, vp, i32, vp, i32, vp, i32, vp, i32], C.c_int),
        "atr_scene_info": ([vp, P(i64), P(i32), P(i32)], C.c_int),
        "atr_workspace_info": ([vp, P(i32), P(i64)], C.c_int),
        "atr_render_start": ([vp, P(atr_camera), vp, i32, P(atr_frame), C.c_uint64, vp], C.c_int),
        "atr_render_start_ex": ([vp, P(atr_camera), vp, i32, P(atr_frame), C.c_uint64, vp, i32], C.c_int),
        "atr_render_start_samples": ([vp, P(atr_camera), vp, i32, P(atr_frame), C.c_uint64, vp, i32, u32, vp],
                                     C.c_int),
        "atr_render_start_adaptive": ([vp, P(atr_camera), vp, i32, P(atr_frame), C.c_uint64, vp, i32, u32, vp, vp,
                                       C.c_float], C.c_int),
        "atr_render_adaptive_info": ([vp, i64 * 4], C.c_int),
        "atr_trace_rays": ([vp, vp, vp, i64, P(atr_ray_hits), i32, i32, vp], C.c_int),
        "atr_occluded_rays": ([vp, vp, vp, vp, i64, vp, vp, i32, i32, vp], C.c_int),
        "atr_gather_occlusion": ([vp, vp, vp, vp, i64, i32, u32, i64, C.c_uint64, P(atr_gather_out), i32, vp],
                                 C.c_int),
        "atr_gather_directions": ([vp, i64, i32, u32, i64, C.c_uint64, vp, vp], C.c_int),
        "atr_radiance_rays": ([vp, vp, vp, i64, i32, u32, i64, i32, C.c_uint64, P(atr_radiance_out), i32, vp],
                              C.c_int),
        "atr_gather_radiance": ([vp, vp, vp, i64, i32, u32, i64, i32, C.c_uint64, P(atr_gather_radiance_out), i32,
                                 vp], C.c_int),
        "atr_probe_sh": ([vp, vp, i64, i32, u32, i64, i32, C.c_uint64, P(atr_probe_sh_out), i32, vp], C.c_int),
        "atr_probe_directions": ([i64, i32, u32, i64, C.c_uint64, vp, vp], C.c_int),
        "atr_sh_basis": ([vp, i64, vp], C.c_int),
        "atr_mesh_texels": ([vp, vp, i32, i32, i32, i64, P(atr_texels_out), P(i64), vp], C.c_int),
        "atr_texels_to_image": ([vp, vp, vp, i64, i32, i32, i32, C.c_float * 3, vp, vp], C.c_int),
        "atr_default_denoise_params": ([P(atr_denoise_params)], None),
        "atr_denoise": ([vp, vp, P(atr_denoise_guides), i32, i32, P(atr_denoise_params), vp, vp, vp], C.c_int),
        "atr_default_accumulate_params": ([P(atr_accumulate_params)], None),
        "atr_accumulate_check": ([vp, P(atr_denoise_guides), P(atr_camera), P(atr_denoise_guides), P(atr_history), i32,
                                  i32, P(atr_accumulate_params), P(atr_history), vp], C.c_int),
        "atr_accumulate": ([vp, vp, P(atr_denoise_guides), P(atr_camera), P(atr_denoise_guides), P(atr_history), i32,
                            i32, P(atr_accumulate_params), P(atr_history), vp, vp, vp], C.c_int),
        "atr_default_denoise_variance_params": ([P(atr_denoise_variance_params)], None),
        "atr_denoise_variance_check": ([vp, vp, P(atr_denoise_guides), vp, vp, i32, i32,
                                        P(atr_denoise_variance_params), vp, vp, vp], C.c_int),
        "atr_denoise_variance": ([vp, vp, vp, P(atr_denoise_guides), vp, vp, i32, i32,
                                  P(atr_denoise_variance_params), vp, vp, vp, vp], C.c_int),
        "atr_camera_rays_host": ([P(atr_camera), i64, i64, vp, vp], C.c_int),
        "atr_camera_rays": ([vp, P(atr_camera), i64, i64, vp, vp, vp], C.c_int),
        "atr_camera_guides": ([vp, P(atr_camera), vp, i32, P(atr_guides_out), vp], C.c_int),
        "atr_render_packed_size": ([vp, i32], i64),
        "atr_render_counters": ([vp, P(atr_camera), vp, i32, C.c_uint64, i32, i64 * 10], C.c_int),
        "atr_render_cull_counters": ([vp, P(atr_camera), vp, i32, C.c_uint64, i32, i64 * 5], C.c_int),
        "atr_render_fold_counters": ([vp, P(atr_camera), vp, i32, C.c_uint64, i32, i64 * 2], C.c_int),
        "atr_camera_pads_row": ([vp, C.c_float * 3, vp, vp, vp, i64], i64),
        "atr_render_leaf_box_counters": ([vp, P(atr_camera), vp, i32, C.c_uint64, i32, i64 * 2], C.c_int),
        "atr_camera_leaf_boxes_row": ([vp, C.c_float * 3, vp, vp, i64], i64),
        "atr_render_sky_cells": ([vp, P(atr_camera), vp, i32, C.c_uint64, i32, P(i64)], C.c_int),
        "atr_scene_sky_record": ([vp, i32 * 4, C.c_float * 28], C.c_int),
        "atr_sky_record_host": ([vp, i32, vp, i32, i32, i32, i32 * 4, C.c_float * 28], C.c_int),
        "atr_render_tile_costs": ([vp, P(atr_camera), vp, i32, C.c_uint64, vp], C.c_int),
        "atr_render_wave_trace": ([vp, P(atr_camera), vp, i32, C.c_uint64, i32, vp, i64, P(i64)], C.c_int),
        "atr_packed_pixel_map": ([vp, i32, i32, i32, vp, i64], i64),
        "atr_unpack": ([vp, vp, i32, i32, vp, vp, vp], C.c_int),
        "atr_tile_ray_casts": ([vp, vp, i32, i32, vp, vp, vp], C.c_int),
        "atr_packed_tile_ray_casts": ([vp, vp, i32, i32, i32, vp, i32, i64, vp, vp], C.c_int),
        "atr_set_cell_plan": ([vp, i32, i32, vp], C.c_int),
        "atr_render_phase_clocks": ([vp, P(atr_camera), vp, i32, C.c_uint64, i32, vp], C.c_int),
        "atr_default_tuning": ([P(atr_tuning)], None),
        "atr_set_tuning": ([vp, P(atr_tuning)], C.c_int),
        "atr_get_tuning": ([vp, P(atr_tuning)], C.c_int),
        "atr_pack_bgr": ([vp, vp, i64, vp, vp], C.c_int),
        "atr_render_plan_info": ([vp, vp, i32, i32, i32, vp, vp, i64, vp, P(i64)], C.c_int),
        "atr_scatter_bgr": ([vp, vp, i64, vp, vp, vp], C.c_int),
        "atr_pack_bgr_masked_bound": ([i64], i64),
        "atr_pack_bgr_masked": ([vp, vp, i64, u32, vp, vp, vp], C.c_int),
        "atr_scatter_bgr_masked": ([vp, vp, i64, vp, vp, vp], C.c_int),
        "atr_unpack_masked": ([vp, vp, i32, i32, i32, vp, i32, vp, i64, vp], C.c_int),
        "atr_unpack_masked_ranks": ([vp, i32, vp, vp, i32, i32, vp, vp, i32, vp, i64, vp], C.c_int),
        "atr_render_simd_counters": ([vp, P(atr_camera), vp, i32, C.c_uint64, i32, vp], C.c_int),
        "atr_render_path_counters": ([vp, P(atr_camera), vp, i32, C.c_uint64, i32, vp], C.c_int),
        "atr_render_cell_costs": ([vp, P(atr_camera), C.c_uint64, i32, vp], C.c_int),
        "atr_render_wait": ([vp, u32, P(i32)], C.c_int),
        "atr_render_start_progressive": ([vp, P(atr_camera), vp, i32, P(atr_frame), C.c_uint64, vp, i32, i32],
                                         C.c_int),
        "atr_write_bmp": ([vp, i32, i32, C.c_char_p, C.c_char_p, i32], C.c_int),
        "atr_render_start_frames": ([vp, P(atr_camera), vp, i32, P(atr_frame), i32, i64, C.c_uint64, vp, i32],
                                    C.c_int),
        "atr_render_start_cameras": ([vp, vp, i32, vp, i32, P(atr_frame), i64, C.c_uint64, vp, i32], C.c_int),
        "atr_last_kernel_ms": ([vp, P(C.c_float)], C.c_int),
        "atr_device_alloc": ([vp, C.c_size_t, P(vp)], C.c_int),
        "atr_device_free": ([vp, vp], C.c_int),
        "atr_memcpy_d2h": ([vp, vp, vp, C.c_size_t], C.c_int),
        "atr_memcpy_h2d": ([vp, vp, vp, C.c_size_t], C.c_int),
        "atr_memset_d": ([vp, vp, C.c_int, C.c_size_t], C.c_int),
    }
    for name in [n for n in DIAG_EXPORTS if not hasattr(L, n)]:
        del sig[name]  # product build: the diagnostic entry points are absent
    for name, (args, res) in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    global _sig
    _sig = sig
    _lib = L
    return L


_sig = None


def signatures():
    """{symbol: (argtypes, restype)} of the ctypes binding."""
    lib()
    return dict(_sig)


def vec3(t):
    return atr_vec3(float(t[0]), float(t[1]), float(t[2]))


def _sky_record(info, vals):
    v = np.array(list(vals), np.float32)
    return {"on": int(info[0]), "n": int(info[1]), "brute": int(info[2]) & 0xFFFFFFFF, "face": int(info[3]) & 0xFFFFFFFF,
            "t": v[0:1].copy(), "emission": v[1:4].copy(), "boxes": v[4:28].reshape(4, 6).copy()}


def sky_record(materials, models, nspheres=0, nplanes=0):
    """The sky path's record of a scene from upload()'s arguments, on the host (atr_sky_record_host):
    on, n, brute (bit per model), face, t (1,) f32, emission (3,) f32, boxes (4, 6) f32 = lo.xyz, hi.xyz."""
    mats = (atr_material * len(materials))(*[atr_material(vec3(e), vec3(r), float(s)) for e, r, s in materials])
    mods = (atr_model * max(1, len(models)))()
    for i, (mesh, tree, aabb, mat) in enumerate(models):
        mods[i].mesh = mesh.h.value
        mods[i].tree = tree.h.value if tree is not None else None
        for k in range(6):
            mods[i].surrounding_aabb[k] = float(aabb[k])
        mods[i].material = int(mat)
    info, vals = (C.c_int32 * 4)(), (C.c_float * 28)()
    check(lib().atr_sky_record_host(C.cast(mats, C.c_void_p), len(materials), C.cast(mods, C.c_void_p), len(models),
                                    int(nspheres), int(nplanes), info, vals), "sky record")
    return _sky_record(info, vals)


def tiles_array(tiles):
    """(n, 4) int array of inclusive rects -> ctypes atr_tile array."""
    t = np.ascontiguousarray(np.asarray(tiles, dtype=np.int32).reshape(-1, 4))
    arr = (atr_tile * max(1, len(t)))()
    C.memmove(arr, t.ctypes.data, t.nbytes)
    return arr, len(t)


def make_tiles(width, height, threads):
    """Reference tile grid (renderer.cpp:406-445)."""
    L = lib()
    n = L.atr_make_tiles(width, height, threads, None, 0)
    buf = (atr_tile * max(1, n))()
    L.atr_make_tiles(width, height, threads, C.cast(buf, C.c_void_p), n)
    return np.array([[t.min_x, t.min_y, t.max_x, t.max_y] for t in buf[:n]], np.int32).reshape(-1, 4)


def shard_grid(width, height, side):
    """The side x side shard grid, row-major, as an (n, 4) array of inclusive rects."""
    t = []
    for y in range(0, height, side):
        for x in range(0, width, side):
            t.append([x, y, min(x + side, width) - 1, min(y + side, height) - 1])
    return np.array(t, np.int32).reshape(-1, 4)


def balance_shard_tiles(width, height, side, world, costs, rank0_extra=0):
    """Owner rank per grid tile, longest-processing-time-first by measured cost."""
    costs = np.ascontiguousarray(costs, np.int64)
    owner = np.zeros(len(costs), np.int32)
    n = lib().atr_balance_shard_tiles(width, height, side, world, costs.ctypes.data, int(rank0_extra),
                                      owner.ctypes.data)
    if n != len(costs):
        raise AtrError(f"atr_balance_shard_tiles: {n} tiles for {len(costs)} costs")
    return owner


def make_shard_tiles(width, height, side, rank, world):
    L = lib()
    n = L.atr_make_shard_tiles(width, height, side, rank, world, None, 0)
    buf = (atr_tile * max(1, n))()
    L.atr_make_shard_tiles(width, height, side, rank, world, C.cast(buf, C.c_void_p), n)
    return np.array([[t.min_x, t.min_y, t.max_x, t.max_y] for t in buf[:n]], np.int32).reshape(-1, 4)


def write_bmp(pixels, name):
    """BGRX (H, W) u32 image, row 0 = bottom -> '<name>_<id>.bmp' (texture.cpp:66-115); returns the path."""
    px = np.ascontiguousarray(pixels, dtype=np.uint32)
    if px.ndim != 2:
        raise ValueError("write_bmp: pixels must be (height, width)")
    out = C.create_string_buffer(len(os.fsencode(name)) + 32)
    check(lib().atr_write_bmp(px.ctypes.data, px.shape[1], px.shape[0], os.fsencode(name), out, len(out)),
          f"write bmp {name}")
    return os.fsdecode(out.value)


class Mesh:
    """ModelData (model.h:15-23) held by the engine library."""

    def __init__(self, handle):
        self.h = C.c_void_p(handle)

    @classmethod
    def load_obj(cls, path, threads=None):
        """load_model_data; threads None = the library default (host threads, at most 16)."""
        h = C.c_void_p()
        if threads is None:
            check(lib().atr_mesh_load_obj(os.fsencode(path), C.byref(h)), f"load {path}")
        else:
            check(lib().atr_mesh_load_obj_threaded(os.fsencode(path), int(threads), C.byref(h)), f"load {path}")
        return cls(h.value)

    @classmethod
    def parse_obj(cls, text, threads=1):
        b = text.encode() if isinstance(text, str) else bytes(text)
        h = C.c_void_p()
        check(lib().atr_mesh_parse_obj_threaded(b, len(b), int(threads), C.byref(h)), "parse obj")
        return cls(h.value)

    def arrays(self):
        """ModelData copied out: vertices, normals, texcoords (n, 3) f32; face vertex, texcoord
        and normal indices (nfaces, 3) i32, 0-based (-1 = absent)."""
        nv, nn, nf = self.info()
        nt = C.c_uint32()
        check(lib().atr_mesh_export(self.h, None, None, None, C.byref(nt), None, None, None), "mesh export")
        V = np.zeros((max(nv, 1), 3), np.float32)
        N = np.zeros((max(nn, 1), 3), np.float32)
        T = np.zeros((max(nt.value, 1), 3), np.float32)
        FV, FT, FN = (np.zeros((max(nf, 1), 3), np.int32) for _ in range(3))
        check(lib().atr_mesh_export(self.h, V.ctypes.data, N.ctypes.data, T.ctypes.data, C.byref(nt),
                                    FV.ctypes.data, FT.ctypes.data, FN.ctypes.data), "mesh export")
        return V[:nv], N[:nn], T[:nt.value], FV[:nf], FT[:nf], FN[:nf]

    def info(self):
        nv, nn, nf = C.c_uint32(), C.c_uint32(), C.c_uint32()
        check(lib().atr_mesh_info(self.h, C.byref(nv), C.byref(nn), C.byref(nf)))
        return nv.value, nn.value, nf.value

    def aabb(self):
        box = (C.c_float * 6)()
        check(lib().atr_mesh_aabb(self.h, box))
        return np.array(list(box), np.float32)

    def translate_to(self, aabb, center):
        box = (C.c_float * 6)(*[float(x) for x in aabb])
        check(lib().atr_mesh_translate_to(self.h, box, vec3(center)))
        return np.array(list(box), np.float32)

    def __del__(self):
        if getattr(self, "h", None) is not None and self.h.value and _lib is not None:
            _lib.atr_mesh_free(self.h)
            self.h = None


class Octree:
    """KD_Tree (kd_tree.h:38-47): the reference's 8-ary octree, built on the host."""

    def __init__(self, handle):
        self.h = C.c_void_p(handle)

    @classmethod
    def build(cls, mesh: Mesh, max_faces=300):
        h = C.c_void_p()
        check(lib().atr_octree_build(mesh.h, int(max_faces), C.byref(h)), "octree build")
        return cls(h.value)

    @classmethod
    def build_device(cls, mesh: Mesh, max_faces=300, device=0, timings=None):
        """f3: the same build on the GPU (build.hip), bit-identical to build(). `timings`, if a
        dict, receives wall_ms (whole call) and device_ms (build kernels)."""
        h = C.c_void_p()
        ms = (C.c_float * 2)()
        check(lib().atr_octree_build_device(mesh.h, int(max_faces), int(device), C.byref(h), ms),
              "octree build (device)")
        if timings is not None:
            timings["wall_ms"], timings["device_ms"] = float(ms[0]), float(ms[1])
        return cls(h.value)

    @classmethod
    def from_nodes(cls, bounds, children, leaf_first, leaf_count, prim_vertices, prim_face):
        bounds = np.ascontiguousarray(bounds, np.float32)
        children = np.ascontiguousarray(children, np.int32)
        leaf_first = np.ascontiguousarray(leaf_first, np.uint32)
        leaf_count = np.ascontiguousarray(leaf_count, np.uint32)
        prim_vertices = np.ascontiguousarray(prim_vertices, np.float32)
        prim_face = np.ascontiguousarray(prim_face, np.uint32)
        h = C.c_void_p()
        check(lib().atr_octree_from_nodes(len(children), bounds.ctypes.data, children.ctypes.data,
                                          leaf_first.ctypes.data, leaf_count.ctypes.data,
                                          len(prim_face), prim_vertices.ctypes.data,
                                          prim_face.ctypes.data, C.byref(h)), "octree from nodes")
        return cls(h.value)

    def export(self):
        st = self.stats()
        n, p = st["nodes"], st["leaf_prim_refs"]
        bounds = np.zeros((n, 6), np.float32)
        children = np.zeros(n, np.int32)
        first = np.zeros(n, np.uint32)
        count = np.zeros(n, np.uint32)
        verts = np.zeros((max(p, 1), 9), np.float32)
        face = np.zeros(max(p, 1), np.uint32)
        check(lib().atr_octree_export(self.h, bounds.ctypes.data, children.ctypes.data,
                                      first.ctypes.data, count.ctypes.data, verts.ctypes.data,
                                      face.ctypes.data), "octree export")
        return bounds, children, first, count, verts[:p], face[:p]

    def stats(self):
        s = (C.c_int64 * 7)()
        check(lib().atr_octree_stats(self.h, s))
        keys = ["nodes", "inner", "leaves", "empty_leaves", "leaf_prim_refs", "max_leaf", "depth"]
        return dict(zip(keys, [int(x) for x in s]))

    def __del__(self):
        if getattr(self, "h", None) is not None and self.h.value and _lib is not None:
            _lib.atr_octree_free(self.h)
            self.h = None


def camera(width, height, spp=1, bounces=1, aa=False, eye=(0.1, 2.0, 0.0),
           facing=(-0.1, -0.5, -1.0), h_fov=1.0):
    """set_camera (camera.h:40-45); defaults are the app's (app.cpp:81-88)."""
    cm = atr_camera()
    check(lib().atr_camera_set(C.byref(cm), vec3(eye), vec3(facing), int(width), int(height),
                               int(bool(aa)), int(spp), int(bounces), float(h_fov)), "camera")
    return cm


def segment_rays(p, q, margin=1e-3):
    """The shadow rays of the segments p -> q for occluded_rays: (orig, dirs, t_max) with v = q - p,
    len = sqrt(len2(v)), dirs = v * (1 / len), t_max = len * (1 - margin). Pure torch (CPU or device
    tensors, (n, 3) float32); every step a separately rounded f32 operation in engine.h's order
    (len2 = (x*x + y*y) + z*z), so a non-degenerate segment passes the query's 2^-20 validity test.
    p == q gives a NaN direction, hence ATR_OCCL_INVALID. The margin keeps the surface at q itself
    out of the window."""
    import torch
    for name, a in (("p", p), ("q", q)):
        if not isinstance(a, torch.Tensor) or a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != 3:
            raise ValueError(f"{name}: an (n, 3) float32 tensor is required")
    if p.shape != q.shape:
        raise ValueError("p and q differ in length")
    v = q - p
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    # the correctly rounded f32 square root: through f64 (rounding its 53-bit root to 24 bits is
    # exact rounding); torch's vectorised f32 sqrt on the CPU is not correctly rounded
    length = torch.sqrt(((x * x + y * y) + z * z).double()).float()
    inv = torch.ones_like(length) / length
    keep = torch.ones_like(length) - torch.full_like(length, float(margin))
    return p, v * inv[:, None], length * keep


def gather_directions(normals, nsamples, first_sample=0, point_base=0, seed=0):
    """atr_gather_directions: the gather's sampler on the host, no device. normals: (n, 3) float32
    (numpy, or anything numpy converts). Returns (dirs (n, nsamples, 3) float32, traced (n, nsamples)
    uint8): the direction of every (point, sample) and whether gather_occlusion traces it (above the
    tangent plane and a valid direction); a normal that is not unit gives zeros."""
    nrm = np.ascontiguousarray(normals, np.float32)
    if nrm.ndim != 2 or nrm.shape[1] != 3:
        raise ValueError("normals: an (n, 3) float32 array is required")
    n, ns = len(nrm), int(nsamples)
    dirs = np.zeros((n, max(ns, 0), 3), np.float32)
    traced = np.zeros((n, max(ns, 0)), np.uint8)
    check(lib().atr_gather_directions(nrm.ctypes.data if n else None, n, ns, int(first_sample), int(point_base),
                                      C.c_uint64(int(seed) & (2**64 - 1)), dirs.ctypes.data if dirs.size else None,
                                      traced.ctypes.data if traced.size else None), "gather directions")
    return dirs, traced


def probe_directions(npoints, nsamples, first_sample=0, point_base=0, seed=0):
    """atr_probe_directions: the light probes' sphere sampler on the host, no device. Returns (dirs
    (npoints, nsamples, 3) float32, tries (npoints, nsamples) uint8): the direction of every (probe,
    sample), the bits probe_sh's dirs holds for a valid probe, and the try that was accepted (1..32, or
    33 where all 32 failed and the direction is +z)."""
    n, ns = int(npoints), int(nsamples)
    dirs = np.zeros((max(n, 0), max(ns, 0), 3), np.float32)
    tries = np.zeros((max(n, 0), max(ns, 0)), np.uint8)
    check(lib().atr_probe_directions(n, ns, int(first_sample), int(point_base), C.c_uint64(int(seed) & (2**64 - 1)),
                                     dirs.ctypes.data if dirs.size else None,
                                     tries.ctypes.data if tries.size else None), "probe directions")
    return dirs, tries


def sh_basis(dirs):
    """atr_sh_basis: the nine real spherical harmonics of bands 0..2 on unit directions, in the device's
    f32 operation order. dirs: (..., 3) float32 (numpy, or anything numpy converts). Returns (..., 9)
    float32."""
    d = np.ascontiguousarray(dirs, np.float32)
    if d.ndim < 1 or d.shape[-1] != 3:
        raise ValueError("dirs: an (..., 3) float32 array is required")
    out = np.zeros(d.shape[:-1] + (9,), np.float32)
    n = out.size // 9
    check(lib().atr_sh_basis(d.ctypes.data if n else None, n, out.ctypes.data if n else None), "sh basis")
    return out


def probe_grid(lo, hi, counts):
    """The probe points of a regular grid: counts = (nx, ny, nz) points per axis from lo to hi inclusive
    (an axis with one point sits at the middle of its range), x fastest, then y, then z. Returns
    (nx * ny * nz, 3) float32."""
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    counts = tuple(int(c) for c in counts)
    if len(counts) != 3 or min(counts) < 1:
        raise ValueError("counts: three positive integers are required")
    axes = [np.linspace(lo[a], hi[a], counts[a]) if counts[a] > 1 else np.array([(lo[a] + hi[a]) * 0.5])
            for a in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], axis=1).astype(np.float32)


# the cosine lobe's zonal factors for bands 0, 1, 2 (Ramamoorthi and Hanrahan 2001), per coefficient
_SH_COSINE = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5, np.float32)


def sh_irradiance(sh, normals):
    """The Lambertian irradiance that probe coefficients give a surface with unit normal n: the
    projected radiance convolved with the clamped cosine lobe, E(n) = sum_k A_k sh[k] Y_k(n) with A =
    pi, 2 pi / 3 and pi / 4 for bands 0, 1 and 2, in numpy float32. sh: (..., 9, 3) (probe_sh's sh
    viewed as coefficient x channel); normals: (m, 3). Returns (..., m, 3). This is the irradiance of
    the band-limited radiance -- a constant radiance L gives pi L for every normal -- and not
    gather_radiance's mean, which weights directions by the renderer's own bounce sampler and not by
    the cosine."""
    sh = np.asarray(sh, np.float32)
    if sh.ndim < 2 or sh.shape[-2:] != (9, 3):
        raise ValueError("sh: an (..., 9, 3) float32 array is required")
    y = sh_basis(normals)
    if y.ndim != 2:
        raise ValueError("normals: an (m, 3) float32 array is required")
    w = (y * _SH_COSINE[None, :]).astype(np.float32)  # (m, 9)
    return np.einsum("mk,...kc->...mc", w, sh).astype(np.float32)


def surface_points(orig, dirs, t, normal):
    """A trace_rays result as a gather's input, in bounce_shade's convention: (p, n) with p = o + d * t
    (a multiply, then an add, each rounded on its own) and n = the hit's normal, negated where
    dot(-d, n) < 0 (dot as engine.h: (x*x' + y*y') + z*z'). Pure torch: (n, 3) float32 tensors and an
    (n,) float32 t, on any one device. Rows of rays that missed are the caller's to drop."""
    import torch
    for name, a in (("orig", orig), ("dirs", dirs), ("normal", normal)):
        if not isinstance(a, torch.Tensor) or a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != 3:
            raise ValueError(f"{name}: an (n, 3) float32 tensor is required")
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1:
        raise ValueError("t: an (n,) float32 tensor is required")
    if not (orig.shape == dirs.shape == normal.shape and t.shape[0] == orig.shape[0]):
        raise ValueError("orig, dirs, t and normal differ in length")
    p = orig + dirs * t[:, None]
    m = -dirs
    att = (m[:, 0] * normal[:, 0] + m[:, 1] * normal[:, 1]) + m[:, 2] * normal[:, 2]
    n = torch.where((att < 0)[:, None], -normal, normal)
    return p, n


def camera_rays(cam):
    """The primary rays of an atr_camera without anti-aliasing, in pixel order (row y, then x), as
    atr_render_start_ex casts them: (orig, dirs), (width * height, 3) float32 numpy arrays. Host-side,
    every step a separately rounded f32 operation in the kernels' order (film_x, film_y, the point on
    the film, unit()), so radiance_rays on them with ray_base 0 equals the render bit for bit, and a
    slice of them with ray_base = its first pixel re-renders that region."""
    F = np.float32
    W, H = int(cam.width), int(cam.height)
    v = lambda a: np.array([a.x, a.y, a.z], F)  # noqa: E731
    eye, fc, cx, cy = v(cam.eye), v(cam.frame_center), v(cam.camera_x), v(cam.camera_y)
    fy = F(-1.0) + F(2.0) * (np.arange(H, dtype=F) / F(H))
    fx = ((F(-1.0) + F(2.0) * (np.arange(W, dtype=F) / F(W))) * F(cam.h_fov)) * F(cam.aspect_ratio)
    fx, fy = np.tile(fx, H), np.repeat(fy, W)
    p = (fc[None, :] + cx[None, :] * fx[:, None]) + cy[None, :] * fy[:, None]
    d = p - eye[None, :]
    len2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    # the correctly rounded f32 square root, through f64 (as segment_rays)
    inv = F(1.0) / np.sqrt(len2.astype(np.float64)).astype(F)
    dirs = np.ascontiguousarray(d * inv[:, None], F)
    return np.ascontiguousarray(np.broadcast_to(eye, dirs.shape), F), dirs


def camera_rays_host(cam, first_pixel=0, npixels=None):
    """atr_camera_rays_host: the primary rays of pixels first_pixel .. first_pixel + npixels - 1 of an
    atr_camera (npixels None: to the last pixel), from the library's own generator -- the function the
    device kernels call -- on the host, no device: (orig, dirs), (npixels, 3) float32 numpy arrays, the
    bits of camera_rays(cam)[first_pixel:first_pixel + npixels]."""
    first = int(first_pixel)
    n = int(cam.width) * int(cam.height) - first if npixels is None else int(npixels)
    orig, dirs = np.zeros((max(n, 0), 3), np.float32), np.zeros((max(n, 0), 3), np.float32)
    check(lib().atr_camera_rays_host(C.byref(cam), first, n, orig.ctypes.data if orig.size else None,
                                     dirs.ctypes.data if dirs.size else None), "camera rays host")
    return orig, dirs


class Engine:
    """One device context (atr_ctx): scene upload + renders on a HIP stream."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        check(lib().atr_create(int(device), C.byref(self.h)), "atr_create")
        self.device = device
        self._keep = []

    def upload(self, materials, models, spheres=(), planes=()):
        """materials: [(emission, reflection, scatter)], models: [(Mesh, Octree|None, aabb6, mat)]."""
        mats = (atr_material * len(materials))(
            *[atr_material(vec3(e), vec3(r), float(s)) for e, r, s in materials])
        mods = (atr_model * max(1, len(models)))()
        for i, (mesh, tree, aabb, mat) in enumerate(models):
            mods[i].mesh = mesh.h.value
            mods[i].tree = tree.h.value if tree is not None else None
            for k in range(6):
                mods[i].surrounding_aabb[k] = float(aabb[k])
            mods[i].material = int(mat)
        sph = (atr_sphere * max(1, len(spheres)))(
            *[atr_sphere(vec3(c), float(r), int(m)) for c, r, m in spheres])
        pln = (atr_plane * max(1, len(planes)))(
            *[atr_plane(vec3(n), float(d), int(m)) for n, d, m in planes])
        check(lib().atr_scene_upload(self.h, C.cast(mats, C.c_void_p), len(materials),
                                     C.cast(mods, C.c_void_p), len(models),
                                     C.cast(sph, C.c_void_p), len(spheres),
                                     C.cast(pln, C.c_void_p), len(planes)), "scene upload")
        self._keep = [materials, models]

    def workspace_info(self):
        """Path-engine workspaces held (count, device bytes): atr_workspace_info."""
        n, b = C.c_int32(), C.c_int64()
        check(lib().atr_workspace_info(self.h, C.byref(n), C.byref(b)))
        return {"workspaces": n.value, "device_bytes": b.value}

    def scene_info(self):
        b, n, d = C.c_int64(), C.c_int32(), C.c_int32()
        check(lib().atr_scene_info(self.h, C.byref(b), C.byref(n), C.byref(d)))
        return {"device_bytes": b.value, "max_nodes": n.value, "max_depth": d.value}

    def render_start(self, cam, tiles, frame: atr_frame, seed, stream=None, variant=ATR_KERNEL_AUTO):
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        check(lib().atr_render_start_ex(self.h, C.byref(cam), C.cast(arr, C.c_void_p), n,
                                        C.byref(frame), C.c_uint64(seed & (2**64 - 1)),
                                        C.c_void_p(stream) if stream else None, int(variant)),
              "render start")

    def render_start_samples(self, cam, tiles, frame: atr_frame, seed, first_sample, sum_ptr, stream=None,
                             variant=ATR_KERNEL_AUTO):
        """One sample pass of a frame: samples first_sample .. first_sample + cam.samples_per_pixel - 1,
        continuing the running sums at sum_ptr (device, 3 f32 per output slot, indexed as frame.rgb).
        Passes covering [0, N) in order on one stream leave the N-spp render, bit for bit."""
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        check(lib().atr_render_start_samples(self.h, C.byref(cam), C.cast(arr, C.c_void_p), n,
                                             C.byref(frame), C.c_uint64(seed & (2**64 - 1)),
                                             C.c_void_p(stream) if stream else None, int(variant),
                                             int(first_sample), C.c_void_p(sum_ptr) if sum_ptr else None),
              "sample pass start")

    def render_start_adaptive(self, cam, tiles, frame: atr_frame, seed, first_sample, sum_ptr, count_ptr, tolerance,
                              stream=None, variant=ATR_KERNEL_AUTO):
        """One adaptive sample pass: render_start_samples for the pixels still live only -- those whose
        u32 at count_ptr (device, one per output slot) equals first_sample with ATR_SAMPLES_CONVERGED
        clear; every pixel when first_sample is 0. A live pixel whose mean moved by less than
        tolerance x its brightness gets the flag and stops for good (atray.h has the rule)."""
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        check(lib().atr_render_start_adaptive(self.h, C.byref(cam), C.cast(arr, C.c_void_p), n,
                                              C.byref(frame), C.c_uint64(seed & (2**64 - 1)),
                                              C.c_void_p(stream) if stream else None, int(variant),
                                              int(first_sample), C.c_void_p(sum_ptr) if sum_ptr else None,
                                              C.c_void_p(count_ptr) if count_ptr else None, float(tolerance)),
              "adaptive pass start")

    def _xyz(self, **arrays):
        """The check of a query's (n, 3) inputs, by name: float32 tensors on the engine's device,
        contiguous and of one length. Returns (the device, n)."""
        import torch
        dev = torch.device("cuda", self.device)
        for name, a in arrays.items():
            if not isinstance(a, torch.Tensor) or a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != 3:
                raise ValueError(f"{name}: an (n, 3) float32 tensor is required")
            if a.device != dev:
                raise ValueError(f"{name}: not on {dev}")
            if not a.is_contiguous():
                raise ValueError(f"{name}: not contiguous")
        first, *rest = arrays
        for name in rest:
            if arrays[name].shape[0] != arrays[first].shape[0]:
                raise ValueError(f"{first} and {name} differ in length")
        return dev, int(arrays[first].shape[0])

    def _path_outputs(self, table, struct, noun, dev, n, ns, want, first_sample, given, required, keywords=False):
        """The outputs of a path query (radiance_rays, gather_radiance, probe_sh) of n `noun`: `want`
        checked against the call's output table (name -> (torch dtype name, trailing shape; "s" = ns), in
        the order of `struct`'s pointers), the earlier call's tensors in `given` checked and taken as
        they are -- those named in `required` must be there when first_sample > 0 -- and the rest
        allocated. `keywords`: the tensors came as keyword arguments, not in a `start` dict. Returns
        ({name: tensor}, the traced-ray tensor, the call's out-struct)."""
        import torch
        bad = [k for k in want if k not in table]
        if bad:
            raise ValueError(f"unknown outputs {bad}")
        if ns is not None and not 1 <= ns <= 65536:
            raise ValueError("nsamples: 1..65536")

        def shape(k):
            return (n,) + tuple(ns if d == "s" else d for d in table[k][1])

        bad = [k for k in given if k not in ("sum", "ray_casts") + tuple(required)]
        if bad:
            raise ValueError(f"start: unknown entries {bad}")
        for k, a in given.items():
            dt = table[k][0]
            if (not isinstance(a, torch.Tensor) or a.dtype != getattr(torch, dt) or a.device != dev
                    or not a.is_contiguous() or tuple(a.shape) != shape(k)):
                name = k if keywords else f"start[{k!r}]"
                raise ValueError(f"{name}: a contiguous {dt} tensor of {n} {noun} on {dev} is required")
        if int(first_sample) > 0 and any(k not in given for k in required):
            names = " and ".join(required)
            raise ValueError(f"{names}: required when first_sample > 0" if keywords else
                             f"start: {names} {'are' if len(required) > 1 else 'is'} required when first_sample > 0")
        out = {}
        for k in tuple(want) + tuple(k for k in given if k not in want):
            out[k] = given[k] if k in given else torch.empty(shape(k), dtype=getattr(torch, table[k][0]), device=dev)
        traced = torch.zeros(1, dtype=torch.int64, device=dev)
        return out, traced, struct(*[out[k].data_ptr() if k in out and n else None for k in table], traced.data_ptr())

    # atr_ray_hits outputs: name -> (torch dtype name, elements per ray, fill before the call)
    _RAY_OUTPUTS = {"t": ("float32", 1), "face": ("int32", 1), "model": ("int32", 1), "uv": ("float32", 2),
                    "kind": ("int32", 1), "material": ("int32", 1), "normal": ("float32", 3)}

    def trace_rays(self, orig, dirs, variant=ATR_KERNEL_AUTO, sort_bits=-1, stream=None,
                   outputs=("t", "face", "model", "uv", "kind", "material", "normal")):
        """atr_trace_rays: the closest hit of every ray of a batch. orig, dirs: contiguous (n, 3) float32
        tensors on the engine's device; directions normalised (a ray that is not, or not finite, comes
        back as ATR_RAY_INVALID with the miss record). Enqueued on `stream` (a raw HIP stream), or
        torch's current one. Returns ({name: tensor} for the requested outputs, in input order -- face
        as int32 bits, MISS = -1 -- and the traced-ray count as a one-element int64 tensor); valid
        once the stream has run, e.g. after wait()."""
        import torch
        dev, n = self._xyz(orig=orig, dirs=dirs)
        bad = [k for k in outputs if k not in self._RAY_OUTPUTS]
        if bad:
            raise ValueError(f"unknown outputs {bad}")
        out = {}
        for k in outputs:
            dt, per = self._RAY_OUTPUTS[k]
            out[k] = torch.empty((n, per) if per > 1 else (n,), dtype=getattr(torch, dt), device=dev)
        traced = torch.zeros(1, dtype=torch.int64, device=dev)
        hits = atr_ray_hits(*[out[k].data_ptr() if k in out and n else None
                              for k in ("t", "face", "model", "uv", "kind", "material", "normal")],
                            traced.data_ptr())
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib().atr_trace_rays(self.h, C.c_void_p(orig.data_ptr()) if n else None,
                                   C.c_void_p(dirs.data_ptr()) if n else None, n, C.byref(hits), int(variant),
                                   int(sort_bits), C.c_void_p(stream) if stream else None), "trace rays")
        return out, traced

    def occluded_rays(self, orig, dirs, t_max=None, variant=ATR_KERNEL_AUTO, sort_bits=-1, stream=None):
        """atr_occluded_rays: for every ray of a batch, is there any hit with 1e-4 < t < t_max. orig,
        dirs: as for trace_rays; t_max: a contiguous (n,) float32 tensor on the engine's device, or None
        (every ray unbounded). Returns (a uint8 tensor of ATR_OCCL_* in input order, the traced-ray count
        as a one-element int64 tensor); valid once the stream has run, e.g. after wait()."""
        import torch
        dev, n = self._xyz(orig=orig, dirs=dirs)
        if t_max is not None:
            if not isinstance(t_max, torch.Tensor) or t_max.dtype != torch.float32 or t_max.dim() != 1:
                raise ValueError("t_max: an (n,) float32 tensor is required")
            if t_max.device != dev:
                raise ValueError(f"t_max: not on {dev}")
            if not t_max.is_contiguous():
                raise ValueError("t_max: not contiguous")
            if t_max.shape[0] != n:
                raise ValueError("t_max and orig differ in length")
        occ = torch.empty(n, dtype=torch.uint8, device=dev)
        traced = torch.zeros(1, dtype=torch.int64, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib().atr_occluded_rays(self.h, C.c_void_p(orig.data_ptr()) if n else None,
                                      C.c_void_p(dirs.data_ptr()) if n else None,
                                      C.c_void_p(t_max.data_ptr()) if n and t_max is not None else None, n,
                                      C.c_void_p(occ.data_ptr()) if n else None, C.c_void_p(traced.data_ptr()),
                                      int(variant), int(sort_bits), C.c_void_p(stream) if stream else None),
              "occluded rays")
        return occ, traced

    def occluded_segments(self, p, q, margin=1e-3, variant=ATR_KERNEL_AUTO, sort_bits=-1, stream=None):
        """Is the segment from p towards q blocked before it reaches q: segment_rays, then occluded_rays
        (p == q comes back as ATR_OCCL_INVALID). p, q: (n, 3) float32 tensors on the engine's device."""
        orig, dirs, t_max = segment_rays(p, q, margin)
        return self.occluded_rays(orig.contiguous(), dirs.contiguous(), t_max.contiguous(), variant=variant,
                                  sort_bits=sort_bits, stream=stream)

    # atr_gather_out outputs: name -> elements per point or per (point, sample)
    _GATHER_OUTPUTS = ("visible", "occluded", "mask", "dirs")

    def gather_occlusion(self, points, normals, nsamples, t_max=None, first_sample=0, point_base=0, seed=0,
                         variant=ATR_KERNEL_AUTO, stream=None, outputs=("visible", "occluded")):
        """atr_gather_occlusion: nsamples hemisphere directions per surface point, drawn on the device and
        answered as occluded_rays answers them. points, normals: contiguous (n, 3) float32 tensors on the
        engine's device (unit normals); t_max: a contiguous (n,) float32 tensor there, or None (unbounded).
        Returns ({name: tensor} for the requested outputs -- visible, occluded: (n,) int32 counts; mask:
        (n, ceil(nsamples / 32)) int32 words, bit s % 32 of word s // 32 set iff sample s is visible;
        dirs: (n, nsamples, 3) float32 -- and the traced-sample count as a one-element int64 tensor);
        valid once the stream has run, e.g. after wait()."""
        import torch
        dev, n = self._xyz(points=points, normals=normals)
        ns = int(nsamples)
        if t_max is not None:
            if not isinstance(t_max, torch.Tensor) or t_max.dtype != torch.float32 or t_max.dim() != 1:
                raise ValueError("t_max: an (n,) float32 tensor is required")
            if t_max.device != dev:
                raise ValueError(f"t_max: not on {dev}")
            if not t_max.is_contiguous():
                raise ValueError("t_max: not contiguous")
            if t_max.shape[0] != n:
                raise ValueError("t_max and points differ in length")
        bad = [k for k in outputs if k not in self._GATHER_OUTPUTS]
        if bad:
            raise ValueError(f"unknown outputs {bad}")
        if not 1 <= ns <= 65536:
            raise ValueError("nsamples: 1..65536")
        shapes = {"visible": ((n,), torch.int32), "occluded": ((n,), torch.int32),
                  "mask": ((n, (ns + 31) // 32), torch.int32), "dirs": ((n, ns, 3), torch.float32)}
        out = {k: torch.empty(shapes[k][0], dtype=shapes[k][1], device=dev) for k in outputs}
        traced = torch.zeros(1, dtype=torch.int64, device=dev)
        go = atr_gather_out(*[out[k].data_ptr() if k in out and n else None for k in self._GATHER_OUTPUTS],
                            traced.data_ptr())
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib().atr_gather_occlusion(self.h, C.c_void_p(points.data_ptr()) if n else None,
                                         C.c_void_p(normals.data_ptr()) if n else None,
                                         C.c_void_p(t_max.data_ptr()) if n and t_max is not None else None, n, ns,
                                         int(first_sample), int(point_base), C.c_uint64(int(seed) & (2**64 - 1)),
                                         C.byref(go), int(variant), C.c_void_p(stream) if stream else None),
              "gather occlusion")
        return out, traced

    def ambient_occlusion(self, points, normals, nsamples, t_max=None, first_sample=0, point_base=0, seed=0,
                          variant=ATR_KERNEL_AUTO, stream=None):
        """The visible share of every point's traced samples, visible / max(visible + occluded, 1), as an
        (n,) float32 tensor (gather_occlusion's arguments; computed on torch's current stream, so pass
        that stream or None)."""
        import torch
        out, _ = self.gather_occlusion(points, normals, nsamples, t_max, first_sample, point_base, seed, variant,
                                       stream, outputs=("visible", "occluded"))
        vis, occ = out["visible"], out["occluded"]
        return vis.to(torch.float32) / torch.clamp(vis + occ, min=1).to(torch.float32)

    # atr_radiance_out outputs: name -> (torch dtype name, trailing shape)
    _RADIANCE_OUTPUTS = {"rgb": ("float32", (3,)), "sum": ("float32", (3,)), "ray_casts": ("int32", ()),
                         "invalid": ("uint8", ())}

    def radiance_rays(self, orig, dirs, nsamples, bounces, seed=0, first_sample=0, ray_base=0, sort_bits=-1,
                      stream=None, want=("rgb", "ray_casts", "invalid"), sum=None, ray_casts=None):
        """atr_radiance_rays: the path-traced colour along every ray of a batch, nsamples samples of at
        most `bounces` bounces each on the streams of (seed, ray_base + i, first_sample + s). orig, dirs:
        contiguous (n, 3) float32 tensors on the engine's device, directions normalised (a ray that is
        not, or not finite, comes back with invalid 1, untraced). `want` names the outputs (rgb, sum,
        ray_casts, invalid). A later sample range continues an earlier one through `sum` (an (n, 3)
        float32 tensor of an earlier call, required when first_sample > 0 and updated in place) and,
        optionally, `ray_casts` (an (n,) int32 tensor of an earlier call, likewise). Enqueued on `stream`
        (a raw HIP stream), or torch's current one. Returns ({name: tensor}, the traced-ray count as a
        one-element int64 tensor); valid once the stream has run, e.g. after wait()."""
        import torch
        dev, n = self._xyz(orig=orig, dirs=dirs)
        given = {k: a for k, a in (("sum", sum), ("ray_casts", ray_casts)) if a is not None}
        out, traced, ro = self._path_outputs(self._RADIANCE_OUTPUTS, atr_radiance_out, "rays", dev, n, None, want,
                                             first_sample, given, ("sum",), keywords=True)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib().atr_radiance_rays(self.h, C.c_void_p(orig.data_ptr()) if n else None,
                                      C.c_void_p(dirs.data_ptr()) if n else None, n, int(nsamples),
                                      int(first_sample), int(ray_base), int(bounces),
                                      C.c_uint64(int(seed) & (2**64 - 1)), C.byref(ro), int(sort_bits),
                                      C.c_void_p(stream) if stream else None), "radiance rays")
        return out, traced

    # atr_gather_radiance_out outputs: name -> (torch dtype name, trailing shape; "s" = nsamples)
    _GATHER_RADIANCE_OUTPUTS = {"rgb": ("float32", (3,)), "sum": ("float32", (3,)), "samples": ("int32", ()),
                                "ray_casts": ("int32", ()), "invalid": ("uint8", ()),
                                "sample_rgb": ("float32", ("s", 3)), "dirs": ("float32", ("s", 3))}

    def gather_radiance(self, points, normals, nsamples, bounces, seed=0, first_sample=0, point_base=0,
                        sort_bits=-1, start=None, stream=None, want=("rgb", "samples", "invalid")):
        """atr_gather_radiance: the light arriving at every surface point over its hemisphere, nsamples
        paths per point, each the renderer's own path after a diffuse hit there (the direction drawn on
        the device on the stream of (seed, point_base + i, first_sample + s), then at most `bounces`
        bounces on that stream). points, normals: contiguous (n, 3) float32 tensors on the engine's
        device (unit normals; a point that is not finite or whose normal is not unit comes back with
        invalid 1, untraced). `want` names the outputs: rgb, sum (n, 3) float32; samples, ray_casts (n,)
        int32; invalid (n,) uint8; sample_rgb, dirs (n, nsamples, 3) float32. A later sample range
        continues an earlier one through `start`, a dict with that call's `sum` and `samples` tensors
        (required when first_sample > 0) and optionally its `ray_casts`; they are updated in place and
        returned. Enqueued on `stream` (a raw HIP stream), or torch's current one. Returns ({name:
        tensor}, the traced-ray count as a one-element int64 tensor); valid once the stream has run,
        e.g. after wait()."""
        import torch
        dev, n = self._xyz(points=points, normals=normals)
        ns = int(nsamples)
        out, traced, go = self._path_outputs(self._GATHER_RADIANCE_OUTPUTS, atr_gather_radiance_out, "points", dev, n,
                                             ns, want, first_sample, dict(start or {}), ("sum", "samples"))
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib().atr_gather_radiance(self.h, C.c_void_p(points.data_ptr()) if n else None,
                                        C.c_void_p(normals.data_ptr()) if n else None, n, ns, int(first_sample),
                                        int(point_base), int(bounces), C.c_uint64(int(seed) & (2**64 - 1)),
                                        C.byref(go), int(sort_bits), C.c_void_p(stream) if stream else None),
              "gather radiance")
        return out, traced

    # atr_probe_sh_out outputs: name -> (torch dtype name, trailing shape; "s" = nsamples)
    _PROBE_SH_OUTPUTS = {"sh": ("float32", (9, 3)), "sum": ("float32", (9, 3)), "ray_casts": ("int32", ()),
                         "invalid": ("uint8", ()), "sample_rgb": ("float32", ("s", 3)),
                         "dirs": ("float32", ("s", 3))}

    def probe_sh(self, points, nsamples, bounces, seed=0, first_sample=0, point_base=0, start=None,
                 want=("sh", "invalid"), sort_bits=-1, stream=None):
        """atr_probe_sh: light probes -- the radiance arriving at every point over the whole sphere,
        nsamples paths per probe (the direction drawn uniformly on the device on the stream of (seed,
        point_base + i, first_sample + s), then at most `bounces` bounces on that stream), projected
        on the nine real spherical harmonics of bands 0..2. points: a contiguous (n, 3) float32 tensor
        on the engine's device (a point that is not finite comes back with invalid 1, untraced).
        `want` names the outputs: sh, sum (n, 9, 3) float32 (coefficient, channel); ray_casts (n,)
        int32; invalid (n,) uint8; sample_rgb, dirs (n, nsamples, 3) float32. A later sample range
        continues an earlier one through `start`, a dict with that call's `sum` tensor (required when
        first_sample > 0) and optionally its `ray_casts`; they are updated in place and returned.
        Enqueued on `stream` (a raw HIP stream), or torch's current one. Returns ({name: tensor}, the
        traced-ray count as a one-element int64 tensor); valid once the stream has run, e.g. after
        wait(). sh_irradiance(sh, normals) lights a normal from the result."""
        import torch
        dev, n = self._xyz(points=points)
        ns = int(nsamples)
        out, traced, go = self._path_outputs(self._PROBE_SH_OUTPUTS, atr_probe_sh_out, "probes", dev, n, ns, want,
                                             first_sample, dict(start or {}), ("sum",))
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib().atr_probe_sh(self.h, C.c_void_p(points.data_ptr()) if n else None, n, ns, int(first_sample),
                                 int(point_base), int(bounces), C.c_uint64(int(seed) & (2**64 - 1)), C.byref(go),
                                 int(sort_bits), C.c_void_p(stream) if stream else None), "probe sh")
        return out, traced

    # atr_texels_out outputs: name -> (torch dtype name, trailing shape); slot is per texel, the rest per covered k
    _TEXEL_OUTPUTS = {"slot": ("int32", ()), "texel": ("int32", ()), "face": ("int32", ()), "bary": ("float32", (2,)),
                      "point": ("float32", (3,)), "normal": ("float32", (3,))}

    def mesh_texels(self, mesh, width, height, flip=False, timings=None):
        """atr_mesh_texels: one surface sample per texel of `mesh`'s UV layout that a face covers, made on
        the device (two calls: a size query, then the fill). Returns a dict of tensors on the engine's
        device: slot (height * width,) int32, the texel's rank k among the covered ones or -1; and per
        covered k, in ascending texel order, texel (n,) int32 (j * width + i), face (n,) int32, bary
        (n, 2), point (n, 3) and normal (n, 3) float32 -- point and normal are what the gathers take.
        flip negates the normals. The mesh is the host Mesh: to bake an uploaded scene, pass the mesh
        that was uploaded, at the position it was uploaded with. Synchronous: complete on return.
        timings (a dict, optional) receives wall_ms and device_ms of the second call."""
        import torch
        dev = torch.device("cuda", self.device)
        w, h = int(width), int(height)
        flags = ATR_TEXELS_FLIP if flip else 0
        out = {"slot": torch.empty(max(w, 0) * max(h, 0), dtype=torch.int32, device=dev)}
        n = C.c_int64()
        torch.cuda.synchronize(dev)  # the call runs on a stream of the context's own
        check(lib().atr_mesh_texels(self.h, mesh.h, w, h, flags, 0, C.byref(atr_texels_out()), C.byref(n), None),
              "mesh texels (size)")
        for k, (dt, tail) in self._TEXEL_OUTPUTS.items():
            if k != "slot":
                out[k] = torch.empty((n.value,) + tail, dtype=getattr(torch, dt), device=dev)
        torch.cuda.synchronize(dev)
        to = atr_texels_out(*[out[k].data_ptr() if out[k].numel() else None for k in self._TEXEL_OUTPUTS])
        ms = (C.c_float * 2)()
        check(lib().atr_mesh_texels(self.h, mesh.h, w, h, flags, n.value, C.byref(to), C.byref(n), ms), "mesh texels")
        if timings is not None:
            timings["wall_ms"], timings["device_ms"] = float(ms[0]), float(ms[1])
        return out

    def texels_to_image(self, values, texel, width, height, passes=2, fill=(0, 0, 0), stream=None):
        """atr_texels_to_image: per-texel results into a finished lightmap. values: a contiguous (n, 3)
        float32 tensor, texel: the contiguous (n,) int32 tensor mesh_texels returned (ascending, unique),
        both on the engine's device. The covered texels get their values, then `passes` (0..64) dilation
        passes give every empty texel next to a filled one the mean of its filled neighbours, and the
        texels still empty get `fill`. Enqueued on `stream` (a raw HIP stream), or torch's current one.
        Returns the image as a (height, width, 3) float32 tensor (row 0 at v near 0); valid once the
        stream has run, e.g. after wait()."""
        import torch
        dev = torch.device("cuda", self.device)
        if (not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.dim() != 2
                or values.shape[1] != 3 or values.device != dev or not values.is_contiguous()):
            raise ValueError(f"values: a contiguous (n, 3) float32 tensor on {dev} is required")
        if (not isinstance(texel, torch.Tensor) or texel.dtype != torch.int32 or texel.dim() != 1
                or texel.device != dev or not texel.is_contiguous()):
            raise ValueError(f"texel: a contiguous (n,) int32 tensor on {dev} is required")
        if values.shape[0] != texel.shape[0]:
            raise ValueError("values and texel differ in length")
        n, w, h = int(texel.shape[0]), int(width), int(height)
        image = torch.empty((max(h, 0), max(w, 0), 3), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib().atr_texels_to_image(self.h, C.c_void_p(values.data_ptr()) if n else None,
                                        C.c_void_p(texel.data_ptr()) if n else None, n, w, h, int(passes),
                                        (C.c_float * 3)(*[float(x) for x in fill]),
                                        C.c_void_p(image.data_ptr()) if image.numel() else None,
                                        C.c_void_p(stream) if stream else None), "texels to image")
        return image

    def denoise(self, color, normal=None, position=None, ident=None, passes=5, sigma_color=0.01, sigma_position=0.0,
                normal_power_log2=5, out=None, framebuffer=False, stream=None):
        """atr_denoise: the edge-avoiding a-trous filter on an image (atray.h has the formulas). color: a
        contiguous (H, W, 3) float32 tensor on the engine's device; the guides normal, position: the
        same, or None; ident: a contiguous (H, W) int32 or uint32 tensor, or None (ATR_DENOISE_EMPTY, -1
        as int32, marks a pixel that is left alone and never read). out: an (H, W, 3) float32 tensor to
        write (it may be `color` itself), or None for a new one. Enqueued on `stream` (a raw HIP
        stream), or torch's current one. Returns the image, or with framebuffer=True (the image, the
        BGRX framebuffer as an (H, W) int32 tensor); valid once the stream has run, e.g. after wait()."""
        import torch
        dev = torch.device("cuda", self.device)
        if (not isinstance(color, torch.Tensor) or color.dtype != torch.float32 or color.dim() != 3
                or color.shape[2] != 3 or color.device != dev or not color.is_contiguous()):
            raise ValueError(f"color: a contiguous (H, W, 3) float32 tensor on {dev} is required")
        h, w = int(color.shape[0]), int(color.shape[1])
        for name, a in (("normal", normal), ("position", position), ("out", out)):
            if a is None:
                continue
            if (not isinstance(a, torch.Tensor) or a.dtype != torch.float32 or tuple(a.shape) != (h, w, 3)
                    or a.device != dev or not a.is_contiguous()):
                raise ValueError(f"{name}: a contiguous ({h}, {w}, 3) float32 tensor on {dev} is required")
        if ident is not None:
            kinds = (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ())
            if (not isinstance(ident, torch.Tensor) or ident.dtype not in kinds or tuple(ident.shape) != (h, w)
                    or ident.device != dev or not ident.is_contiguous()):
                raise ValueError(f"ident: a contiguous ({h}, {w}) int32 or uint32 tensor on {dev} is required")
        if out is None:
            out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        fb = torch.empty((h, w), dtype=torch.int32, device=dev) if framebuffer else None
        ptr = lambda a: C.c_void_p(a.data_ptr()) if a is not None and a.numel() else None  # noqa: E731
        guides = atr_denoise_guides(*[a.data_ptr() if a is not None and a.numel() else None
                                      for a in (normal, position, ident)])
        params = atr_denoise_params(int(passes), float(sigma_color), float(sigma_position), int(normal_power_log2))
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib().atr_denoise(self.h, ptr(color), C.byref(guides), w, h, C.byref(params), ptr(out), ptr(fb),
                                C.c_void_p(stream) if stream else None), "denoise")
        return (out, fb) if framebuffer else out

    def denoise_variance(self, color, variance, normal=None, position=None, ident=None, moments=None, length=None,
                         passes=3, sigma_luminance=8.0, luminance_floor=1e-4, sigma_position=0.0, normal_power_log2=5,
                         spatial_below=4, out=None, variance_out=False, framebuffer=False, stream=None):
        """atr_denoise_variance: the variance-guided a-trous filter (atray.h has the formulas). color,
        normal, position, ident and out as in denoise(); variance: a contiguous (H, W) float32 tensor, the
        variance of each pixel's luminance (accumulate()'s); moments (H, W, 2) float32 and length (H, W)
        int32 or uint32: a history's, both or neither, for the spatial estimate of pixels whose length
        is below spatial_below. variance_out: False, True for a new (H, W) float32 tensor, or a tensor
        to write (it may be `variance` itself). Enqueued on `stream` (a raw HIP stream), or torch's
        current one. Returns the image, or a tuple (image, variance_out, framebuffer) of the requested
        ones; valid once the stream has run, e.g. after wait()."""
        import torch
        dev = torch.device("cuda", self.device)
        if (not isinstance(color, torch.Tensor) or color.dtype != torch.float32 or color.dim() != 3
                or color.shape[2] != 3 or color.device != dev or not color.is_contiguous()):
            raise ValueError(f"color: a contiguous (H, W, 3) float32 tensor on {dev} is required")
        h, w = int(color.shape[0]), int(color.shape[1])
        kinds = (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ())

        def image(name, a, dtypes, shape):
            if (not isinstance(a, torch.Tensor) or a.dtype not in dtypes or tuple(a.shape) != shape
                    or a.device != dev or not a.is_contiguous()):
                what = " or ".join(str(d).replace("torch.", "") for d in dtypes)
                raise ValueError(f"{name}: a contiguous {shape} {what} tensor on {dev} is required")

        image("variance", variance, (torch.float32,), (h, w))
        for name, a in (("normal", normal), ("position", position), ("out", out)):
            if a is not None:
                image(name, a, (torch.float32,), (h, w, 3))
        if ident is not None:
            image("ident", ident, kinds, (h, w))
        if (moments is None) != (length is None):
            raise ValueError("moments and length: both or neither")
        if moments is not None:
            image("moments", moments, (torch.float32,), (h, w, 2))
            image("length", length, kinds, (h, w))
        if isinstance(variance_out, torch.Tensor):
            image("variance_out", variance_out, (torch.float32,), (h, w))
            vout = variance_out
        else:
            vout = torch.empty((h, w), dtype=torch.float32, device=dev) if variance_out else None
        if out is None:
            out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        fb = torch.empty((h, w), dtype=torch.int32, device=dev) if framebuffer else None
        ptr = lambda a: C.c_void_p(a.data_ptr()) if a is not None and a.numel() else None  # noqa: E731
        guides = atr_denoise_guides(*[a.data_ptr() if a is not None and a.numel() else None
                                      for a in (normal, position, ident)])
        params = atr_denoise_variance_params(int(passes), float(sigma_luminance), float(luminance_floor),
                                             float(sigma_position), int(normal_power_log2), int(spatial_below))
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib().atr_denoise_variance(self.h, ptr(color), ptr(variance), C.byref(guides), ptr(moments), ptr(length),
                                         w, h, C.byref(params), ptr(out), ptr(vout), ptr(fb),
                                         C.c_void_p(stream) if stream else None), "denoise_variance")
        extra = tuple(a for a, on in ((vout, vout is not None), (fb, framebuffer)) if on)
        return (out,) + extra if extra else out

    def render_guides(self, cam, stream=None):
        """The denoiser's guides for a frame of `cam`: trace_rays on camera_rays(cam), then (normal,
        position, ident) as (H, W, 3), (H, W, 3) float32 and (H, W) int32 tensors in the render's IMAGE
        orientation. normal and position are surface_points' (the normal turned towards the eye);
        ident is ATR_DENOISE_EMPTY (-1) where the ray met the sky or was invalid, else (kind << 28) |
        (model + 1). Computed on torch's current stream, so pass that stream or None."""
        import torch
        dev = torch.device("cuda", self.device)
        h, w = int(cam.height), int(cam.width)
        orig, dirs = (torch.from_numpy(a).to(dev) for a in camera_rays(cam))
        hit, _ = self.trace_rays(orig, dirs, stream=stream, outputs=("t", "model", "kind", "normal"))
        pos, nrm = surface_points(orig, dirs, hit["t"], hit["normal"])
        kind, model = hit["kind"], hit["model"]
        ident = torch.where((kind == ATR_RAY_SKY) | (kind == ATR_RAY_INVALID), torch.full_like(kind, -1),
                            (kind << 28) | (model + 1))
        return (nrm.reshape(h, w, 3).contiguous(), pos.reshape(h, w, 3).contiguous(),
                ident.to(torch.int32).reshape(h, w).contiguous())

    _GUIDE_OUTPUTS = {"normal": ("float32", 3), "position": ("float32", 3), "ident": ("int32", 1),
                      "depth": ("float32", 1), "material": ("int32", 1)}

    def camera_guides(self, cam, tiles=None, outputs=("normal", "position", "ident"), out=None, stream=None):
        """atr_camera_guides: the guides of a frame of `cam` in one device call, the bits render_guides
        returns (atray.h has the formulas). tiles: (n, 4) inclusive rects inside the image, or None for
        the full frame. outputs: any of "normal", "position" (H, W, 3) float32, "ident" (H, W) int32
        (ATR_DENOISE_EMPTY is -1), "depth" (H, W) float32 (the hit's t), "material" (H, W) int32. out:
        None for new tensors, or a dict of contiguous tensors of those shapes to write (ident and material
        int32 or uint32); pixels outside the tiles keep what they hold (in a new tensor: undefined).
        Enqueued on `stream` (a raw HIP stream), or torch's current one. Returns the tensors as a tuple in
        the order of `outputs`; valid once the stream has run, e.g. after wait()."""
        import torch
        dev = torch.device("cuda", self.device)
        h, w = int(cam.height), int(cam.width)
        outputs = tuple(outputs)
        bad = [k for k in outputs if k not in self._GUIDE_OUTPUTS]
        if bad or not outputs or len(set(outputs)) != len(outputs):
            raise ValueError(f"outputs: a non-empty choice of {tuple(self._GUIDE_OUTPUTS)} is required")
        given = dict(out) if out is not None else {}
        extra = [k for k in given if k not in outputs]
        if extra:
            raise ValueError(f"out: entries {extra} are not among the outputs")
        res = {}
        for k in outputs:
            dt, per = self._GUIDE_OUTPUTS[k]
            shape = (h, w, per) if per > 1 else (h, w)
            a = given.get(k)
            if a is None:
                a = torch.empty(shape, dtype=getattr(torch, dt), device=dev)
            else:
                kinds = (getattr(torch, dt),) + ((torch.uint32,) if dt == "int32" and hasattr(torch, "uint32") else ())
                if (not isinstance(a, torch.Tensor) or a.dtype not in kinds or tuple(a.shape) != shape
                        or a.device != dev or not a.is_contiguous()):
                    raise ValueError(f"out[{k!r}]: a contiguous {shape} {dt} tensor on {dev} is required")
            res[k] = a
        if tiles is None:
            tiles = [[0, 0, w - 1, h - 1]]
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        g = atr_guides_out(*[res[k].data_ptr() if k in res else None
                             for k in ("normal", "position", "ident", "depth", "material")])
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib().atr_camera_guides(self.h, C.byref(cam), C.cast(arr, C.c_void_p), n, C.byref(g),
                                      C.c_void_p(stream) if stream else None), "camera guides")
        return tuple(res[k] for k in outputs)

    def camera_rays(self, cam, first_pixel=0, npixels=None, stream=None):
        """atr_camera_rays: the primary rays of pixels first_pixel .. first_pixel + npixels - 1 of `cam`
        (npixels None: to the last pixel) made on the device: (orig, dirs), (npixels, 3) float32 tensors,
        the bits of camera_rays(cam) -- input for trace_rays and radiance_rays without a host build or a
        copy. Enqueued on `stream` (a raw HIP stream), or torch's current one."""
        import torch
        dev = torch.device("cuda", self.device)
        first = int(first_pixel)
        n = int(cam.width) * int(cam.height) - first if npixels is None else int(npixels)
        orig = torch.empty((max(n, 0), 3), dtype=torch.float32, device=dev)
        dirs = torch.empty((max(n, 0), 3), dtype=torch.float32, device=dev)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib().atr_camera_rays(self.h, C.byref(cam), first, n, C.c_void_p(orig.data_ptr()) if n > 0 else None,
                                    C.c_void_p(dirs.data_ptr()) if n > 0 else None,
                                    C.c_void_p(stream) if stream else None), "camera rays")
        return orig, dirs

    def accumulate(self, color, guides, prev=None, cam=None, alpha=0.0, alpha_moments=0.0, max_length=64,
                   plane_tolerance=0.02, min_normal_dot=0.9, moments=True, out=None, variance=False, framebuffer=False,
                   stream=None):
        """atr_accumulate: this frame blended into the history reprojected from the previous camera
        (atray.h has the formulas). color: a contiguous (H, W, 3) float32 tensor on the engine's device.
        guides: (normal, position, ident) as render_guides returns them, (H, W, 3), (H, W, 3) float32 and
        (H, W) int32 or uint32, any of them None (position is required once there is a history). prev:
        None to start a history, else the dict an earlier call returned: "cam" (the atr_camera of that
        frame), "guides" (its triple), "color", "moments" (or None), "length". cam: this frame's camera,
        only stored in the returned dict for the next call. moments: whether a history that starts
        carries moments (with prev, its own decides). out: None for new tensors, or a dict with "color"
        (it may be `color` itself), "moments" and "length" to write, none of them prev's. Enqueued on
        `stream` (a raw HIP stream), or torch's current one. Returns the new dict; with variance=True
        and/or framebuffer=True a tuple (dict, variance (H, W) float32, framebuffer (H, W) int32) of the
        requested ones; valid once the stream has run, e.g. after wait()."""
        import torch
        dev = torch.device("cuda", self.device)
        if (not isinstance(color, torch.Tensor) or color.dtype != torch.float32 or color.dim() != 3
                or color.shape[2] != 3 or color.device != dev or not color.is_contiguous()):
            raise ValueError(f"color: a contiguous (H, W, 3) float32 tensor on {dev} is required")
        h, w = int(color.shape[0]), int(color.shape[1])
        kinds = (torch.int32,) + ((torch.uint32,) if hasattr(torch, "uint32") else ())

        def image(name, a, dtypes, shape):
            if a is None:
                return
            if (not isinstance(a, torch.Tensor) or a.dtype not in dtypes or tuple(a.shape) != shape
                    or a.device != dev or not a.is_contiguous()):
                what = " or ".join(str(d).replace("torch.", "") for d in dtypes)
                raise ValueError(f"{name}: a contiguous {shape} {what} tensor on {dev} is required")

        def triple(name, g):
            if g is None:
                g = (None, None, None)
            if not isinstance(g, (tuple, list)) or len(g) != 3:
                raise ValueError(f"{name}: (normal, position, ident) is required")
            image(f"{name} normal", g[0], (torch.float32,), (h, w, 3))
            image(f"{name} position", g[1], (torch.float32,), (h, w, 3))
            image(f"{name} ident", g[2], kinds, (h, w))
            return tuple(g)

        guides = triple("guides", guides)
        if prev is not None:
            missing = [k for k in ("cam", "guides", "color", "length") if prev.get(k) is None]
            if missing:
                raise ValueError(f"prev: entries {missing} are required")
            pg = triple("prev guides", prev["guides"])
            image("prev color", prev["color"], (torch.float32,), (h, w, 3))
            image("prev moments", prev.get("moments"), (torch.float32,), (h, w, 2))
            image("prev length", prev["length"], kinds, (h, w))
            moments = prev.get("moments") is not None
        new = dict(out) if out is not None else {}
        image("out color", new.get("color"), (torch.float32,), (h, w, 3))
        image("out moments", new.get("moments"), (torch.float32,), (h, w, 2))
        image("out length", new.get("length"), kinds, (h, w))
        if new.get("color") is None:
            new["color"] = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        if new.get("length") is None:
            new["length"] = torch.empty((h, w), dtype=torch.int32, device=dev)
        if not moments:
            new["moments"] = None
        elif new.get("moments") is None:
            new["moments"] = torch.empty((h, w, 2), dtype=torch.float32, device=dev)
        if variance and not moments:
            raise ValueError("variance needs a history with moments")
        var = torch.empty((h, w), dtype=torch.float32, device=dev) if variance else None
        fb = torch.empty((h, w), dtype=torch.int32, device=dev) if framebuffer else None
        addr = lambda a: a.data_ptr() if a is not None and a.numel() else None  # noqa: E731
        ptr = lambda a: C.c_void_p(addr(a)) if addr(a) else None  # noqa: E731
        g = atr_denoise_guides(*[addr(a) for a in guides])
        ho = atr_history(addr(new["color"]), addr(new["moments"]), addr(new["length"]))
        params = atr_accumulate_params(float(alpha), float(alpha_moments), int(max_length), float(plane_tolerance),
                                       float(min_normal_dot))
        if prev is not None:
            pgs = atr_denoise_guides(*[addr(a) for a in pg])
            hp = atr_history(addr(prev["color"]), addr(prev.get("moments")), addr(prev["length"]))
            pargs = (C.byref(prev["cam"]), C.byref(pgs), C.byref(hp))
        else:
            pargs = (None, None, None)
        if stream is None:
            stream = torch.cuda.current_stream(dev).cuda_stream
        check(lib().atr_accumulate(self.h, ptr(color), C.byref(g), *pargs, w, h, C.byref(params), C.byref(ho),
                                   ptr(var), ptr(fb), C.c_void_p(stream) if stream else None), "accumulate")
        new["cam"] = atr_camera.from_buffer_copy(cam) if cam is not None else None
        new["guides"] = guides
        extra = tuple(a for a, on in ((var, variance), (fb, framebuffer)) if on)
        return (new,) + extra if extra else new

    def bake_lightmap(self, mesh, width, height, nsamples, bounces=None, t_max=None, seed=0, passes=2, flip=False,
                      denoise=None):
        """A lightmap of `mesh` in three device calls: mesh_texels, a hemisphere gather on the texels'
        points and normals, texels_to_image. bounces None: gather_occlusion (t_max: one bound for every
        texel, or None), the value visible / (visible + occluded) on all three channels and 0 where both
        are 0; an int: gather_radiance's rgb with that many bounces. `mesh` has to be the mesh of the
        uploaded scene, at the position it was uploaded with: the texels' points are taken from it, the
        rays are traced in the uploaded scene. denoise: None, or a dict of denoise()'s keywords (passes,
        sigma_color, sigma_position, normal_power_log2): the per-texel values, and the texels' normals
        and points, are put into images with texels_to_image(passes=0), ident is 0 where slot >= 0 and
        ATR_DENOISE_EMPTY elsewhere, the value image is denoised and read back at texel[], and those
        values go into the dilation in place of the gathered ones. Returns (the image as a (height,
        width, 3) float32 tensor, the texel dict of mesh_texels); on torch's current stream, complete on
        return."""
        import torch
        dev = torch.device("cuda", self.device)
        tex = self.mesh_texels(mesh, width, height, flip=flip)
        pts, nrm = tex["point"], tex["normal"]
        if bounces is None:
            tm = None if t_max is None else torch.full((pts.shape[0],), float(t_max), dtype=torch.float32, device=dev)
            out, _ = self.gather_occlusion(pts, nrm, nsamples, t_max=tm, seed=seed)
            vis, tot = out["visible"].to(torch.float32), (out["visible"] + out["occluded"]).to(torch.float32)
            val = torch.where(tot > 0, vis / torch.clamp(tot, min=1), torch.zeros_like(vis))
            values = val[:, None].expand(-1, 3).contiguous()
        else:
            out, _ = self.gather_radiance(pts, nrm, nsamples, int(bounces), seed=seed, want=("rgb",))
            values = out["rgb"]
        if denoise is not None:
            bad = [k for k in denoise if k not in ("passes", "sigma_color", "sigma_position", "normal_power_log2")]
            if bad:
                raise ValueError(f"denoise: unknown entries {bad}")
            col, nim, pim = (self.texels_to_image(v, tex["texel"], width, height, passes=0)
                             for v in (values, nrm, pts))
            h, w = int(col.shape[0]), int(col.shape[1])
            ident = torch.where(tex["slot"] >= 0, 0, -1).to(torch.int32).reshape(h, w).contiguous()
            den = self.denoise(col, normal=nim, position=pim, ident=ident, **denoise)
            values = den.reshape(-1, 3)[tex["texel"].to(torch.int64)].contiguous()
        image = self.texels_to_image(values, tex["texel"], width, height, passes=passes)
        rc, _ = self.wait()
        check(rc, "bake lightmap")
        torch.cuda.synchronize(dev)
        return image, tex

    def adaptive_info(self):
        """The last adaptive pass's counts, once wait() returned 0: (pixels live at its start, blocks
        with a live pixel, camera path groups traced, pixels still live after it)."""
        out = (C.c_int64 * 4)()
        check(lib().atr_render_adaptive_info(self.h, out), "adaptive info")
        return tuple(int(x) for x in out)

    def render_start_progressive(self, cam, tiles, frame: atr_frame, seed, tiles_per_launch, stream=None,
                                 variant=ATR_KERNEL_AUTO):
        """Live-view render: tiles_per_launch tiles per launch; wait() reports finished tiles."""
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        check(lib().atr_render_start_progressive(self.h, C.byref(cam), C.cast(arr, C.c_void_p), n,
                                                 C.byref(frame), C.c_uint64(seed & (2**64 - 1)),
                                                 C.c_void_p(stream) if stream else None, int(variant),
                                                 int(tiles_per_launch)), "progressive render start")

    def render_start_frames(self, cam, tiles, frame: atr_frame, nframes, frame_stride, seed, stream=None,
                            variant=ATR_KERNEL_AUTO):
        """nframes renders in one launch; frame f's outputs at f * frame_stride elements."""
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        check(lib().atr_render_start_frames(self.h, C.byref(cam), C.cast(arr, C.c_void_p), n, C.byref(frame),
                                            int(nframes), int(frame_stride), C.c_uint64(seed & (2**64 - 1)),
                                            C.c_void_p(stream) if stream else None, int(variant)),
              "render start frames")

    def render_start_cameras(self, cams, tiles, frame: atr_frame, frame_stride, seed, stream=None,
                             variant=ATR_KERNEL_AUTO):
        """len(cams) frames (at most 24) in one launch, frame f from cams[f]; outputs frame_stride apart."""
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        ca = (atr_camera * len(cams))(*cams)
        check(lib().atr_render_start_cameras(self.h, C.cast(ca, C.c_void_p), len(cams), C.cast(arr, C.c_void_p), n,
                                             C.byref(frame), int(frame_stride), C.c_uint64(seed & (2**64 - 1)),
                                             C.c_void_p(stream) if stream else None, int(variant)),
              "render start cameras")

    def counters(self, cam, tiles, seed, variant=ATR_KERNEL_AUTO):
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        out = (C.c_int64 * 10)()
        check(lib().atr_render_counters(self.h, C.byref(cam), C.cast(arr, C.c_void_p), n,
                                        C.c_uint64(seed & (2**64 - 1)), int(variant), out), "counters")
        keys = ["n_rays", "n_box", "n_tri", "n_leaf", "wave_tri_iters", "passes", "box_all", "waves",
                "cluster_boxes", "screened"]
        return dict(zip(keys, [int(x) for x in out]))

    def cull_counters(self, cam, tiles, seed, variant=ATR_KERNEL_AUTO):
        """The primary kernels' wave cull in one instrumented render (atr_render_cull_counters)."""
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        out = (C.c_int64 * 5)()
        check(lib().atr_render_cull_counters(self.h, C.byref(cam), C.cast(arr, C.c_void_p), n,
                                             C.c_uint64(seed & (2**64 - 1)), int(variant), out), "cull counters")
        return dict(zip(["culled", "lane_private_iters", "dealt_rounds", "dealt_items", "cluster_tests"], [int(x) for x in out]))

    def fold_counters(self, cam, tiles, seed, variant=ATR_KERNEL_AUTO):
        """What the facing fold removes from the primary kernels' work, counted by one instrumented render
        (atr_render_fold_counters): (ray, cluster) pairs past the loose box, primitives screened for them."""
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        out = (C.c_int64 * 2)()
        check(lib().atr_render_fold_counters(self.h, C.byref(cam), C.cast(arr, C.c_void_p), n,
                                             C.c_uint64(seed & (2**64 - 1)), int(variant), out), "fold counters")
        return {"loose_passes_removed": int(out[0]), "screened_removed": int(out[1])}

    def camera_pads_row(self, eye):
        """The row of the table of box growths that a one-camera launch at `eye` reads, built by the launch's
        own table kernel (atr_camera_pads_row), per scene cluster: row (n, 4) f32 = the entry's loose growth
        (folded) and tight growth, then the det floor and bits(mask of the primitives treated as
        rejected); boxes (n, 12) f32 = lo.xyz, P, hi.xyz, q, unfolded loose growth, 0, 0, 0;
        edges (n, 16, 6) f32 = ab, ac of the cluster's primitive slots (0 past its count)."""
        e = (C.c_float * 3)(*[float(x) for x in eye])
        n = int(lib().atr_camera_pads_row(self.h, e, None, None, None, 0))
        check(min(n, 0), "camera pads row")
        row, boxes = np.zeros((n, 4), np.float32), np.zeros((n, 12), np.float32)
        edges = np.zeros((n, 16, 6), np.float32)
        if n:
            check(min(int(lib().atr_camera_pads_row(self.h, e, row.ctypes.data, boxes.ctypes.data,
                                                    edges.ctypes.data, n)), 0), "camera pads row")
        return row, boxes, edges

    def leaf_box_counters(self, cam, tiles, seed, variant=ATR_KERNEL_AUTO):
        """The primary kernels' leaf boxes in one instrumented render (atr_render_leaf_box_counters):
        (ray, leaf) visits the product passes leave out, and the unsound ones among them (always 0)."""
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        out = (C.c_int64 * 2)()
        check(lib().atr_render_leaf_box_counters(self.h, C.byref(cam), C.cast(arr, C.c_void_p), n,
                                                 C.c_uint64(seed & (2**64 - 1)), int(variant), out), "leaf box counters")
        return {"skipped_visits": int(out[0]), "unsound_skips": int(out[1])}

    def sky_cells(self, cam, tiles, seed, variant=ATR_KERNEL_AUTO):
        """The wavefronts of one instrumented render none of whose rays passes any model's first box test
        (atr_render_sky_cells): the ones the product kernels finish without reading the scene."""
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        out = C.c_int64()
        check(lib().atr_render_sky_cells(self.h, C.byref(cam), C.cast(arr, C.c_void_p), n,
                                         C.c_uint64(seed & (2**64 - 1)), int(variant), C.byref(out)), "sky cells")
        return int(out.value)

    def sky_record(self):
        """What the sky path's kernels get of the uploaded scene (atr_scene_sky_record); see sky_record()."""
        info, vals = (C.c_int32 * 4)(), (C.c_float * 28)()
        check(lib().atr_scene_sky_record(self.h, info, vals), "sky record")
        return _sky_record(info, vals)

    def camera_leaf_boxes_row(self, eye):
        """The row of the table of leaf boxes that a one-camera launch at `eye` reads, built by the launch's
        own table kernels (atr_camera_leaf_boxes_row), per scene leaf: lo (n, 3) f32, hi (n, 3) f32,
        flag (n,) u32 (0 test, 1 no clusters, 2 never left out), ranges (n, 2) i32 = the leaf's first
        cluster in camera_pads_row's numbering and its cluster count."""
        e = (C.c_float * 3)(*[float(x) for x in eye])
        n = int(lib().atr_camera_leaf_boxes_row(self.h, e, None, None, 0))
        check(min(n, 0), "camera leaf boxes row")
        row, ranges = np.zeros((n, 8), np.float32), np.zeros((n, 2), np.int32)
        if n:
            check(min(int(lib().atr_camera_leaf_boxes_row(self.h, e, row.ctypes.data, ranges.ctypes.data, n)), 0),
                  "camera leaf boxes row")
        return row[:, 0:3].copy(), row[:, 4:7].copy(), row[:, 3].copy().view(np.uint32), ranges

    def tile_costs(self, cam, tiles, seed):
        """Shader clocks spent per tile by one render of `tiles` (load-balance calibration)."""
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        out = np.zeros(max(1, n), np.int64)
        check(lib().atr_render_tile_costs(self.h, C.byref(cam), C.cast(arr, C.c_void_p), n,
                                          C.c_uint64(seed & (2**64 - 1)), out.ctypes.data), "tile costs")
        return out[:n]

    def wave_trace(self, cam, tiles, seed, variant=0):
        """Diagnostic: (nblocks, 3) u64 per work block: start, end (100 MHz), HW_ID | XCC_ID << 32."""
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        nb = C.c_int64()
        args = (self.h, C.byref(cam), C.cast(arr, C.c_void_p), n, C.c_uint64(seed & (2**64 - 1)), int(variant))
        check(lib().atr_render_wave_trace(*args, None, 0, C.byref(nb)), "wave trace")
        out = np.zeros((max(1, nb.value), 3), np.uint64)
        check(lib().atr_render_wave_trace(*args, out.ctypes.data, out.size, C.byref(nb)), "wave trace")
        return out[:nb.value]

    def wait(self, timeout_ms=0xFFFFFFFF):
        done = C.c_int32()
        rc = check(lib().atr_render_wait(self.h, int(timeout_ms), C.byref(done)), "render wait")
        return rc, done.value

    def last_kernel_ms(self):
        ms = C.c_float()
        check(lib().atr_last_kernel_ms(self.h, C.byref(ms)))
        return ms.value

    def unpack(self, tiles, width, packed_ptr, image_ptr, stream=None):
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        check(lib().atr_unpack(self.h, C.cast(arr, C.c_void_p), n, int(width), C.c_void_p(packed_ptr),
                               C.c_void_p(image_ptr), C.c_void_p(stream) if stream else None), "unpack")

    def tile_ray_casts(self, tiles, width, casts_ptr, out_ptr, stream=None):
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        check(lib().atr_tile_ray_casts(self.h, C.cast(arr, C.c_void_p), n, int(width),
                                       C.c_void_p(casts_ptr), C.c_void_p(out_ptr),
                                       C.c_void_p(stream) if stream else None), "tile casts")

    def packed_tile_ray_casts(self, tiles, width, height, casts_ptr, nframes, frame_stride, out_ptr, stream=None):
        """out[f * ntiles + i] (device int64) = ray_casts of tile i in PACKED frame f (asynchronous)."""
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        check(lib().atr_packed_tile_ray_casts(self.h, C.cast(arr, C.c_void_p), n, int(width), int(height),
                                              C.c_void_p(casts_ptr), int(nframes), int(frame_stride),
                                              C.c_void_p(out_ptr), C.c_void_p(stream) if stream else None),
              "packed tile casts")

    def set_cell_plan(self, width, height, plan=None):
        """Per-8x8-cell split/priority bytes (atr_set_cell_plan); None clears."""
        if plan is None:
            check(lib().atr_set_cell_plan(self.h, int(width), int(height), None), "cell plan")
            return
        plan = np.ascontiguousarray(plan, np.uint8)
        assert plan.size == ((width + 7) // 8) * ((height + 7) // 8)
        check(lib().atr_set_cell_plan(self.h, int(width), int(height), plan.ctypes.data), "cell plan")

    def phase_clocks(self, cam, tiles, seed, variant=ATR_KERNEL_AUTO):
        """Wave clocks in DFS passes, lane-private scans, dealt rounds, whole waves (diagnostic)."""
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        out = (C.c_int64 * 6)()
        check(lib().atr_render_phase_clocks(self.h, C.byref(cam), C.cast(arr, C.c_void_p), n, C.c_uint64(seed),
                                            int(variant), out), "phase clocks")
        return dict(zip(["pass", "lane_private", "dealt", "wave", "step_prep", "scan"], list(out)))

    def pack_bgr(self, fb_ptr, npixels, out_ptr, stream=None):
        """BGRX u32 -> 3 bytes per pixel (atr_pack_bgr; device pointers, async on `stream`)."""
        check(lib().atr_pack_bgr(self.h, C.c_void_p(fb_ptr), int(npixels), C.c_void_p(out_ptr),
                                 C.c_void_p(stream) if stream else None), "pack bgr")

    def scatter_bgr(self, packed_ptr, npixels, index_ptr, image_ptr, stream=None):
        """3-byte pixels -> BGRX u32 at image[index[i]] (atr_scatter_bgr; device pointers, async)."""
        check(lib().atr_scatter_bgr(self.h, C.c_void_p(packed_ptr), int(npixels), C.c_void_p(index_ptr),
                                    C.c_void_p(image_ptr), C.c_void_p(stream) if stream else None), "scatter bgr")

    def pack_bgr_masked(self, fb_ptr, npixels, background, out_ptr, nbytes_ptr, stream=None):
        """BGRX u32 -> the masked stream (atr_pack_bgr_masked: a bit per pixel, 3 bytes per pixel that
        differs from `background`); its byte count goes to the device int64 at nbytes_ptr."""
        check(lib().atr_pack_bgr_masked(self.h, C.c_void_p(fb_ptr), int(npixels), int(background) & 0xFFFFFFFF,
                                        C.c_void_p(out_ptr), C.c_void_p(nbytes_ptr),
                                        C.c_void_p(stream) if stream else None), "pack bgr masked")

    def scatter_bgr_masked(self, packed_ptr, npixels, index_ptr, image_ptr, stream=None):
        """A masked stream of npixels -> BGRX u32 at image[index[i]] (atr_scatter_bgr_masked)."""
        check(lib().atr_scatter_bgr_masked(self.h, C.c_void_p(packed_ptr), int(npixels), C.c_void_p(index_ptr),
                                           C.c_void_p(image_ptr), C.c_void_p(stream) if stream else None),
              "scatter bgr masked")

    def unpack_masked(self, tiles, width, height, packed_ptr, nframes, image_ptr, image_stride, stream=None):
        """The masked stream of a PACKED render of `tiles` (nframes frames) into IMAGE frames
        image_stride pixels apart (atr_unpack_masked: positions from the tile list's blocks)."""
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        check(lib().atr_unpack_masked(self.h, C.cast(arr, C.c_void_p), n, int(width), int(height),
                                      C.c_void_p(packed_ptr), int(nframes), C.c_void_p(image_ptr), int(image_stride),
                                      C.c_void_p(stream) if stream else None), "unpack masked")

    def unpack_masked_ranks(self, tiles_list, width, height, packed_ptrs, nframes, image_ptr, image_stride,
                            stream=None, raw=None):
        """Several masked streams (source i: the PACKED render of tiles_list[i], its stream at
        packed_ptrs[i]; with raw[i] true, that render's u32 PACKED frames themselves) into the same
        IMAGE frames in one call (atr_unpack_masked_ranks)."""
        arrs = [t if isinstance(t, tuple) else tiles_array(t) for t in tiles_list]
        n = len(arrs)
        tp = (C.c_void_p * max(1, n))(*[C.cast(a, C.c_void_p) for a, _ in arrs])
        nt = (C.c_int32 * max(1, n))(*[k for _, k in arrs])
        pp = (C.c_void_p * max(1, n))(*[int(p) for p in packed_ptrs])
        rw = (C.c_int32 * max(1, n))(*[int(bool(x)) for x in raw]) if raw is not None else None
        check(lib().atr_unpack_masked_ranks(self.h, n, tp, nt, int(width), int(height), pp, rw, int(nframes),
                                            C.c_void_p(image_ptr), int(image_stride),
                                            C.c_void_p(stream) if stream else None), "unpack masked ranks")

    def plan_info(self, tiles, width, height):
        """The single-frame plan of a tile list (diagnostic): (base index per planned block, masks
        (n, 2) u32, cost per base block) or None before the first planned launch."""
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        npl = C.c_int64()
        args = (self.h, C.cast(arr, C.c_void_p), n, int(width), int(height))
        check(lib().atr_render_plan_info(*args, None, None, 0, None, C.byref(npl)), "plan info")
        if npl.value == 0:
            return None
        base = np.zeros(npl.value, np.int32)
        masks = np.zeros((npl.value, 2), np.uint32)
        cost = np.zeros(npl.value, np.uint64)  # the base list is shorter than the planned one
        check(lib().atr_render_plan_info(*args, base.ctypes.data, masks.ctypes.data, npl.value, cost.ctypes.data,
                                         C.byref(npl)), "plan info")
        return base, masks, cost

    def tuning(self):
        """The context's scheduling knobs (atr_get_tuning) as a dict."""
        t = atr_tuning()
        check(lib().atr_get_tuning(self.h, C.byref(t)), "get tuning")
        return {f: getattr(t, f) for f, _ in atr_tuning._fields_ if f != "reserved"}

    def set_tuning(self, **kw):
        """Change scheduling knobs (atr_set_tuning); unnamed fields keep their current value. Outputs
        never change; cluster_size applies at the next upload."""
        t = atr_tuning()
        check(lib().atr_get_tuning(self.h, C.byref(t)), "get tuning")
        for k, v in kw.items():
            if k not in {f for f, _ in atr_tuning._fields_} or k == "reserved":
                raise KeyError(k)
            setattr(t, k, int(v))
        check(lib().atr_set_tuning(self.h, C.byref(t)), "set tuning")

    def path_counters(self, cam, tiles, seed, variant=ATR_KERNEL_AUTO):
        """Bounce-loop lane use (diagnostic): wave steps and tracing lanes of bounce 0, 1, >= 2."""
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        out = (C.c_int64 * 6)()
        check(lib().atr_render_path_counters(self.h, C.byref(cam), C.cast(arr, C.c_void_p), n, C.c_uint64(seed),
                                             int(variant), out), "path counters")
        v = list(out)
        return {"steps": v[:3], "active": v[3:], "lane_use": [a / (64.0 * s) if s else 0.0 for s, a in zip(v[:3], v[3:])]}

    def simd_counters(self, cam, tiles, seed, variant=ATR_KERNEL_AUTO):
        """SIMD efficiency of the clustered scans (diagnostic, atr_render_simd_counters)."""
        arr, n = tiles if isinstance(tiles, tuple) else tiles_array(tiles)
        out = (C.c_int64 * 7)()
        check(lib().atr_render_simd_counters(self.h, C.byref(cam), C.cast(arr, C.c_void_p), n, C.c_uint64(seed),
                                             int(variant), out), "simd counters")
        keys = ["cand_wave_iters", "full_tests", "dfs_wave_iters", "dfs_lane_iters", "dealt_rounds", "dealt_items",
                "rays"]
        return dict(zip(keys, [int(x) for x in out]))

    def cell_costs(self, cam, seed, variant=ATR_KERNEL_AUTO):
        """Shader clocks per 8x8 cell of one full-frame render ((H+7)/8, (W+7)/8)."""
        out = np.zeros(((cam.height + 7) // 8) * ((cam.width + 7) // 8), np.int64)
        check(lib().atr_render_cell_costs(self.h, C.byref(cam), C.c_uint64(seed), int(variant), out.ctypes.data),
              "cell costs")
        return out.reshape((cam.height + 7) // 8, (cam.width + 7) // 8)

    def close(self):
        if getattr(self, "h", None) is not None and self.h.value:
            lib().atr_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TemporalAccumulator:
    """Frames of a static scene accumulated across cameras with Engine.accumulate: two history sets,
    ping-ponged, and the previous frame's camera and guides. A change of frame size starts the history
    again, as reset() does. Keywords are accumulate()'s parameters (alpha, alpha_moments, max_length,
    plane_tolerance, min_normal_dot)."""

    def __init__(self, engine, **params):
        bad = [k for k in params
               if k not in ("alpha", "alpha_moments", "max_length", "plane_tolerance", "min_normal_dot")]
        if bad:
            raise ValueError(f"unknown parameters {bad}")
        self.engine, self.params = engine, params
        self.sets, self.prev, self.index, self.variance = [None, None], None, 0, None

    def reset(self):
        """The next push starts a new history."""
        self.prev = self.variance = None

    def push(self, cam, color, guides=None, stream=None):
        """One frame: `color` (H, W, 3) float32 as rendered from `cam`, guides (normal, position, ident)
        or None for camera_guides(cam) (the bits of render_guides(cam), made in one device call). Returns
        (accumulated (H, W, 3), variance (H, W)); the accumulated tensor belongs to the history and is
        overwritten by the push after the next. On `stream` (a raw HIP stream), or torch's current one."""
        import torch
        if guides is None:
            guides = self.engine.camera_guides(cam, stream=stream)
        h, w = int(color.shape[0]), int(color.shape[1])
        if self.prev is not None and tuple(self.prev["color"].shape[:2]) != (h, w):
            self.prev = None
        k = self.index
        if self.sets[k] is None or tuple(self.sets[k]["color"].shape[:2]) != (h, w):
            dev = color.device
            self.sets[k] = {"color": torch.empty((h, w, 3), dtype=torch.float32, device=dev),
                            "moments": torch.empty((h, w, 2), dtype=torch.float32, device=dev),
                            "length": torch.empty((h, w), dtype=torch.int32, device=dev)}
        new, var = self.engine.accumulate(color, guides, prev=self.prev, cam=cam, out=self.sets[k], variance=True,
                                          stream=stream, **self.params)
        self.prev, self.index, self.variance = new, k ^ 1, var
        return new["color"], var

    def filtered(self, stream=None, **params):
        """The last push's accumulated frame through Engine.denoise_variance, with its variance, moments,
        length and guides; keywords are denoise_variance()'s parameters and framebuffer. Returns a new
        image (with framebuffer=True, (image, framebuffer)); the history is read, never written, so the
        next push sees what it would have seen."""
        bad = [k for k in params if k not in ("passes", "sigma_luminance", "luminance_floor", "sigma_position",
                                              "normal_power_log2", "spatial_below", "framebuffer")]
        if bad:
            raise ValueError(f"unknown parameters {bad}")
        if self.prev is None or self.variance is None:
            raise ValueError("filtered() needs a push first")
        normal, position, ident = self.prev["guides"]
        return self.engine.denoise_variance(self.prev["color"], self.variance, normal, position, ident,
                                            moments=self.prev["moments"], length=self.prev["length"], stream=stream,
                                            **params)


def pack_bgr_masked_bound(npixels):
    """Largest masked exchange stream of npixels pixels, in bytes (atr_pack_bgr_masked_bound)."""
    return int(lib().atr_pack_bgr_masked_bound(int(npixels)))


def packed_size(tiles):
    arr, n = tiles_array(tiles)
    return int(lib().atr_render_packed_size(C.cast(arr, C.c_void_p), n))


def packed_pixel_map(tiles, width, height):
    """Pixel index of every slot of a PACKED render of `tiles` (host-only)."""
    arr, n = tiles_array(tiles)
    L = lib()
    cnt = int(L.atr_packed_pixel_map(C.cast(arr, C.c_void_p), n, int(width), int(height), None, 0))
    out = np.zeros(max(cnt, 1), np.int64)
    L.atr_packed_pixel_map(C.cast(arr, C.c_void_p), n, int(width), int(height), out.ctypes.data, cnt)
    return out[:cnt]
