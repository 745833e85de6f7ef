"""Host-side mirror of the reference's render API over the HIP engine.

Names, argument meaning and return conventions follow Source/engine/renderer/renderer.h:
  prep_scene(scene) -> max_nodes                                   (renderer.h:35)
  start_render_from_camera(info, engine)                           (renderer.h:32)
  wait_for_render_from_camera_to_finish(info, engine, ms) -> bool  (renderer.h:33; True = running)
with Scene (scene.h:13-24), Model (model.h:66-71), Material (material.h), RenderSettings
(settings.h), Camera/set_camera (camera.h), RenderTile/RenderInfo (renderer.h:11-30),
load_model_data (OBJ_loader.h:6), get_AABB / translate_to (model.h:41-61,136-152).

The engine replaces the reference's ThreadPool: tiles are the reference grid for `threads`
(renderer.cpp:406-445), every pixel is traced once on the GPU, the framebuffer lands in the
caller's Texture (BGRX u32, row 0 = bottom) and per-tile ray_casts are the reference's sums
over the inclusive tile rects (overlaps counted twice, as the reference's threads do).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from . import engine as E

SKY_DEFAULT = ((0.3, 0.4, 0.5), (0.2, 0.3, 0.4), 0.3)     # app.cpp:91
MODEL_DEFAULT = ((0.4, 0.2, 0.2), (0.92, 0.5, 0.0), 0.3)  # app.cpp:96


@dataclass
class Material:
    emission_color: tuple = (0.0, 0.0, 0.0)
    reflection_color: tuple = (0.0, 0.0, 0.0)
    scatter: float = 0.0


@dataclass
class RenderSettings:
    resolution: tuple = (1280, 720)
    anti_aliasing: bool = False
    samples_per_pixel: int = 5
    bounce_limit: int = 5


@dataclass
class Camera:
    render_settings: RenderSettings
    c: E.atr_camera = None


def set_camera(eye, facing_towards, render_settings: RenderSettings, h_fov=1.0) -> Camera:
    rs = render_settings
    c = E.camera(rs.resolution[0], rs.resolution[1], rs.samples_per_pixel, rs.bounce_limit,
                 rs.anti_aliasing, eye=eye, facing=facing_towards, h_fov=h_fov)
    return Camera(rs, c)


class ModelData:
    def __init__(self, mesh: E.Mesh):
        self.mesh = mesh
        self.material = 0

    @property
    def sizes(self):
        return self.mesh.info()


def load_model_data(path: str) -> ModelData:
    return ModelData(E.Mesh.load_obj(path))


@dataclass
class Model:
    data: ModelData = None
    surrounding_aabb: np.ndarray = None
    kd_tree: Optional[E.Octree] = None
    max_no_faces_per_node: int = 300
    use_kd_tree: bool = True  # renderer.h:8 USE_KD_TREE


def get_AABB(data: ModelData) -> np.ndarray:
    return data.mesh.aabb()


def translate_to(model: Model, center) -> None:
    model.surrounding_aabb = model.data.mesh.translate_to(model.surrounding_aabb, center)


@dataclass
class Scene:
    materials: List[Material] = field(default_factory=list)
    models: List[Model] = field(default_factory=list)
    spheres: list = field(default_factory=list)   # (center, radius, material index)
    planes: list = field(default_factory=list)    # (normal, distance, material index)


def prep_scene(scene: Scene, engine: Optional[E.Engine] = None) -> int:
    """Build every model's octree (kd_tree.cpp:20-64) and upload the flattened scene.
    Plane normals are normalized first (renderer.cpp:267-270). Returns the max node count."""
    max_nodes = 0
    planes = []
    for n, d, m in scene.planes:
        v = np.array(n, np.float32)
        inv = np.float32(1.0) / np.sqrt(np.float32((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]))
        planes.append((tuple((v * inv).tolist()), d, m))
    for mdl in scene.models:
        if mdl.use_kd_tree and mdl.kd_tree is None:
            mdl.kd_tree = E.Octree.build(mdl.data.mesh, mdl.max_no_faces_per_node)
        if mdl.kd_tree is not None:
            max_nodes = max(max_nodes, mdl.kd_tree.stats()["nodes"])
    if engine is not None:
        mats = [(m.emission_color, m.reflection_color, m.scatter) for m in scene.materials]
        models = [(m.data.mesh, m.kd_tree if m.use_kd_tree else None, m.surrounding_aabb,
                   m.data.material) for m in scene.models]
        engine.upload(mats, models, scene.spheres, planes)
    return max_nodes


@dataclass
class RenderTile:
    tile: tuple
    ray_casts: int = 0


@dataclass
class RenderInfo:
    camera: Camera
    scene: Scene
    camera_tex: np.ndarray = None   # H x W uint32 BGRX, row 0 = bottom (texture.h:27-38)
    threads: int = 8                # tile grid of renderer.cpp:406 (the reference's pool size)
    seed: int = 0x853C49E6748FEA9B
    jobs: List[RenderTile] = field(default_factory=list)
    jobs_done: int = 0
    samples_done: int = 0           # sample-progressive renders: samples per pixel finished so far
    total_ray_casts: int = 0
    sample_counts: np.ndarray = None  # adaptive renders: H x W uint32 samples per pixel, refreshed with camera_tex
    pixels_live: int = 0              # adaptive renders: pixels the last pass left live (0: every pixel stopped)
    _dev: dict = field(default_factory=dict)


def sample_schedule(spp: int) -> List[int]:
    """The default refinement schedule of a sample-progressive render: passes of 1, 1, 2, 4, ...
    samples (the samples done double with every pass), the last pass trimmed so they sum to spp:
    64 -> [1, 1, 2, 4, 8, 16, 32], 100 -> [1, 1, 2, 4, 8, 16, 32, 36]."""
    spp = int(spp)
    if spp < 1:
        raise ValueError("sample_schedule: spp must be at least 1")
    passes, done = [], 0
    while done < spp:
        n = min(max(done, 1), spp - done)
        passes.append(n)
        done += n
    return passes


def start_render_from_camera(info: RenderInfo, engine: E.Engine, tiles_per_launch: int = 0,
                             sample_passes=None, adaptive_tolerance=None) -> None:
    """renderer.cpp:447-455. tiles_per_launch > 0 renders progressively by tile for a live view
    (app.cpp:162-186): wait_for_render_from_camera_to_finish then reports finished tiles in
    jobs_done and refreshes camera_tex with them while the render runs.

    sample_passes renders progressively by sample instead: a list of pass sizes summing to the
    camera's samples_per_pixel, or True for sample_schedule(spp). Every pass renders the whole
    image (atr_render_start_samples), so a noisy full frame exists after the first pass and
    wait_for_render_from_camera_to_finish reports the samples finished in samples_done. The final
    outputs are those of the one-shot render, bit for bit. The two progressive modes do not
    combine (ValueError).

    adaptive_tolerance (with sample_passes) enqueues the schedule through atr_render_start_adaptive:
    a pixel whose mean moved by less than tolerance x its brightness in a pass takes no further
    samples. sample_counts then tells how many each pixel got (every pixel's outputs are the one-shot
    render's at its own count) and pixels_live how many were still refining at the end. Tolerance 0
    stops nothing and equals the plain schedule. Without sample_passes it is a ValueError."""
    import torch
    W, H = info.camera.render_settings.resolution
    spp = int(info.camera.render_settings.samples_per_pixel)
    if sample_passes is not None and sample_passes is not False:
        if tiles_per_launch > 0:
            raise ValueError("start_render_from_camera: tiles_per_launch and sample_passes do not combine")
        passes = sample_schedule(spp) if sample_passes is True else [int(n) for n in sample_passes]
        if not passes or min(passes) < 1 or sum(passes) != spp:
            raise ValueError(f"start_render_from_camera: sample_passes must be positive and sum to {spp}")
    else:
        passes = None
    if adaptive_tolerance is not None:
        if passes is None:
            raise ValueError("start_render_from_camera: adaptive_tolerance needs sample_passes")
        adaptive_tolerance = float(adaptive_tolerance)
        if not (0.0 <= adaptive_tolerance < float("inf")):
            raise ValueError("start_render_from_camera: adaptive_tolerance must be finite and not negative")
    tiles = E.make_tiles(W, H, info.threads)
    info.jobs = [RenderTile(tuple(int(v) for v in t)) for t in tiles]
    info.jobs_done = 0
    dev = torch.device("cuda", engine.device)
    fb = torch.zeros(H * W, dtype=torch.int32, device=dev)
    casts = torch.zeros(H * W, dtype=torch.int32, device=dev)
    per_tile = torch.zeros(len(tiles), dtype=torch.int64, device=dev)
    frame = E.atr_frame(E.ATR_LAYOUT_IMAGE, fb.data_ptr(), None, None, None, casts.data_ptr(), None)
    d = {"fb": fb, "casts": casts, "per_tile": per_tile, "tiles": tiles}
    info.samples_done = 0
    info.sample_counts, info.pixels_live = None, 0
    if passes is not None:
        # own stream, as below; one event per pass tells the live view how far the frame is
        rs = torch.cuda.Stream(dev)
        rs.wait_stream(torch.cuda.current_stream(dev))
        d["render_stream"], d["copy_stream"] = rs, torch.cuda.Stream(dev)
        d["host"] = torch.empty(H * W, dtype=torch.int32, pin_memory=True)
        d["stream"] = rs.cuda_stream
        d["sum"] = torch.empty(3 * H * W, dtype=torch.float32, device=dev)  # written by the first pass
        d["pass_events"], d["pass_totals"] = [], []
        if adaptive_tolerance is not None:
            d["count"] = torch.empty(H * W, dtype=torch.int32, device=dev)  # written by the first pass
            d["host_count"] = torch.empty(H * W, dtype=torch.int32, pin_memory=True)
        cam = E.atr_camera.from_buffer_copy(info.camera.c)
        first = 0
        for n in passes:
            cam.samples_per_pixel = n
            if adaptive_tolerance is not None:
                engine.render_start_adaptive(cam, tiles, frame, info.seed, first, d["sum"].data_ptr(),
                                             d["count"].data_ptr(), adaptive_tolerance, stream=rs.cuda_stream)
            else:
                engine.render_start_samples(cam, tiles, frame, info.seed, first, d["sum"].data_ptr(),
                                            stream=rs.cuda_stream)
            ev = torch.cuda.Event()
            ev.record(rs)
            first += n
            d["pass_events"].append(ev)
            d["pass_totals"].append(first)
    elif tiles_per_launch > 0:
        # own stream, so the live copies (another stream) run beside the render
        rs = torch.cuda.Stream(dev)
        rs.wait_stream(torch.cuda.current_stream(dev))
        d["render_stream"], d["copy_stream"] = rs, torch.cuda.Stream(dev)
        d["host"] = torch.empty(H * W, dtype=torch.int32, pin_memory=True)
        d["stream"] = rs.cuda_stream
        engine.render_start_progressive(info.camera.c, tiles, frame, info.seed, tiles_per_launch, stream=rs.cuda_stream)
    else:
        d["stream"] = torch.cuda.current_stream(dev).cuda_stream
        engine.render_start(info.camera.c, tiles, frame, info.seed, stream=d["stream"])
    info._dev = d


def _strip_flag(counts) -> np.ndarray:
    return counts.view(np.uint32) & np.uint32(E.ATR_SAMPLES_CONVERGED - 1)


def _live_copy(info: RenderInfo) -> None:
    import torch
    d = info._dev
    W, H = info.camera.render_settings.resolution
    with torch.cuda.stream(d["copy_stream"]):
        d["host"].copy_(d["fb"], non_blocking=True)
        if "count" in d:
            d["host_count"].copy_(d["count"], non_blocking=True)
    d["copy_stream"].synchronize()
    info.camera_tex = d["host"].numpy().view(np.uint32).reshape(H, W).copy()
    if "count" in d:
        info.sample_counts = _strip_flag(d["host_count"].numpy()).reshape(H, W)


def wait_for_render_from_camera_to_finish(info: RenderInfo, engine: E.Engine, ms_to_wait_for: int) -> bool:
    """TRUE while still rendering after the timeout, FALSE once done (renderer.cpp:457-471)."""
    rc, done = engine.wait(ms_to_wait_for)
    d = info._dev
    if rc == 1:
        if "pass_events" in d:
            # the passes whose events have completed. The copy below runs beside the next pass, so
            # it may mix the states after two adjacent passes; each pixel is still a valid mean of
            # its own sample count (every pass rewrites a pixel with one 4-byte store).
            total = 0
            for ev, t in zip(d["pass_events"], d["pass_totals"]):
                if not ev.query():
                    break
                total = t
            if total > info.samples_done:
                info.samples_done = total
                _live_copy(info)
            return True
        if "copy_stream" in d and done > info.jobs_done:
            info.jobs_done = done
            _live_copy(info)  # the pixels of the first `done` tiles are final
        return True
    W, H = info.camera.render_settings.resolution
    engine.tile_ray_casts(d["tiles"], W, d["casts"].data_ptr(), d["per_tile"].data_ptr(), d["stream"])
    if "render_stream" in d:
        import torch
        torch.cuda.current_stream(d["fb"].device).wait_stream(d["render_stream"])
    per_tile = d["per_tile"].cpu().numpy()
    for j, c in zip(info.jobs, per_tile.tolist()):
        j.ray_casts = int(c)
    info.total_ray_casts += int(per_tile.sum())
    info.jobs_done = len(info.jobs)
    if "pass_totals" in d:
        info.samples_done = d["pass_totals"][-1]
    info.camera_tex = d["fb"].cpu().numpy().view(np.uint32).reshape(H, W)
    if "count" in d:
        info.sample_counts = _strip_flag(d["count"].cpu().numpy()).reshape(H, W)
        info.pixels_live = engine.adaptive_info()[3]
    return False


def write_to_file(info: RenderInfo, file_name: str) -> str:
    """The app's 'save render' (texture.cpp:66-115 via app.cpp): camera_tex as <file_name>_<id>.bmp."""
    if info.camera_tex is None:
        raise ValueError("write_to_file: nothing rendered yet")
    return E.write_bmp(info.camera_tex, file_name)


def app_scene(obj_path: str, center=(0.0, -15.0, -38.0), use_tree=True, leaf=300) -> Scene:
    """The app's scene (app.cpp:65-146): one model, sky = materials[0], model = materials[5]."""
    mats = [Material(*SKY_DEFAULT), Material((0, 0, 0), (0.2, 0.8, 0.2), 0.3),
            Material((0, 0, 0), (0.4, 0.8, 0.9), 0.9), Material((0, 0.4, 0.6), (0.2, 0.3, 0.2), 0.0),
            Material((0, 0, 0), (0.5, 0.5, 0.5), 0.0), Material(*MODEL_DEFAULT),
            Material((0.8, 0.2, 0.2), (0.92, 0.0, 0.0), 0.3)]
    data = load_model_data(obj_path)
    m = Model(data=data, surrounding_aabb=get_AABB(data), max_no_faces_per_node=leaf,
              use_kd_tree=use_tree)
    translate_to(m, center)
    data.material = 5
    return Scene(materials=mats, models=[m])
