"""What atr_camera_guides costs against what it replaces: the bench's c3 scene (the Dragon
from the app's camera) at 1920 x 1080 and 3840 x 2160.

Device time, per size, interleaved in one process, the order rotating by round, after warm-up rounds:
  guides        atr_last_kernel_ms of atr_camera_guides (normal, position, ident);
  composition   HIP events around Engine.render_guides' device part with the rays already on the device:
                atr_trace_rays (t, model, kind, normal; sort_bits 0), surface_points, the ident -- twice a
                round (composition, composition_again), so the file shows the spread between two runs of
                the same thing;
  trace         atr_last_kernel_ms of that atr_trace_rays alone;
  render        atr_last_kernel_ms of one c3 frame (1 spp, 1 bounce) of the same camera.
Wall time (host build and copies included, each call followed by a device synchronisation):
  camera_guides, render_guides     one frame;
  orbit_camera_guides, orbit_render_guides   --orbit frames of the 0.02-rad orbit through
                TemporalAccumulator.push, with the guides it obtains itself and with render_guides' handed in.
Medians with min and max. Prints one JSON line and, with --out, writes it there.

python tools/guides_bench.py [--rounds N] [--warmup N] [--wall-rounds N] [--orbit N] [--sizes 1920x1080,3840x2160] [--out FILE]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import atray_amd.engine as E  # noqa: E402
from atray_amd.assets import CENTERS, asset_path  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--wall-rounds", type=int, default=3)
ap.add_argument("--orbit", type=int, default=16)
ap.add_argument("--sizes", default="1920x1080,3840x2160")
ap.add_argument("--asset", default="Dragon")
ap.add_argument("--out", default="")
args = ap.parse_args()

SEED = 0x853C49E6748FEA9B
SKY, MODEL = ((0.3, 0.4, 0.5), (0.2, 0.3, 0.4), 0.3), ((0.4, 0.2, 0.2), (0.92, 0.5, 0.0), 0.3)
APP_EYE, APP_FACING, STEP = (0.1, 2.0, 0.0), (-0.1, -0.5, -1.0), 0.02
if not torch.cuda.is_available():
    sys.exit("guides_bench: no GPU")
dev = torch.device("cuda", 0)
s = torch.cuda.current_stream(dev)

eng = E.Engine(0)
mesh = E.Mesh.load_obj(asset_path(args.asset))
box = mesh.translate_to(mesh.aabb(), CENTERS[args.asset])
eng.upload([SKY, MODEL], [(mesh, E.Octree.build(mesh, 300), box, 1)])


def orbit(k):
    """The app's camera turned by k * STEP rad about the vertical axis through the model's centre."""
    c, a = np.array(CENTERS[args.asset], np.float64), k * STEP
    rot = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    eye = c + rot @ (np.array(APP_EYE, np.float64) - c)
    return tuple(float(x) for x in eye), tuple(float(x) for x in rot @ np.array(APP_FACING, np.float64))


def done():
    assert eng.wait()[0] == 0
    torch.cuda.synchronize()


class Case:
    def __init__(self, w, h):
        self.w, self.h = w, h
        self.cam = E.camera(w, h)
        self.tiles = E.tiles_array([[0, 0, w - 1, h - 1]])
        self.orig, self.dirs = eng.camera_rays(self.cam)
        self.out = {"normal": torch.empty((h, w, 3), dtype=torch.float32, device=dev),
                    "position": torch.empty((h, w, 3), dtype=torch.float32, device=dev),
                    "ident": torch.empty((h, w), dtype=torch.int32, device=dev)}
        self.fb = torch.zeros(w * h, dtype=torch.int32, device=dev)
        self.frame = E.atr_frame(E.ATR_LAYOUT_IMAGE, self.fb.data_ptr(), None, None, None, None, None)
        self.color = torch.rand((h, w, 3), dtype=torch.float32, device=dev)
        done()
        got, want = eng.camera_guides(self.cam, tiles=self.tiles, out=self.out), eng.render_guides(self.cam)
        done()
        assert all(torch.equal(a, b) for a, b in zip(got, want)), "the two disagree"
        self.hits = int((got[2] != -1).sum().item())
        self.ms = {k: [] for k in ("guides", "composition", "composition_again", "trace", "render")}
        self.wall = {k: [] for k in ("camera_guides", "render_guides", "orbit_camera_guides", "orbit_render_guides")}

    def guides(self, keep):
        eng.camera_guides(self.cam, tiles=self.tiles, out=self.out, stream=s.cuda_stream)
        done()
        if keep:
            self.ms["guides"].append(eng.last_kernel_ms())

    def compose(self):
        hit, _ = eng.trace_rays(self.orig, self.dirs, sort_bits=0, stream=s.cuda_stream,
                                outputs=("t", "model", "kind", "normal"))
        pos, nrm = E.surface_points(self.orig, self.dirs, hit["t"], hit["normal"])
        kind, model = hit["kind"], hit["model"]
        ident = torch.where((kind == E.ATR_RAY_SKY) | (kind == E.ATR_RAY_INVALID), torch.full_like(kind, -1),
                            (kind << 28) | (model + 1))
        return (nrm.reshape(self.h, self.w, 3).contiguous(), pos.reshape(self.h, self.w, 3).contiguous(),
                ident.to(torch.int32).reshape(self.h, self.w).contiguous())

    def composition(self, keep, name="composition"):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record(s)
        self.compose()
        e[1].record(s)
        done()
        if keep:
            self.ms[name].append(e[0].elapsed_time(e[1]))

    def composition_again(self, keep):
        self.composition(keep, "composition_again")

    def trace(self, keep):
        eng.trace_rays(self.orig, self.dirs, sort_bits=0, stream=s.cuda_stream, outputs=("t", "model", "kind", "normal"))
        done()
        if keep:
            self.ms["trace"].append(eng.last_kernel_ms())

    def render(self, keep):
        eng.render_start(self.cam, self.tiles, self.frame, SEED, stream=s.cuda_stream)
        done()
        if keep:
            self.ms["render"].append(eng.last_kernel_ms())

    def walls(self):
        for name, fn in (("camera_guides", eng.camera_guides), ("render_guides", eng.render_guides)):
            t0 = time.perf_counter()
            fn(self.cam)
            done()
            self.wall[name].append((time.perf_counter() - t0) * 1e3)
        cams = [E.camera(self.w, self.h, eye=eye, facing=facing) for eye, facing in map(orbit, range(args.orbit))]
        for name in ("orbit_camera_guides", "orbit_render_guides"):
            acc = E.TemporalAccumulator(eng)
            t0 = time.perf_counter()
            for cam in cams:
                acc.push(cam, self.color, None if name == "orbit_camera_guides" else eng.render_guides(cam))
            done()
            self.wall[name].append((time.perf_counter() - t0) * 1e3)


cases = [Case(*[int(v) for v in size.split("x")]) for size in args.sizes.split(",")]
steps = [(c, f) for c in cases for f in (Case.guides, Case.composition, Case.trace, Case.composition_again, Case.render)]
for r in range(args.warmup + args.rounds):
    k = r % len(steps)
    for c, f in steps[k:] + steps[:k]:
        f(c, r >= args.warmup)
for c in cases:
    for r in range(args.wall_rounds):
        c.walls()
res = {"config": f"{args.asset} from the app's camera; atr_camera_guides writes normal, position, ident; the "
                 "composition is atr_trace_rays (t, model, kind, normal; sort_bits 0) and render_guides' torch "
                 f"kernels on rays already on the device; wall times include a device synchronisation; orbit: "
                 f"{args.orbit} frames through TemporalAccumulator.push",
       "rounds": args.rounds, "warmup": args.warmup, "wall_rounds": args.wall_rounds}
for c in cases:
    row = {"pixels": c.w * c.h, "hit_pixels": c.hits}
    for k, v in list(c.ms.items()) + list(c.wall.items()):
        row[k + ("_wall_ms" if k in c.wall else "_ms")] = {
            "median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}
    m = lambda k: row[k]["median"]  # noqa: E731
    row["composition_spread_ms"] = round(abs(m("composition_ms") - m("composition_again_ms")), 4)
    row["guides_over_composition"] = round(m("guides_ms") / m("composition_ms"), 3)
    row["guides_over_trace"] = round(m("guides_ms") / m("trace_ms"), 3)
    row["guides_over_render"] = round(m("guides_ms") / m("render_ms"), 3)
    row["render_guides_over_camera_guides_wall"] = round(m("render_guides_wall_ms") / m("camera_guides_wall_ms"), 1)
    row["orbit_wall_ratio"] = round(m("orbit_render_guides_wall_ms") / m("orbit_camera_guides_wall_ms"), 1)
    res[f"{c.w}x{c.h}"] = row
line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
eng.close()
