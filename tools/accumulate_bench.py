"""What atr_accumulate costs: the Dragon frame (1 spp, 3 bounces) at 1920 x 1080 and 3840
x 2160 from two cameras, rendered and given their guides (render_guides) on the device; the first starts
a history with moments, the second is accumulated into it with all three guides and the default
parameters, with variance and framebuffer. The second camera is the first again ("rest") or one step of
0.02 rad on the orbit about the model's centre ("step"). Per size and move: atr_last_kernel_ms of the
call, and in the same run, under HIP events, a device-to-device copy that moves the call's compulsory
bytes (92 B read and 32 B written per pixel: a copy of 62 B per pixel). The calls are interleaved, their
order rotating by round, after warm-up rounds; medians with min and max. The kernel's own time comes from
running this script under a kernel trace (the script after `--`, no counters in that run); the kernel is
accumulate_kernel<normal, ident, moments>. Prints one JSON line and, with --out, writes it there.

--live makes every pixel live (the sky's guides zeroed, ident 0 everywhere): the Dragon covers 14 % of its
frame, and an inert pixel reads 40 B and writes 32 B. A sky pixel made live finds no history (its point
lies in front of no camera), so it reads and writes the same 72 B; only the Dragon's pixels gather.
--wall replaces the guides by those of a wall z = -40 that fills the frame (positions are the camera's rays
times an analytic t, one normal, ident 0): every pixel gathers its four taps, the full 124 B and more.

python tools/accumulate_bench.py [--rounds N] [--warmup N] [--sizes 1920x1080,3840x2160] [--live | --wall] [--out FILE]"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import atray_amd.engine as E  # noqa: E402
from atray_amd.assets import CENTERS, asset_path  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--sizes", default="1920x1080,3840x2160")
ap.add_argument("--asset", default="Dragon")
ap.add_argument("--live", action="store_true",
                help="every pixel live: ident 0 everywhere, the sky's normals and positions set to 0")
ap.add_argument("--wall", action="store_true",
                help="synthetic guides of a wall z = -40 that fills the frame: every pixel finds its history")
ap.add_argument("--out", default="")
args = ap.parse_args()

SEED = 0x853C49E6748FEA9B
SKY, MODEL = ((0.3, 0.4, 0.5), (0.2, 0.3, 0.4), 0.3), ((0.4, 0.2, 0.2), (0.92, 0.5, 0.0), 0.3)
APP_EYE, APP_FACING, STEP = (0.1, 2.0, 0.0), (-0.1, -0.5, -1.0), 0.02
# per pixel: this frame's colour, normal, position 12 B each and ident 4 B; the previous normal, position,
# colour 12 B each, ident 4 B, moments 8 B, length 4 B; out colour 12 B, moments 8 B, length, variance and
# framebuffer 4 B each
READ_B, WRITE_B = 92, 32
if not torch.cuda.is_available():
    sys.exit("accumulate_bench: no GPU")
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


class Frame:
    """One camera's 1-spp frame and its guides."""

    def __init__(self, w, h, k, seed):
        eye, facing = orbit(k)
        self.cam = E.camera(w, h, 1, 3, eye=eye, facing=facing)
        fb = torch.zeros(w * h, dtype=torch.int32, device=dev)
        self.color = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
        fr = E.atr_frame(E.ATR_LAYOUT_IMAGE, fb.data_ptr(), None, None, self.color.data_ptr(), None, None)
        eng.render_start(self.cam, [[0, 0, w - 1, h - 1]], fr, seed, stream=s.cuda_stream)
        assert eng.wait()[0] == 0
        normal, position, ident = eng.render_guides(self.cam)
        assert eng.wait()[0] == 0
        torch.cuda.synchronize()
        if args.live:  # the cost of a frame without sky
            sky = (ident == -1)[..., None]
            normal = torch.where(sky, torch.zeros_like(normal), normal)
            position = torch.where(sky, torch.zeros_like(position), position)
            ident = torch.zeros_like(ident)
            assert bool(torch.isfinite(normal).all() and torch.isfinite(position).all())
        if args.wall:
            orig, dirs = (torch.from_numpy(a).to(dev) for a in E.camera_rays(self.cam))
            t = (-40.0 - orig[:, 2]) / dirs[:, 2]
            assert bool((t > 0).all())
            position = (orig + dirs * t[:, None]).reshape(h, w, 3).contiguous()
            normal = torch.zeros_like(position)
            normal[..., 2] = 1.0
            ident = torch.zeros_like(ident)
        self.guides = (normal, position, ident)


class Case:
    def __init__(self, w, h):
        self.w, self.h, n = w, h, w * h
        self.first = Frame(w, h, 0, SEED)
        self.second = {"rest": Frame(w, h, 0, SEED + 1), "step": Frame(w, h, 1, SEED + 1)}
        self.prev = eng.accumulate(self.first.color, self.first.guides, None, cam=self.first.cam)
        assert eng.wait()[0] == 0
        torch.cuda.synchronize()
        self.live = int((self.prev["length"] != 0).sum().item())
        self.out = {"color": torch.empty((h, w, 3), dtype=torch.float32, device=dev),
                    "moments": torch.empty((h, w, 2), dtype=torch.float32, device=dev),
                    "length": torch.empty((h, w), dtype=torch.int32, device=dev)}
        self.src = torch.empty(n * (READ_B + WRITE_B) // 2, dtype=torch.uint8, device=dev)
        self.dst = torch.empty_like(self.src)
        self.ms = {"rest_kernel": [], "rest_events": [], "step_kernel": [], "step_events": [], "copy": []}
        self.found = {}

    def accumulate(self, move, keep):
        fr = self.second[move]
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record(s)
        new, _, _ = eng.accumulate(fr.color, fr.guides, self.prev, cam=fr.cam, out=self.out, variance=True,
                                   framebuffer=True, stream=s.cuda_stream)
        e[1].record(s)
        assert eng.wait()[0] == 0
        torch.cuda.synchronize()
        if keep:
            self.ms[move + "_kernel"].append(eng.last_kernel_ms())
            self.ms[move + "_events"].append(e[0].elapsed_time(e[1]))
            self.found[move] = int((new["length"] == 2).sum().item())

    def rest(self, keep):
        self.accumulate("rest", keep)

    def step(self, keep):
        self.accumulate("step", keep)

    def copy(self, keep):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record(s)
        self.dst.copy_(self.src)
        e[1].record(s)
        torch.cuda.synchronize()
        if keep:
            self.ms["copy"].append(e[0].elapsed_time(e[1]))


cases = [Case(*[int(v) for v in size.split("x")]) for size in args.sizes.split(",")]
steps = [(c, f) for c in cases for f in (Case.rest, Case.copy, Case.step)]
for r in range(args.warmup + args.rounds):
    k = r % len(steps)
    for c, f in steps[k:] + steps[:k]:
        f(c, r >= args.warmup)
res = {"config": f"{args.asset} 1 spp x 3 bounces; normal, position, ident{' (every pixel live)' if args.live else ''}"
                 f"{' (guides of a wall that fills the frame)' if args.wall else ''}; "
                 "moments; default parameters; variance and framebuffer",
       "rounds": args.rounds, "warmup": args.warmup}
for c in cases:
    row = {"pixels": c.w * c.h, "live_pixels": c.live, "pixels_with_history": c.found,
           "compulsory_bytes": c.w * c.h * (READ_B + WRITE_B)}
    for k, v in c.ms.items():
        row[k + "_ms"] = {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4),
                          "max": round(float(np.max(v)), 4)}
    for move in ("rest", "step"):
        row[move + "_over_copy"] = round(row[move + "_kernel_ms"]["median"] / row["copy_ms"]["median"], 2)
    res[f"{c.w}x{c.h}"] = row
line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
eng.close()
