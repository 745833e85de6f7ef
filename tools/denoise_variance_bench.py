"""What atr_denoise_variance costs: the Dragon frame (1 spp, 3 bounces) at 1920 x 1080 and
3840 x 2160 from two cameras one 0.02-rad step apart, rendered and given their guides (render_guides) on
the device and accumulated (atr_accumulate), so that colour, variance, moments and length are a real
history's: lengths 1 and 2 side by side. Per size, interleaved in one process, their order rotating by
round, after warm-up rounds: atr_last_kernel_ms of atr_denoise_variance with all guides and the default
parameters, out, variance_out and framebuffer written, with the spatial estimate (moments and length
given) and without it; atr_last_kernel_ms of atr_denoise at the same pass count with the same guides,
out and framebuffer written; and, under HIP events, a device-to-device copy that moves the call's
compulsory bytes (56 B read and 20 B written per pixel with the estimate: a copy of 38 B per pixel).
Medians with min and max. Prints one JSON line and, with --out, writes it there.

--live makes every pixel live (the sky's guides zeroed, ident 0 everywhere): the Dragon covers 14 % of its
frame, and an inert pixel costs a pass one record read and one written.

python tools/denoise_variance_bench.py [--rounds N] [--warmup N] [--sizes 1920x1080,3840x2160] [--live] [--out FILE]"""
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
ap.add_argument("--out", default="")
args = ap.parse_args()

SEED = 0x853C49E6748FEA9B
SKY, MODEL = ((0.3, 0.4, 0.5), (0.2, 0.3, 0.4), 0.3), ((0.4, 0.2, 0.2), (0.92, 0.5, 0.0), 0.3)
APP_EYE, APP_FACING, STEP = (0.1, 2.0, 0.0), (-0.1, -0.5, -1.0), 0.02
# per pixel: colour, normal, position 12 B each, variance and ident 4 B, moments 8 B, length 4 B; out 12 B,
# variance_out and framebuffer 4 B each
READ_B, WRITE_B = 56, 20
if not torch.cuda.is_available():
    sys.exit("denoise_variance_bench: no GPU")
dev = torch.device("cuda", 0)
s = torch.cuda.current_stream(dev)

eng = E.Engine(0)
mesh = E.Mesh.load_obj(asset_path(args.asset))
box = mesh.translate_to(mesh.aabb(), CENTERS[args.asset])
eng.upload([SKY, MODEL], [(mesh, E.Octree.build(mesh, 300), box, 1)])
defaults = E.atr_denoise_variance_params()
E.lib().atr_default_denoise_variance_params(defaults)


def orbit(k):
    """The app's camera turned by k * STEP rad about the vertical axis through the model's centre."""
    c, a = np.array(CENTERS[args.asset], np.float64), k * STEP
    rot = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    eye = c + rot @ (np.array(APP_EYE, np.float64) - c)
    return tuple(float(x) for x in eye), tuple(float(x) for x in rot @ np.array(APP_FACING, np.float64))


def frame(w, h, k, seed):
    """One camera's 1-spp frame and its guides: (cam, colour, (normal, position, ident))."""
    eye, facing = orbit(k)
    cam = E.camera(w, h, 1, 3, eye=eye, facing=facing)
    fb = torch.zeros(w * h, dtype=torch.int32, device=dev)
    color = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
    fr = E.atr_frame(E.ATR_LAYOUT_IMAGE, fb.data_ptr(), None, None, color.data_ptr(), None, None)
    eng.render_start(cam, [[0, 0, w - 1, h - 1]], fr, seed, stream=s.cuda_stream)
    assert eng.wait()[0] == 0
    normal, position, ident = eng.render_guides(cam)
    assert eng.wait()[0] == 0
    torch.cuda.synchronize()
    if args.live:  # the cost of a frame without sky
        sky = (ident == -1)[..., None]
        normal = torch.where(sky, torch.zeros_like(normal), normal)
        position = torch.where(sky, torch.zeros_like(position), position)
        ident = torch.zeros_like(ident)
        assert bool(torch.isfinite(normal).all() and torch.isfinite(position).all())
    return cam, color, (normal, position, ident)


class Case:
    def __init__(self, w, h):
        self.w, self.h, n = w, h, w * h
        acc = E.TemporalAccumulator(eng)
        for k in range(2):
            cam, color, guides = frame(w, h, k, SEED + k)
            self.color, self.variance = acc.push(cam, color, guides)
            assert eng.wait()[0] == 0
            torch.cuda.synchronize()
        self.guides, self.moments, self.length = guides, acc.prev["moments"], acc.prev["length"]
        self.live = int((self.length != 0).sum().item())
        self.short = int(((self.length != 0) & (self.length < defaults.spatial_below)).sum().item())
        self.out = torch.empty((h, w, 3), dtype=torch.float32, device=dev)
        self.vout = torch.empty((h, w), dtype=torch.float32, device=dev)
        self.src = torch.empty(n * (READ_B + WRITE_B) // 2, dtype=torch.uint8, device=dev)
        self.dst = torch.empty_like(self.src)
        self.ms = {"estimate_on": [], "estimate_off": [], "denoise": [], "copy": []}

    def call(self, name, keep, fn):
        fn()
        assert eng.wait()[0] == 0
        torch.cuda.synchronize()
        if keep:
            self.ms[name].append(eng.last_kernel_ms())

    def estimate_on(self, keep):
        self.call("estimate_on", keep, lambda: eng.denoise_variance(
            self.color, self.variance, *self.guides, moments=self.moments, length=self.length, out=self.out,
            variance_out=self.vout, framebuffer=True, stream=s.cuda_stream))

    def estimate_off(self, keep):
        self.call("estimate_off", keep, lambda: eng.denoise_variance(
            self.color, self.variance, *self.guides, out=self.out, variance_out=self.vout, framebuffer=True,
            stream=s.cuda_stream))

    def denoise(self, keep):
        self.call("denoise", keep, lambda: eng.denoise(self.color, *self.guides, passes=defaults.passes, out=self.out,
                                                       framebuffer=True, stream=s.cuda_stream))

    def copy(self, keep):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record(s)
        self.dst.copy_(self.src)
        e[1].record(s)
        torch.cuda.synchronize()
        if keep:
            self.ms["copy"].append(e[0].elapsed_time(e[1]))


cases = [Case(*[int(v) for v in size.split("x")]) for size in args.sizes.split(",")]
steps = [(c, f) for c in cases for f in (Case.estimate_on, Case.denoise, Case.estimate_off, Case.copy)]
for r in range(args.warmup + args.rounds):
    k = r % len(steps)
    for c, f in steps[k:] + steps[:k]:
        f(c, r >= args.warmup)
res = {"config": f"{args.asset} 1 spp x 3 bounces, two frames accumulated; normal, position, ident"
                 f"{' (every pixel live)' if args.live else ''}; default parameters (passes {defaults.passes}, "
                 f"sigma_luminance {defaults.sigma_luminance:g}, spatial_below {defaults.spatial_below}); out, "
                 "variance_out and framebuffer; atr_denoise: the same passes and guides, its other defaults",
       "rounds": args.rounds, "warmup": args.warmup}
for c in cases:
    row = {"pixels": c.w * c.h, "live_pixels": c.live, "pixels_below_spatial_below": c.short,
           "compulsory_bytes": c.w * c.h * (READ_B + WRITE_B)}
    for k, v in c.ms.items():
        row[k + "_ms"] = {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4),
                          "max": round(float(np.max(v)), 4)}
    for k in ("estimate_on", "estimate_off"):
        row[k + "_over_denoise"] = round(row[k + "_ms"]["median"] / row["denoise_ms"]["median"], 2)
        row[k + "_over_copy"] = round(row[k + "_ms"]["median"] / row["copy_ms"]["median"], 2)
    res[f"{c.w}x{c.h}"] = row
line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
eng.close()
