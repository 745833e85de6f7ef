"""What atr_denoise costs: the Dragon frame (4 spp, 5 bounces) at 1920 x 1080 and 3840 x
2160, rendered and given its guides (render_guides) on the device, then filtered with all three guides
and the default parameters into `out` and the framebuffer. Per size: atr_last_kernel_ms of the call, and
in the same run two yardsticks under HIP events: a device-to-device copy that moves the call's
compulsory bytes (40 B read and 16 B written per pixel: a copy of 28 B per pixel), and
atr_texels_to_image with 5 dilation passes on a fully covered map of the same size. The three are
interleaved, their order rotating by round, after warm-up rounds; medians with min and max. The
per-pass kernel times come from running this script under a kernel trace (the script after `--`, no
counters in that run); the kernels are denoise_pack_kernel and denoise_pass_kernel<normal, position,
colour>, the passes in launch order. Prints one JSON line and, with --out, writes it there.

--live makes every pixel live (the sky's guides zeroed, ident 0 everywhere): the Dragon covers 14 % of its
frame, and an inert pixel costs a pass one record read and one written.

python tools/denoise_bench.py [--rounds N] [--warmup N] [--sizes 1920x1080,3840x2160] [--live] [--out FILE]"""
import argparse
import json
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
READ_B, WRITE_B = 40, 16  # per pixel: colour, normal, position 12 B each and ident 4 B; out 12 B, framebuffer 4 B
if not torch.cuda.is_available():
    sys.exit("denoise_bench: no GPU")
dev = torch.device("cuda", 0)
s = torch.cuda.current_stream(dev)

eng = E.Engine(0)
mesh = E.Mesh.load_obj(asset_path(args.asset))
box = mesh.translate_to(mesh.aabb(), CENTERS[args.asset])
eng.upload([SKY, MODEL], [(mesh, E.Octree.build(mesh, 300), box, 1)])


class Case:
    def __init__(self, w, h):
        self.w, self.h, n = w, h, w * h
        cam = E.camera(w, h, 4, 5)
        fb = torch.zeros(n, dtype=torch.int32, device=dev)
        self.color = torch.zeros((h, w, 3), dtype=torch.float32, device=dev)
        fr = E.atr_frame(E.ATR_LAYOUT_IMAGE, fb.data_ptr(), None, None, self.color.data_ptr(), None, None)
        eng.render_start(cam, [[0, 0, w - 1, h - 1]], fr, SEED, stream=s.cuda_stream)
        assert eng.wait()[0] == 0
        self.normal, self.position, self.ident = eng.render_guides(E.camera(w, h))
        assert eng.wait()[0] == 0
        torch.cuda.synchronize()
        if args.live:  # the cost of a frame without sky, or of a fully covered lightmap
            sky = (self.ident == -1)[..., None]
            self.normal = torch.where(sky, torch.zeros_like(self.normal), self.normal)
            self.position = torch.where(sky, torch.zeros_like(self.position), self.position)
            self.ident = torch.zeros_like(self.ident)
            assert bool(torch.isfinite(self.normal).all() and torch.isfinite(self.position).all())
        self.live = int((self.ident != -1).sum().item())
        self.out = torch.empty_like(self.color)
        self.src = torch.empty(n * (READ_B + WRITE_B) // 2, dtype=torch.uint8, device=dev)
        self.dst = torch.empty_like(self.src)
        self.values = torch.rand((n, 3), dtype=torch.float32, device=dev)
        self.texel = torch.arange(n, dtype=torch.int32, device=dev)
        self.ms = {"denoise_kernels": [], "denoise_events": [], "copy": [], "texels_to_image_5": []}

    def denoise(self, keep):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record(s)
        eng.denoise(self.color, self.normal, self.position, self.ident, out=self.out, framebuffer=True,
                    stream=s.cuda_stream)
        e[1].record(s)
        assert eng.wait()[0] == 0
        torch.cuda.synchronize()
        if keep:
            self.ms["denoise_kernels"].append(eng.last_kernel_ms())
            self.ms["denoise_events"].append(e[0].elapsed_time(e[1]))

    def copy(self, keep):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record(s)
        self.dst.copy_(self.src)
        e[1].record(s)
        torch.cuda.synchronize()
        if keep:
            self.ms["copy"].append(e[0].elapsed_time(e[1]))

    def image(self, keep):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        e[0].record(s)
        eng.texels_to_image(self.values, self.texel, self.w, self.h, passes=5, stream=s.cuda_stream)
        e[1].record(s)
        assert eng.wait()[0] == 0
        torch.cuda.synchronize()
        if keep:
            self.ms["texels_to_image_5"].append(e[0].elapsed_time(e[1]))


cases = [Case(*[int(v) for v in size.split("x")]) for size in args.sizes.split(",")]
steps = [(c, f) for c in cases for f in (Case.denoise, Case.copy, Case.image)]
for r in range(args.warmup + args.rounds):
    k = r % len(steps)
    for c, f in steps[k:] + steps[:k]:
        f(c, r >= args.warmup)
res = {"config": f"{args.asset} 4 spp x 5 bounces; normal, position, ident{' (every pixel live)' if args.live else ''}; "
                 "default parameters; out and framebuffer",
       "rounds": args.rounds, "warmup": args.warmup}
for c in cases:
    row = {"pixels": c.w * c.h, "live_pixels": c.live, "compulsory_bytes": c.w * c.h * (READ_B + WRITE_B)}
    for k, v in c.ms.items():
        row[k + "_ms"] = {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4),
                          "max": round(float(np.max(v)), 4)}
    row["denoise_over_copy"] = round(row["denoise_kernels_ms"]["median"] / row["copy_ms"]["median"], 2)
    row["denoise_over_texels_to_image_5"] = round(row["denoise_kernels_ms"]["median"] /
                                                  row["texels_to_image_5_ms"]["median"], 2)
    res[f"{c.w}x{c.h}"] = row
line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
eng.close()
