"""What sample passes cost: the 1080p, 64-spp, 5-bounce Dragon frame (bench.py's c4
shape, app camera) rendered (a) in one shot by atr_render_start_ex -- the entry point bench.py times
for its one-frame figure -- and (b) as the passes of renderer.sample_schedule(64) through
atr_render_start_samples, enqueued back to back; (c) is the time from the start of (b) until the
first pass's framebuffer is complete. HIP events on the render stream, A and B interleaved in one
process (their order alternating by round) after warm-up rounds; medians, with the spread. The two
framebuffers are compared at the end. Prints one JSON line.

python tools/progressive_cost.py [--rounds N] [--warmup N] [--spp N] [--passes a,b,...]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import atray_amd.engine as E  # noqa: E402
from atray_amd.assets import CENTERS, asset_path  # noqa: E402
from atray_amd.renderer import sample_schedule  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--bounces", type=int, default=5)
ap.add_argument("--size", default="1920x1080")
ap.add_argument("--passes", default="", help="pass sizes instead of sample_schedule(spp)")
args = ap.parse_args()

W, H = (int(v) for v in args.size.split("x"))
SEED = 0x853C49E6748FEA9B
passes = [int(v) for v in args.passes.split(",")] if args.passes else sample_schedule(args.spp)
assert sum(passes) == args.spp, passes
mesh = E.Mesh.load_obj(asset_path("Dragon"))
box = mesh.translate_to(mesh.aabb(), CENTERS["Dragon"])
tree = E.Octree.build(mesh, 300)
eng = E.Engine(0)
eng.upload([((0.3, 0.4, 0.5), (0.2, 0.3, 0.4), 0.3), ((0.4, 0.2, 0.2), (0.92, 0.5, 0.0), 0.3)], [(mesh, tree, box, 1)])
full = [[0, 0, W - 1, H - 1]]
s = torch.cuda.current_stream()
n = W * H


def frame():
    fb = torch.zeros(n, dtype=torch.int32, device="cuda")
    casts = torch.zeros(n, dtype=torch.int32, device="cuda")
    return fb, casts, E.atr_frame(E.ATR_LAYOUT_IMAGE, fb.data_ptr(), None, None, None, casts.data_ptr(), None)


fb_a, casts_a, fr_a = frame()
fb_b, casts_b, fr_b = frame()
ssum = torch.empty(3 * n, dtype=torch.float32, device="cuda")
cam = E.camera(W, H, args.spp, args.bounces)
pass_cams = [E.camera(W, H, k, args.bounces) for k in passes]


def ev():
    return torch.cuda.Event(enable_timing=True)


def one_shot():
    a, b = ev(), ev()
    a.record(s)
    eng.render_start(cam, full, fr_a, SEED, stream=s.cuda_stream)
    b.record(s)
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def in_passes():
    a, first_done, b = ev(), ev(), ev()
    a.record(s)
    first = 0
    for i, (k, c) in enumerate(zip(passes, pass_cams)):
        eng.render_start_samples(c, full, fr_b, SEED, first, ssum.data_ptr(), stream=s.cuda_stream)
        first += k
        if i == 0:
            first_done.record(s)
    b.record(s)
    torch.cuda.synchronize()
    return a.elapsed_time(b), a.elapsed_time(first_done)


ta, tb, tc = [], [], []
for r in range(args.warmup + args.rounds):
    if r % 2 == 0:
        x = one_shot()
        y, z = in_passes()
    else:
        y, z = in_passes()
        x = one_shot()
    if r >= args.warmup:
        ta.append(x)
        tb.append(y)
        tc.append(z)
rc, _ = eng.wait()


def stat(v):
    return {"median_ms": round(float(np.median(v)), 3), "min_ms": round(float(np.min(v)), 3),
            "max_ms": round(float(np.max(v)), 3)}


print(json.dumps({"config": f"Dragon {W}x{H} {args.spp} spp {args.bounces} bounces", "passes": passes,
                  "rounds": args.rounds, "warmup": args.warmup, "wait_rc": rc,
                  "a_one_shot": stat(ta), "b_passes_total": stat(tb), "c_first_pass_done": stat(tc),
                  "b_over_a": round(float(np.median(tb) / np.median(ta)), 4),
                  "b_over_a_per_round": [round(y / x, 4) for x, y in zip(ta, tb)],
                  "identical": bool(torch.equal(fb_a, fb_b) and torch.equal(casts_a, casts_b))}), flush=True)
eng.close()
