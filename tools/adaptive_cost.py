"""What adaptive passes cost and save: the 1080p, 5-bounce Dragon frame (bench.py's
c4 shape, app camera) rendered as the passes 4, 4, 8, 16, 32 (a) through atr_render_start_samples --
whose kernels adaptive sampling left unchanged --, (b) through atr_render_start_adaptive at
tolerance 0, which skips nothing: the price of the live list, and (c) at tolerances that stop
pixels, each with the fraction of the 64 x pixels samples actually rendered. The passes of a case
are enqueued back to back; HIP events on the render stream, the cases interleaved in one process
(their order rotating by round) after warm-up rounds; medians, with the spread. With --per-pass every
pass of every case is timed too (an event between passes). Prints one JSON line.

python tools/adaptive_cost.py [--rounds N] [--warmup N] [--passes a,b,...] [--tolerances x,y,...]"""
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
ap.add_argument("--bounces", type=int, default=5)
ap.add_argument("--size", default="1920x1080")
ap.add_argument("--passes", default="4,4,8,16,32")
ap.add_argument("--tolerances", default="0.005,0.01,0.02")
ap.add_argument("--per-pass", action="store_true")
args = ap.parse_args()

W, H = (int(v) for v in args.size.split("x"))
SEED = 0x853C49E6748FEA9B
passes = [int(v) for v in args.passes.split(",")]
spp = sum(passes)
mesh = E.Mesh.load_obj(asset_path("Dragon"))
box = mesh.translate_to(mesh.aabb(), CENTERS["Dragon"])
tree = E.Octree.build(mesh, 300)
eng = E.Engine(0)
eng.upload([((0.3, 0.4, 0.5), (0.2, 0.3, 0.4), 0.3), ((0.4, 0.2, 0.2), (0.92, 0.5, 0.0), 0.3)], [(mesh, tree, box, 1)])
full = [[0, 0, W - 1, H - 1]]
s = torch.cuda.current_stream()
n = W * H
pass_cams = [E.camera(W, H, k, args.bounces) for k in passes]


class Case:
    def __init__(self, name, tolerance):
        self.name, self.tol = name, tolerance
        self.fb = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.casts = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.sum = torch.empty(3 * n, dtype=torch.float32, device="cuda")
        self.count = torch.empty(n, dtype=torch.int32, device="cuda")
        self.fr = E.atr_frame(E.ATR_LAYOUT_IMAGE, self.fb.data_ptr(), None, None, None, self.casts.data_ptr(), None)
        self.ms, self.pass_ms, self.live = [], [], None

    def run(self, keep):
        evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(passes) + 1)]
        evs[0].record(s)
        first = 0
        for i, (k, c) in enumerate(zip(passes, pass_cams)):
            if self.tol is None:
                eng.render_start_samples(c, full, self.fr, SEED, first, self.sum.data_ptr(), stream=s.cuda_stream)
            else:
                eng.render_start_adaptive(c, full, self.fr, SEED, first, self.sum.data_ptr(), self.count.data_ptr(),
                                          self.tol, stream=s.cuda_stream)
            first += k
            if args.per_pass or i == len(passes) - 1:
                evs[i + 1].record(s)
        torch.cuda.synchronize()
        if keep:
            self.ms.append(evs[0].elapsed_time(evs[-1]))
            if args.per_pass:
                self.pass_ms.append([evs[i].elapsed_time(evs[i + 1]) for i in range(len(passes))])
        if self.tol is not None:
            self.live = eng.adaptive_info()[3]

    def report(self):
        r = {"median_ms": round(float(np.median(self.ms)), 3), "min_ms": round(float(np.min(self.ms)), 3),
             "max_ms": round(float(np.max(self.ms)), 3)}
        if self.pass_ms:
            r["pass_median_ms"] = [round(float(v), 3) for v in np.median(np.array(self.pass_ms), axis=0)]
        if self.tol is not None:
            cnt = self.count.cpu().numpy().view(np.uint32) & np.uint32(E.ATR_SAMPLES_CONVERGED - 1)
            r["tolerance"] = self.tol
            r["sample_fraction"] = round(float(cnt.astype(np.int64).sum()) / (spp * n), 4)
            r["pixels_live_at_end"] = self.live
        return r


cases = [Case("a_samples", None), Case("b_adaptive_tol0", 0.0)]
cases += [Case(f"c_adaptive_tol{t}", float(t)) for t in args.tolerances.split(",") if t]
for r in range(args.warmup + args.rounds):
    k = r % len(cases)
    for c in cases[k:] + cases[:k]:
        c.run(r >= args.warmup)
rc, _ = eng.wait()
out = {"config": f"Dragon {W}x{H} {spp} spp {args.bounces} bounces", "passes": passes, "rounds": args.rounds,
       "warmup": args.warmup, "wait_rc": rc}
a = float(np.median(cases[0].ms))
for c in cases:
    out[c.name] = c.report()
    if c is not cases[0]:
        out[c.name]["over_a"] = round(float(np.median(c.ms)) / a, 4)
        out[c.name]["over_a_per_round"] = [round(y / x, 4) for x, y in zip(cases[0].ms, c.ms)]
out["tol0_identical"] = bool(torch.equal(cases[0].fb, cases[1].fb) and torch.equal(cases[0].casts, cases[1].casts))
print(json.dumps(out), flush=True)
eng.close()
