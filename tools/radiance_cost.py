"""What radiance along caller rays costs: atr_radiance_rays on the app camera's own
1920x1080 rays (camera_rays) at 16 samples and 5 bounces, with the queue order on and off, against the
only way to get those bits before it -- atr_render_start_ex (PATHS) of the same camera -- in the same
rounds; then on second-generation rays (the camera's triangle hits through surface_points, one diffuse
direction each from gather_directions), where no yardstick exists. Scenes: the Dragon surrogate and the
tests' `mixed` scene. HIP events on one stream, the cases interleaved in one process (their order
rotating by round) after warm-up rounds; medians with min and max. Prints one JSON line.

python tools/radiance_cost.py [--rounds N] [--warmup N] [--scenes dragon,mixed] [--size WxH]
                              [--samples N] [--bounces N]"""
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
ap.add_argument("--size", default="1920x1080")
ap.add_argument("--scenes", default="dragon,mixed")
ap.add_argument("--samples", type=int, default=16)
ap.add_argument("--bounces", type=int, default=5)
args = ap.parse_args()

W, H = (int(v) for v in args.size.split("x"))
N, NS, BL = W * H, args.samples, args.bounces
SEED = 0x853C49E6748FEA9B
dev = torch.device("cuda", 0)
s = torch.cuda.current_stream(dev)
cam = E.camera(W, H, NS, BL)


def make_engine(name):
    eng = E.Engine(0)
    if name == "dragon":
        mesh = E.Mesh.load_obj(asset_path("Dragon"))
        box = mesh.translate_to(mesh.aabb(), CENTERS["Dragon"])
        eng.upload([((0.3, 0.4, 0.5), (0.2, 0.3, 0.4), 0.3), ((0.4, 0.2, 0.2), (0.92, 0.5, 0.0), 0.3)],
                   [(mesh, E.Octree.build(mesh, 300), box, 1)])
    else:
        from tests.test_gpu_scenes import MIXED
        MIXED.upload(eng)
    return eng


def second_generation(eng, oa, da):
    """The camera's triangle hits, one diffuse direction each (the traced ones of gather_directions)."""
    out, _ = eng.trace_rays(oa, da, sort_bits=0, outputs=("t", "kind", "normal"))
    eng.wait()
    torch.cuda.synchronize()
    tri = out["kind"] == E.ATR_RAY_TRI
    p, n = E.surface_points(oa[tri], da[tri], out["t"][tri], out["normal"][tri])
    d, t = E.gather_directions(n.cpu().numpy(), 1, seed=SEED)
    keep = torch.from_numpy(t.reshape(-1).astype(bool)).to(dev)
    return p[keep].contiguous(), torch.from_numpy(d.reshape(-1, 3)).to(dev)[keep].contiguous()


class Case:
    def __init__(self, scene, eng, what, rays=None, sort_bits=-1):
        self.name = f"{scene}/{what}"
        self.eng, self.what, self.rays, self.sort_bits = eng, what, rays, sort_bits
        self.ms, self.traced, self.check = [], None, None
        self.nrays = N if rays is None else int(rays[0].shape[0])
        if rays is None:  # the render: its frame, allocated once
            self.fb = torch.zeros(N, dtype=torch.int32, device=dev)
            self.rgb = torch.zeros(3 * N, dtype=torch.float32, device=dev)
            self.casts = torch.zeros(N, dtype=torch.int32, device=dev)

    def run(self, keep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        if self.rays is None:
            traced = torch.zeros(1, dtype=torch.int64, device=dev)
            fr = E.atr_frame(E.ATR_LAYOUT_IMAGE, self.fb.data_ptr(), None, None, self.rgb.data_ptr(),
                             self.casts.data_ptr(), traced.data_ptr())
            self.eng.render_start(cam, [[0, 0, W - 1, H - 1]], fr, SEED, stream=s.cuda_stream,
                                  variant=E.ATR_KERNEL_PATHS)
            rgb, casts = self.rgb, self.casts
        else:
            out, traced = self.eng.radiance_rays(self.rays[0], self.rays[1], NS, BL, seed=SEED,
                                                 sort_bits=self.sort_bits, stream=s.cuda_stream,
                                                 want=("rgb", "ray_casts"))
            rgb, casts = out["rgb"], out["ray_casts"]
        e1.record(s)
        torch.cuda.synchronize()
        if keep:
            self.ms.append(e0.elapsed_time(e1))
        self.traced = int(traced.item())
        self.paths = self.nrays * NS
        # what the outputs were: compared between the cases of one ray set after the rounds
        self.check = (int(casts.to(torch.int64).sum()), int(rgb.view(torch.int32).to(torch.int64).sum()))


engines, cases = [], []
res = {"config": f"app camera {W}x{H}, {NS} samples, {BL} bounces", "rounds": args.rounds, "warmup": args.warmup}
for scene in args.scenes.split(","):
    eng = make_engine(scene)
    engines.append(eng)
    oa, da = (torch.from_numpy(a).to(dev) for a in E.camera_rays(cam))
    second = second_generation(eng, oa, da)
    res[scene] = {"camera_rays": N, "second_generation_rays": int(second[0].shape[0])}
    cases += [Case(scene, eng, "camera/render_paths"),
              Case(scene, eng, "camera/radiance_sorted", (oa, da), -1),
              Case(scene, eng, "camera/radiance_queue_order", (oa, da), 0),
              Case(scene, eng, "second/radiance_sorted", second, -1),
              Case(scene, eng, "second/radiance_queue_order", second, 0)]
for r in range(args.warmup + args.rounds):
    k = r % len(cases)
    for c in cases[k:] + cases[:k]:
        c.run(r >= args.warmup)
res["wait_rc"] = [e.wait()[0] for e in engines]
for c in cases:
    med = float(np.median(c.ms))
    res[c.name] = {"median_ms": round(med, 4), "min_ms": round(float(np.min(c.ms)), 4),
                   "max_ms": round(float(np.max(c.ms)), 4), "rays": c.nrays,
                   "mpaths_per_s": round(c.paths / med / 1e3, 1), "traced": c.traced,
                   "mrays_traced_per_s": round(c.traced / med / 1e3, 1), "casts_sum": c.check[0],
                   "rgb_bits_sum": c.check[1]}
print(json.dumps(res), flush=True)
for e in engines:
    e.close()
