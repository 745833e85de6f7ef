"""What ray queries cost: atr_trace_rays on the Dragon surrogate with three batches
of about 2 M rays -- (a) the app camera's 1920x1080 primary rays in pixel order, built with torch
from the camera record, (b) the same rays shuffled, (c) second-generation rays: (a)'s hit points
with random unit directions -- each traced in input order (sort_bits 0) and in the tuning's default
order, on AUTO (the clustered scan) and LANE. For context the c3 render (atr_render_start of the same
camera, primary only) is timed in the same rounds. HIP events on one stream, the cases interleaved
in one process (their order rotating by round) after warm-up rounds; medians with min and max.
Prints one JSON line.

python tools/trace_rays_cost.py [--rounds N] [--warmup N] [--batches a,b,c] [--sorts 0,default]
                                [--variants auto,lane]
(the option lists narrow the run, e.g. for a kernel trace of one batch: the sort kernels' share of a
sorted call is the share of ray_query_keys, path_sort_* and ray_query_rank in that trace)"""
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
ap.add_argument("--batches", default="a,b,c")
ap.add_argument("--sorts", default="0,default")
ap.add_argument("--variants", default="auto,lane")
args = ap.parse_args()

W, H = (int(v) for v in args.size.split("x"))
SEED = 0x853C49E6748FEA9B
dev = torch.device("cuda", 0)
mesh = E.Mesh.load_obj(asset_path("Dragon"))
box = mesh.translate_to(mesh.aabb(), CENTERS["Dragon"])
tree = E.Octree.build(mesh, 300)
eng = E.Engine(0)
eng.upload([((0.3, 0.4, 0.5), (0.2, 0.3, 0.4), 0.3), ((0.4, 0.2, 0.2), (0.92, 0.5, 0.0), 0.3)], [(mesh, tree, box, 1)])
s = torch.cuda.current_stream(dev)
cam = E.camera(W, H)


def unit(v):  # engine.h unit(), f32
    m2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    return v * (1.0 / torch.sqrt(m2))[:, None]


def v3(a):
    return torch.tensor([a.x, a.y, a.z], dtype=torch.float32, device=dev)


def primary_rays():
    """The camera's rays in pixel order (renderer.cpp:317-351, as the kernels evaluate them)."""
    y, x = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                          torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    fy = (-1.0 + 2.0 * (y / float(H))).reshape(-1)
    fx = (((-1.0 + 2.0 * (x / float(W))) * cam.h_fov) * cam.aspect_ratio).reshape(-1)
    eye = v3(cam.eye)
    d = unit(((v3(cam.frame_center) + v3(cam.camera_x) * fx[:, None]) + v3(cam.camera_y) * fy[:, None]) - eye)
    return eye.expand(W * H, 3).contiguous(), d.contiguous()


gen = torch.Generator(device=dev)
gen.manual_seed(7)
oa, da = primary_rays()
out, _ = eng.trace_rays(oa, da, sort_bits=0, outputs=("t", "kind"))
eng.wait()
torch.cuda.synchronize()
hit = out["t"] < 3.0e38
invalid_a = int((out["kind"] == E.ATR_RAY_INVALID).sum())
perm = torch.randperm(W * H, device=dev, generator=gen)
ob, db = oa[perm].contiguous(), da[perm].contiguous()
# second generation: the hit points, repeated to the size of (a), random unit directions
hp = (oa[hit] + da[hit] * out["t"][hit][:, None])
oc = hp[torch.randint(0, hp.shape[0], (W * H,), device=dev, generator=gen)].contiguous()
dc = unit(torch.randn((W * H, 3), device=dev, generator=gen) + 1e-3).contiguous()
batches = {"a_primary": (oa, da), "b_shuffled": (ob, db), "c_second": (oc, dc)}
batches = {k: v for k, v in batches.items() if k[0] in args.batches.split(",")}
sorts = [(-1 if v == "default" else int(v)) for v in args.sorts.split(",")]
variants = [{"auto": E.ATR_KERNEL_AUTO, "lane": E.ATR_KERNEL_LANE}[v] for v in args.variants.split(",")]


class Query:
    def __init__(self, bname, variant, sort_bits):
        self.name = f"{bname}/{'lane' if variant == E.ATR_KERNEL_LANE else 'auto'}/sort{'_default' if sort_bits < 0 else sort_bits}"
        self.o, self.d = batches[bname]
        self.variant, self.sort_bits = variant, sort_bits
        self.ms, self.n = [], int(self.o.shape[0])
        self.traced = self.invalid = None

    def run(self, keep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        out, traced = eng.trace_rays(self.o, self.d, variant=self.variant, sort_bits=self.sort_bits,
                                     stream=s.cuda_stream, outputs=("t", "face", "kind"))
        e1.record(s)
        torch.cuda.synchronize()
        if keep:
            self.ms.append(e0.elapsed_time(e1))
        self.traced = int(traced.item())
        self.invalid = int((out["kind"] == E.ATR_RAY_INVALID).sum())
        self.hits = int((out["kind"] == E.ATR_RAY_TRI).sum())


class Render:
    name = "c3_render"

    def __init__(self):
        self.fb = torch.zeros(W * H, dtype=torch.int32, device=dev)
        self.fr = E.atr_frame(E.ATR_LAYOUT_IMAGE, self.fb.data_ptr(), None, None, None, None, None)
        self.ms, self.n = [], W * H

    def run(self, keep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        eng.render_start(cam, [[0, 0, W - 1, H - 1]], self.fr, SEED, stream=s.cuda_stream)
        e1.record(s)
        torch.cuda.synchronize()
        if keep:
            self.ms.append(e0.elapsed_time(e1))


cases = [Render()] + [Query(b, v, sb) for b in batches for v in variants for sb in sorts]
for r in range(args.warmup + args.rounds):
    k = r % len(cases)
    for c in cases[k:] + cases[:k]:
        c.run(r >= args.warmup)
rc, _ = eng.wait()
res = {"config": f"Dragon {W}x{H} app camera, {W * H} rays per batch", "rounds": args.rounds, "warmup": args.warmup,
       "wait_rc": rc, "tuning_path_sort_bits": eng.tuning()["path_sort_bits"], "primary_hits": int(hit.sum()),
       "primary_invalid": invalid_a}
for c in cases:
    med = float(np.median(c.ms))
    res[c.name] = {"median_ms": round(med, 4), "min_ms": round(float(np.min(c.ms)), 4),
                   "max_ms": round(float(np.max(c.ms)), 4), "mrays_per_s": round(c.n / med / 1e3, 1)}
    if isinstance(c, Query):
        res[c.name].update(traced=c.traced, invalid=c.invalid, tri_hits=c.hits)
print(json.dumps(res), flush=True)
eng.close()
