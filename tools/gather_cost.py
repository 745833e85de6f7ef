"""What a hemisphere gather costs: atr_gather_occlusion against what a caller did before
it -- atr_occluded_rays in input order on the very same rays, made beforehand with gather_directions
(the traced samples only) and uploaded outside the timing -- in the same rounds. Scenes: the Dragon
surrogate and the tests' `mixed` scene; the points are the app camera's 1920x1080 triangle hits with
their flipped normals (surface_points), gathered at 16, 64 and 256 samples without a radius and with
one (a quarter of the hit points' box diagonal). HIP events on one stream, the cases interleaved in one
process (their order rotating by round) after warm-up rounds; medians with min and max. Prints one
JSON line.

python tools/gather_cost.py [--rounds N] [--warmup N] [--scenes dragon,mixed] [--samples 16,64,256]
                            [--variants auto,lane] [--max-points N]"""
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
ap.add_argument("--samples", default="16,64,256")
ap.add_argument("--variants", default="auto")
ap.add_argument("--max-points", type=int, default=0, help="keep the first N hit points (0: all)")
args = ap.parse_args()

W, H = (int(v) for v in args.size.split("x"))
N = W * H
SEED = 0x853C49E6748FEA9B
dev = torch.device("cuda", 0)
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
    return eye.expand(N, 3).contiguous(), d.contiguous()


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


def make_points(eng):
    """The camera's triangle hits as gather input: (points, normals, radius) and what they are."""
    oa, da = primary_rays()
    out, _ = eng.trace_rays(oa, da, sort_bits=0, outputs=("t", "kind", "normal"))
    eng.wait()
    torch.cuda.synchronize()
    tri = out["kind"] == E.ATR_RAY_TRI  # points on the models (the mixed scene's floor plane is far below)
    p, n = E.surface_points(oa[tri], da[tri], out["t"][tri], out["normal"][tri])
    if args.max_points:
        p, n = p[:args.max_points], n[:args.max_points]
    p, n = p.contiguous(), n.contiguous()
    ext = p.max(dim=0).values - p.min(dim=0).values
    radius = 0.25 * float(torch.sqrt((ext * ext).sum()))
    return p, n, radius, {"points": int(p.shape[0]), "radius": round(radius, 4)}


class Case:
    def __init__(self, scene, eng, what, p, n, ns, tm, variant, rays=None):
        vn = "lane" if variant == E.ATR_KERNEL_LANE else "auto"
        self.name = f"{scene}/s{ns}/{'radius' if tm is not None else 'free'}/{what}/{vn}"
        self.eng, self.what, self.variant, self.ns = eng, what, variant, ns
        self.p, self.n, self.tm, self.rays = p, n, tm, rays
        self.ms, self.items = [], int(p.shape[0]) * ns
        self.traced = self.share = None

    def run(self, keep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        if self.what == "rays":  # the caller's way before: a ray array, a byte per ray, reduced on its side
            o, d, t = self.rays
            out, traced = self.eng.occluded_rays(o, d, t, variant=self.variant, sort_bits=0, stream=s.cuda_stream)
        else:
            out, traced = self.eng.gather_occlusion(self.p, self.n, self.ns, self.tm, seed=SEED, variant=self.variant,
                                                    stream=s.cuda_stream)
        e1.record(s)
        torch.cuda.synchronize()
        if keep:
            self.ms.append(e0.elapsed_time(e1))
        self.traced = int(traced.item())
        if self.what == "rays":
            self.share = float((out == E.ATR_OCCL_OCCLUDED).sum()) / max(self.traced, 1)
        else:
            self.share = float(out["occluded"].sum()) / max(self.traced, 1)


def make_rays(p, n, ns, tm):
    """The gather's traced samples as a ray batch on the device: gather_directions on the host."""
    d, t = E.gather_directions(n.cpu().numpy(), ns, seed=SEED)
    keep = torch.from_numpy(t.reshape(-1).astype(bool))
    dirs = torch.from_numpy(d.reshape(-1, 3))[keep].to(dev).contiguous()
    keep = keep.to(dev)
    orig = p.repeat_interleave(ns, dim=0)[keep].contiguous()
    tmax = None if tm is None else tm.repeat_interleave(ns)[keep].contiguous()
    return orig, dirs, tmax


variants = [{"auto": E.ATR_KERNEL_AUTO, "lane": E.ATR_KERNEL_LANE}[v] for v in args.variants.split(",")]
samples = [int(v) for v in args.samples.split(",")]
engines, cases = [], []
res = {"config": f"app camera {W}x{H}, its triangle hits as points", "rounds": args.rounds, "warmup": args.warmup}
for scene in args.scenes.split(","):
    eng = make_engine(scene)
    engines.append(eng)
    p, n, radius, info = make_points(eng)
    res[scene] = info
    for ns in samples:
        for tm in (None, torch.full((p.shape[0],), radius, dtype=torch.float32, device=dev)):
            rays = make_rays(p, n, ns, tm)
            for v in variants:
                cases.append(Case(scene, eng, "gather", p, n, ns, tm, v))
                cases.append(Case(scene, eng, "rays", p, n, ns, tm, v, rays))
for r in range(args.warmup + args.rounds):
    k = r % len(cases)
    for c in cases[k:] + cases[:k]:
        c.run(r >= args.warmup)
res["wait_rc"] = [e.wait()[0] for e in engines]
for c in cases:
    med = float(np.median(c.ms))
    res[c.name] = {"median_ms": round(med, 4), "min_ms": round(float(np.min(c.ms)), 4),
                   "max_ms": round(float(np.max(c.ms)), 4), "msamples_per_s": round(c.items / med / 1e3, 1),
                   "traced": c.traced, "occluded_share": round(c.share, 4)}
print(json.dumps(res), flush=True)
for e in engines:
    e.close()
