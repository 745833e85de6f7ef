"""What occlusion queries cost: atr_occluded_rays against what a caller did before it,
atr_trace_rays with only t requested (same variant, same sort_bits), in the same rounds. Scenes: the
Dragon surrogate and the tests' `mixed` scene, both at the app camera, 1920x1080 rays per batch:
(a) the camera's primary rays in pixel order, t_max NULL; (c) second-generation rays ((a)'s hit points,
random unit directions), t_max NULL; (s1) shadow segments from (a)'s hit points to a point light above
the scene (segment_rays); (s2) the same segments cast from the light. HIP events on one stream, the
cases interleaved in one process (their order rotating by round) after warm-up rounds; medians with
min and max. Prints one JSON line.

python tools/occlusion_cost.py [--rounds N] [--warmup N] [--scenes dragon,mixed] [--batches a,c,s1,s2]
                               [--sorts 0,default] [--variants auto,lane]"""
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
ap.add_argument("--batches", default="a,c,s1,s2")
ap.add_argument("--sorts", default="0,default")
ap.add_argument("--variants", default="auto,lane")
args = ap.parse_args()

W, H = (int(v) for v in args.size.split("x"))
N = W * H
dev = torch.device("cuda", 0)
s = torch.cuda.current_stream(dev)
cam = E.camera(W, H)
gen = torch.Generator(device=dev)
gen.manual_seed(7)


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


def make_batches(eng):
    """name -> (orig, dirs, t_max or None), and what the batches are made of."""
    oa, da = primary_rays()
    out, _ = eng.trace_rays(oa, da, sort_bits=0, outputs=("t", "kind"))
    eng.wait()
    torch.cuda.synchronize()
    tri = out["kind"] == E.ATR_RAY_TRI  # points on the models (the mixed scene's floor plane is far below)
    hp = oa[tri] + da[tri] * out["t"][tri][:, None]
    pts = hp[torch.randint(0, hp.shape[0], (N,), device=dev, generator=gen)].contiguous()
    dc = unit(torch.randn((N, 3), device=dev, generator=gen) + 1e-3).contiguous()
    lo, hi = hp.min(dim=0).values, hp.max(dim=0).values
    light = (lo + hi) * 0.5
    light[1] = hi[1] + max(float(hi[1] - lo[1]), 1.0)  # above the hit points by their height
    lights = light.expand(N, 3).contiguous()
    b = {"a": (oa, da, None), "c": (pts, dc, None)}
    for k, (p, q) in (("s1", (pts, lights)), ("s2", (lights, pts))):
        o, d, tm = E.segment_rays(p, q)
        b[k] = (o.contiguous(), d.contiguous(), tm.contiguous())
    info = {"primary_tri_hits": int(tri.sum()), "light": [round(float(v), 3) for v in light]}
    return {k: v for k, v in b.items() if k in args.batches.split(",")}, info


class Case:
    def __init__(self, scene, eng, bname, batch, what, variant, sort_bits):
        vn = "lane" if variant == E.ATR_KERNEL_LANE else "auto"
        self.name = f"{scene}/{bname}/{what}/{vn}/sort{'_default' if sort_bits < 0 else sort_bits}"
        self.eng, self.what, self.variant, self.sort_bits = eng, what, variant, sort_bits
        self.o, self.d, self.tm = batch
        self.ms, self.n = [], int(self.o.shape[0])
        self.traced = self.share = None

    def run(self, keep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        if self.what == "occluded":
            out, traced = self.eng.occluded_rays(self.o, self.d, self.tm, variant=self.variant,
                                                 sort_bits=self.sort_bits, stream=s.cuda_stream)
        else:  # the caller's way before: the closest t, compared on its side
            res, traced = self.eng.trace_rays(self.o, self.d, variant=self.variant, sort_bits=self.sort_bits,
                                              stream=s.cuda_stream, outputs=("t",))
        e1.record(s)
        torch.cuda.synchronize()
        if keep:
            self.ms.append(e0.elapsed_time(e1))
        self.traced = int(traced.item())
        if self.what == "occluded":
            self.share = float((out == E.ATR_OCCL_OCCLUDED).float().mean())
        else:
            bound = self.tm if self.tm is not None else torch.full_like(res["t"], 3.0e38)
            self.share = float((res["t"] < bound).float().mean())


sorts = [(-1 if v == "default" else int(v)) for v in args.sorts.split(",")]
variants = [{"auto": E.ATR_KERNEL_AUTO, "lane": E.ATR_KERNEL_LANE}[v] for v in args.variants.split(",")]
engines, cases, res = {}, [], {"config": f"app camera {W}x{H}, {N} rays per batch", "rounds": args.rounds,
                               "warmup": args.warmup}
for scene in args.scenes.split(","):
    eng = engines[scene] = make_engine(scene)
    batches, info = make_batches(eng)
    res[scene] = dict(info, tuning_path_sort_bits=eng.tuning()["path_sort_bits"])
    for bname, batch in batches.items():
        for v in variants:
            for sb in sorts:
                for what in ("occluded", "closest_t"):
                    cases.append(Case(scene, eng, bname, batch, what, v, sb))
for r in range(args.warmup + args.rounds):
    k = r % len(cases)
    for c in cases[k:] + cases[:k]:
        c.run(r >= args.warmup)
res["wait_rc"] = [e.wait()[0] for e in engines.values()]
for c in cases:
    med = float(np.median(c.ms))
    res[c.name] = {"median_ms": round(med, 4), "min_ms": round(float(np.min(c.ms)), 4),
                   "max_ms": round(float(np.max(c.ms)), 4), "mrays_per_s": round(c.n / med / 1e3, 1),
                   "traced": c.traced, "below_bound_share": round(c.share, 4)}
print(json.dumps(res), flush=True)
for e in engines.values():
    e.close()
