"""What a hemisphere radiance gather costs: atr_gather_radiance against what a caller did
before it -- the (point, sample) directions made ahead of time (atr_gather_occlusion's dirs output, the
same sampler on the same streams), the traced ones expanded to a ray array outside the timed range,
then atr_radiance_rays on those rays with one sample each. The workload and the sampler are the same;
the bits are not, because the composition keys each path's stream by its flattened ray index. Shapes:
the app camera's triangle hit points (surface_points; an evenly strided subset of at most --max-points)
at 16 and 256 samples, and a probe case of 64 points x 4,096 samples; the queue order off (sort_bits 0)
and at the tuning's default. Scenes: the Dragon surrogate and the tests' `mixed` scene. HIP events on one
stream, the cases interleaved in one process (their order rotating by round) after warm-up rounds;
medians with min and max. Prints one JSON line and, with --out, writes it there.

python tools/gather_radiance_cost.py [--rounds N] [--warmup N] [--scenes dragon,mixed] [--size WxH]
                                     [--bounces N] [--max-points N] [--only SHAPE] [--out FILE]"""
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
ap.add_argument("--bounces", type=int, default=5)
ap.add_argument("--max-points", type=int, default=1 << 19)
ap.add_argument("--only", default="", help="run the shapes whose name contains this (surface_16, probe, ...)")
ap.add_argument("--out", default="")
args = ap.parse_args()

W, H = (int(v) for v in args.size.split("x"))
BL = args.bounces
SEED = 0x853C49E6748FEA9B
SHAPES = (("surface", 16), ("surface", 256), ("probe", 4096))  # the probe case: 64 points
dev = torch.device("cuda", 0)
s = torch.cuda.current_stream(dev)


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


def surface(eng):
    """The app camera's triangle hit points and flipped normals, thinned evenly to --max-points."""
    oa, da = (torch.from_numpy(a).to(dev) for a in E.camera_rays(E.camera(W, H, 1, 1)))
    out, _ = eng.trace_rays(oa, da, sort_bits=0, outputs=("t", "kind", "normal"))
    eng.wait()
    torch.cuda.synchronize()
    tri = out["kind"] == E.ATR_RAY_TRI
    p, n = E.surface_points(oa[tri], da[tri], out["t"][tri], out["normal"][tri])
    hits = int(p.shape[0])
    if hits > args.max_points:
        keep = torch.linspace(0, hits - 1, args.max_points, device=dev).round().long()
        p, n = p[keep], n[keep]
    return p.contiguous(), n.contiguous(), hits


def composed_rays(eng, p, n, ns):
    """The composition's ray array: every traced (point, sample) of the gather's own directions."""
    out, _ = eng.gather_occlusion(p, n, ns, None, 0, 0, SEED, outputs=("dirs",))
    eng.wait()
    torch.cuda.synchronize()
    d = out["dirs"].reshape(-1, 3)
    o = p.repeat_interleave(ns, dim=0)
    up = (d * n.repeat_interleave(ns, dim=0)).sum(dim=1) > 0
    return o[up].contiguous(), d[up].contiguous()


class Case:
    def __init__(self, name, eng, p, n, ns, sort_bits, rays=None):
        self.name, self.eng, self.p, self.n, self.ns, self.sort_bits, self.rays = name, eng, p, n, ns, sort_bits, rays
        self.ms, self.traced, self.casts = [], None, None
        self.paths = int(p.shape[0]) * ns if rays is None else int(rays[0].shape[0])

    def run(self, keep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        if self.rays is None:
            out, traced = self.eng.gather_radiance(self.p, self.n, self.ns, BL, seed=SEED, sort_bits=self.sort_bits,
                                                   stream=s.cuda_stream, want=("rgb", "samples", "ray_casts"))
        else:
            out, traced = self.eng.radiance_rays(self.rays[0], self.rays[1], 1, BL, seed=SEED,
                                                 sort_bits=self.sort_bits, stream=s.cuda_stream,
                                                 want=("rgb", "ray_casts"))
        e1.record(s)
        torch.cuda.synchronize()
        if keep:
            self.ms.append(e0.elapsed_time(e1))
        self.traced = int(traced.item())
        self.casts = int(out["ray_casts"].to(torch.int64).sum())
        if self.rays is None:
            self.paths = int(out["samples"].to(torch.int64).sum())  # the traced samples


engines, cases = [], []
res = {"config": f"app camera {W}x{H}, {BL} bounces, at most {args.max_points} surface points",
       "rounds": args.rounds, "warmup": args.warmup}
for scene in args.scenes.split(","):
    eng = make_engine(scene)
    engines.append(eng)
    p, n, hits = surface(eng)
    pick = torch.linspace(0, int(p.shape[0]) - 1, 64, device=dev).round().long()
    sets = {"surface": (p, n), "probe": (p[pick].contiguous(), n[pick].contiguous())}
    res[scene] = {"triangle_hits": hits, "surface_points": int(p.shape[0]),
                  "default_sort_bits": eng.tuning()["path_sort_bits"]}
    for what, ns in SHAPES:
        if args.only not in f"{what}_{ns}":
            continue
        pp, nn = sets[what]
        rays = composed_rays(eng, pp, nn, ns)
        for sb, tag in ((0, "queue_order"), (-1, "sorted")):
            cases.append(Case(f"{scene}/{what}_{ns}/gather_{tag}", eng, pp, nn, ns, sb))
            cases.append(Case(f"{scene}/{what}_{ns}/composed_{tag}", eng, pp, nn, ns, sb, rays))
for r in range(args.warmup + args.rounds):
    k = r % len(cases)
    for c in cases[k:] + cases[:k]:
        c.run(r >= args.warmup)
res["wait_rc"] = [e.wait()[0] for e in engines]
for c in cases:
    med = float(np.median(c.ms))
    res[c.name] = {"median_ms": round(med, 4), "min_ms": round(float(np.min(c.ms)), 4),
                   "max_ms": round(float(np.max(c.ms)), 4), "points": int(c.p.shape[0]), "samples": c.ns,
                   "paths": c.paths, "mpaths_per_s": round(c.paths / med / 1e3, 1), "traced": c.traced,
                   "mrays_traced_per_s": round(c.traced / med / 1e3, 1), "casts_sum": c.casts}
for c in cases:  # gather / composed of the same shape and order
    if "/gather_" in c.name:
        other = res[c.name.replace("/gather_", "/composed_")]
        res[c.name]["vs_composed"] = round(res[c.name]["median_ms"] / other["median_ms"], 4)
line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
for e in engines:
    e.close()
