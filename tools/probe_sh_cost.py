"""What light probes cost: atr_probe_sh against atr_gather_radiance at the same item
counts (the same points, the gather with their normals: a hemisphere's paths instead of a sphere's, the
parent commit's code), and against the composition the call replaces with its rays already on the
device -- the (probe, sample) directions made ahead of time (atr_probe_sh's own dirs output), expanded to
a ray array outside the timed range, then atr_radiance_rays with one sample per ray and the projection
on the nine basis functions in torch, both timed. The workload and the sampler are the same; the bits are
not, because the composition keys each path's stream by its flattened ray index and torch sums in its
own order. Shapes: 64 probes x 4,096 samples and 4,096 probes x 256 samples, at bounce limits 1 and 5,
on the Dragon surrogate; the points are the app camera's triangle hit points lifted 0.05 along their
normals, evenly strided. HIP events on one stream, the cases interleaved in one process (their order
rotating by round) after warm-up rounds; medians with min and max. --cases keeps the cases whose name
(PROBESxSAMPLES/bBOUNCES/KIND, KIND one of probe_sh, gather, composed) contains it: with one probe_sh
case alone under a kernel trace, the per-kernel totals give the resolve's share of the call. Prints one
JSON line and, with --out, writes it there.

python tools/probe_sh_cost.py [--rounds N] [--warmup N] [--size WxH] [--cases NAME] [--out FILE]"""
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
ap.add_argument("--cases", default="", help="run the cases whose name contains this (64x4096/b5/probe_sh, gather, ...)")
ap.add_argument("--out", default="")
args = ap.parse_args()

W, H = (int(v) for v in args.size.split("x"))
SEED = 0x853C49E6748FEA9B
SHAPES = ((64, 4096), (4096, 256))  # (probes, samples)
BOUNCES = (1, 5)
LIFT = 0.05
dev = torch.device("cuda", 0)
s = torch.cuda.current_stream(dev)
# the basis in torch, for the composition's projection (its own rounding: not the call's bits)
C1, C2, C6, C8 = 0.488602512, 1.092548431, 0.315391565, 0.546274215


def torch_basis(d):
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return torch.stack([torch.full_like(x, 0.282094792), C1 * y, C1 * z, C1 * x, C2 * (x * y), C2 * (y * z),
                        C6 * (3.0 * (z * z) - 1.0), C2 * (x * z), C8 * (x * x - y * y)], dim=1)


eng = E.Engine(0)
mesh = E.Mesh.load_obj(asset_path("Dragon"))
box = mesh.translate_to(mesh.aabb(), CENTERS["Dragon"])
eng.upload([((0.3, 0.4, 0.5), (0.2, 0.3, 0.4), 0.3), ((0.4, 0.2, 0.2), (0.92, 0.5, 0.0), 0.3)],
           [(mesh, E.Octree.build(mesh, 300), box, 1)])
oa, da = (torch.from_numpy(a).to(dev) for a in E.camera_rays(E.camera(W, H, 1, 1)))
hit, _ = eng.trace_rays(oa, da, sort_bits=0, outputs=("t", "kind", "normal"))
eng.wait()
torch.cuda.synchronize()
tri = hit["kind"] == E.ATR_RAY_TRI
sp, sn = E.surface_points(oa[tri], da[tri], hit["t"][tri], hit["normal"][tri])
sp = (sp + sn * LIFT).contiguous()


class Case:
    def __init__(self, name, kind, p, n, ns, bl, rays=None):
        self.name, self.kind, self.p, self.n, self.ns, self.bl, self.rays = name, kind, p, n, ns, bl, rays
        self.ms, self.traced, self.casts = [], None, None
        self.paths = int(p.shape[0]) * ns

    def run(self, keep):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        if self.kind == "probe_sh":
            out, traced = eng.probe_sh(self.p, self.ns, self.bl, seed=SEED, stream=s.cuda_stream,
                                       want=("sh", "ray_casts", "invalid"))
        elif self.kind == "gather":
            out, traced = eng.gather_radiance(self.p, self.n, self.ns, self.bl, seed=SEED, stream=s.cuda_stream,
                                              want=("rgb", "samples", "ray_casts"))
        else:
            o, d = self.rays
            out, traced = eng.radiance_rays(o, d, 1, self.bl, seed=SEED, stream=s.cuda_stream,
                                            want=("rgb", "ray_casts"))
            y = torch_basis(d).reshape(-1, self.ns, 9)
            rgb = out["rgb"].reshape(-1, self.ns, 3)
            out["sh"] = torch.einsum("psk,psc->pkc", y, rgb) * (12.566370614 / self.ns)
        e1.record(s)
        torch.cuda.synchronize()
        if keep:
            self.ms.append(e0.elapsed_time(e1))
        self.traced = int(traced.item())
        self.casts = int(out["ray_casts"].to(torch.int64).sum())


cases = []
res = {"config": f"Dragon, app camera {W}x{H}: its triangle hit points lifted {LIFT} along the normal",
       "rounds": args.rounds, "warmup": args.warmup, "default_sort_bits": eng.tuning()["path_sort_bits"],
       "triangle_hits": int(sp.shape[0])}
for npts, ns in SHAPES:
    pick = torch.linspace(0, int(sp.shape[0]) - 1, npts, device=dev).round().long()
    p, n = sp[pick].contiguous(), sn[pick].contiguous()
    d, _ = eng.probe_sh(p, ns, 1, seed=SEED, want=("dirs",))
    eng.wait()
    torch.cuda.synchronize()
    rays = (p.repeat_interleave(ns, dim=0).contiguous(), d["dirs"].reshape(-1, 3).contiguous())
    for bl in BOUNCES:
        for kind in ("probe_sh", "gather", "composed"):
            name = f"{npts}x{ns}/b{bl}/{kind}"
            if args.cases in name:
                cases.append(Case(name, kind, p, n, ns, bl, rays if kind == "composed" else None))
for r in range(args.warmup + args.rounds):
    k = r % len(cases)
    for c in cases[k:] + cases[:k]:
        c.run(r >= args.warmup)
res["wait_rc"] = eng.wait()[0]
for c in cases:
    med = float(np.median(c.ms))
    res[c.name] = {"median_ms": round(med, 4), "min_ms": round(float(np.min(c.ms)), 4),
                   "max_ms": round(float(np.max(c.ms)), 4), "points": int(c.p.shape[0]), "samples": c.ns,
                   "paths": c.paths, "mpaths_per_s": round(c.paths / med / 1e3, 1), "traced": c.traced,
                   "mrays_traced_per_s": round(c.traced / med / 1e3, 1), "casts_sum": c.casts}
for c in cases:  # probe_sh over the gather and over the composition of the same shape
    if c.kind == "probe_sh":
        for other in ("gather", "composed"):
            o = res.get(c.name.replace("/probe_sh", "/" + other))
            if o:
                res[c.name]["vs_" + other] = round(res[c.name]["median_ms"] / o["median_ms"], 4)
line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
eng.close()
