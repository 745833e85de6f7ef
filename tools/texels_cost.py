"""What the lightmap texel calls cost, and what share of a bake they are: the device
time of atr_mesh_texels and atr_texels_to_image for the Deer and for the n = 20 UV grid of the tests at
1,024 x 1,024 and 4,096 x 4,096 texels, and next to them the 64-sample atr_gather_occlusion on the same
texels (the mesh uploaded as the scene it is baked in). HIP events on one stream around the two
asynchronous calls; atr_mesh_texels is synchronous and reports its own event time (ms_out[1], the sum
of its three kernel groups) and its wall time. The cases are interleaved in one process, their order
rotating by round, after warm-up rounds; medians with min and max. Prints one JSON line and, with
--out, writes it there.

python tools/texels_cost.py [--rounds N] [--warmup N] [--sizes 1024,4096] [--samples N] [--passes N] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import atray_amd.engine as E  # noqa: E402
from atray_amd.assets import CENTERS, asset_path  # noqa: E402
from tests.test_texels_cpu import grid_obj  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--sizes", default="1024,4096")
ap.add_argument("--samples", type=int, default=64)
ap.add_argument("--passes", type=int, default=2)
ap.add_argument("--out", default="")
args = ap.parse_args()

SEED = 0x853C49E6748FEA9B
dev = torch.device("cuda", 0)
s = torch.cuda.current_stream(dev)
SKY, MODEL = ((0.3, 0.4, 0.5), (0.2, 0.3, 0.4), 0.3), ((0.4, 0.2, 0.2), (0.92, 0.5, 0.0), 0.3)


def make(name):
    eng = E.Engine(0)
    if name == "deer":
        mesh = E.Mesh.load_obj(asset_path("Deer"))
        box = mesh.translate_to(mesh.aabb(), CENTERS["Deer"])
    else:
        mesh = E.Mesh.parse_obj(grid_obj(20, 512, 512))
        box = mesh.aabb()
    eng.upload([SKY, MODEL], [(mesh, E.Octree.build(mesh, 300), box, 1)])
    return eng, mesh


class Case:
    def __init__(self, name, eng, mesh, side):
        self.name, self.eng, self.mesh, self.side = name, eng, mesh, side
        self.ms = {"texels_device": [], "texels_wall": [], "image": [], "gather": []}
        self.covered = 0

    def run(self, keep):
        tm = {}
        tex = self.eng.mesh_texels(self.mesh, self.side, self.side, timings=tm)
        self.covered = int(tex["texel"].shape[0])
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record(s)
        out, _ = self.eng.gather_occlusion(tex["point"], tex["normal"], args.samples, seed=SEED, stream=s.cuda_stream)
        e[1].record(s)
        vis, tot = out["visible"].to(torch.float32), (out["visible"] + out["occluded"]).to(torch.float32)
        values = (vis / torch.clamp(tot, min=1))[:, None].expand(-1, 3).contiguous()
        e[2].record(s)
        self.eng.texels_to_image(values, tex["texel"], self.side, self.side, passes=args.passes, stream=s.cuda_stream)
        e[3].record(s)
        torch.cuda.synchronize()
        if keep:
            self.ms["texels_device"].append(tm["device_ms"])
            self.ms["texels_wall"].append(tm["wall_ms"])
            self.ms["gather"].append(e[0].elapsed_time(e[1]))
            self.ms["image"].append(e[2].elapsed_time(e[3]))


scenes = {k: make(k) for k in ("deer", "grid20")}
cases = [Case(f"{k}/{side}", eng, mesh, side) for k, (eng, mesh) in scenes.items()
         for side in (int(v) for v in args.sizes.split(","))]
for r in range(args.warmup + args.rounds):
    k = r % len(cases)
    for c in cases[k:] + cases[:k]:
        c.run(r >= args.warmup)
res = {"config": f"{args.samples}-sample occlusion gather, {args.passes} dilation passes", "rounds": args.rounds,
       "warmup": args.warmup, "wait_rc": [eng.wait()[0] for eng, _ in scenes.values()]}
for c in cases:
    row = {"texels": c.side * c.side, "covered": c.covered, "faces": c.mesh.info()[2]}
    for k, v in c.ms.items():
        row[k + "_ms"] = {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4),
                          "max": round(float(np.max(v)), 4)}
    new = row["texels_device_ms"]["median"] + row["image_ms"]["median"]
    row["share_of_bake"] = round(new / (new + row["gather_ms"]["median"]), 4)
    res[c.name] = row
line = json.dumps(res)
print(line, flush=True)
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
for eng, _ in scenes.values():
    eng.close()
