"""What the primary kernels' leaf boxes take from a frame, counted on the host and by the
instrumented render. The oracle's leaf trace gives each pixel's scanned leaves in order; the row of
leaf boxes a launch reads (atr_camera_leaf_boxes_row: the host's real clusters and the table's folded
growths) is tested per (ray, leaf) in float32 numpy as trace.h leaf_box_miss does. From that: the
skipped (ray, leaf) visits, and per 8x8 cell the wave's leaf steps (the largest count of its lanes) and
DFS passes at kLeafBuf = 8 (one per started group of 8 steps), before and after. Next to them the GPU's
own count of skipped visits and unsound skips (atr_render_leaf_box_counters).

    python tools/leaf_box_estimate.py [--width 1920 --height 1080] [--asset Dragon --leaf 300] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from atray_amd import engine as E  # noqa: E402
from atray_amd.assets import CENTERS, asset_path, dragon_obj_path  # noqa: E402
from oracle import oracle as O  # noqa: E402

F = np.float32
K = 8  # trace.h kLeafBuf


def leaf_ranks(children):
    """host_scene.cpp inner_table: node -> discovery rank of a leaf (-1: inner)."""
    rank = np.full(len(children), -1, np.int64)
    nxt, stack = 0, [0]
    if children[0] == 0:
        rank[0], nxt = 0, 1
    while stack:
        c = int(children[stack.pop()])
        if not c:
            continue
        for k in range(8):
            if children[c + k] == 0:
                rank[c + k] = nxt
                nxt += 1
        for k in range(8):
            if children[c + k]:
                stack.append(c + k)
    return rank


def directions(cam):
    """render.hip's primary direction per pixel, in float32 (rounding may differ from the device's by an
    ulp in the square root: this is an estimate)."""
    W, H = cam.width, cam.height
    x, y = np.meshgrid(np.arange(W, dtype=F), np.arange(H, dtype=F))
    fy = F(-1.0) + F(2.0) * (y / F(H))
    fx = ((F(-1.0) + F(2.0) * (x / F(W))) * F(cam.h_fov)) * F(cam.aspect_ratio)
    v = lambda a: np.array([a.x, a.y, a.z], F)  # noqa: E731
    p = (v(cam.frame_center) + fx[..., None] * v(cam.camera_x)) + fy[..., None] * v(cam.camera_y) - v(cam.eye)
    l2 = (p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2]
    return (p * (F(1.0) / np.sqrt(l2))[..., None]).astype(F)


def cells(a, H, W):
    """(H, W) per-pixel counts -> per 8x8 cell maxima."""
    Hc, Wc = (H + 7) // 8, (W + 7) // 8
    pad = np.zeros((Hc * 8, Wc * 8), a.dtype)
    pad[:H, :W] = a
    return pad.reshape(Hc, 8, Wc, 8).max(axis=(1, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--asset", default="Dragon")
    ap.add_argument("--leaf", type=int, default=300)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    W, H = a.width, a.height
    path = dragon_obj_path() if a.asset == "Dragon" else asset_path(a.asset)
    mesh = E.Mesh.load_obj(path)
    box = mesh.translate_to(mesh.aabb(), CENTERS[a.asset])
    tree = E.Octree.build(mesh, a.leaf)
    eng = E.Engine(0)
    eng.upload([O.SKY, O.MODEL_MAT], [(mesh, tree, box, 1)])
    cam = E.camera(W, H)
    eye = (cam.eye.x, cam.eye.y, cam.eye.z)
    lo, hi, flag, _ = eng.camera_leaf_boxes_row(eye)
    whole = [[0, 0, W - 1, H - 1]]
    seed = 0x853C49E6748FEA9B
    gpu = {"counters": eng.counters(cam, whole, seed, E.ATR_KERNEL_HYBRID),
           "leaf_box": eng.leaf_box_counters(cam, whole, seed, E.ATR_KERNEL_HYBRID)}
    eng.close()

    s = O.Scene(path, center=CENTERS[a.asset], max_faces=a.leaf)
    leaves, _ = s.leaf_trace(O.Camera(W, H), cap=64)
    rank = leaf_ranks(tree.export()[1])
    valid = leaves >= 0
    assert valid.sum(axis=-1).max() < 64, "raise cap"
    lr = np.where(valid, rank[np.where(valid, leaves, 0)], 0)
    d = directions(cam)
    with np.errstate(all="ignore"):
        inv = (F(1.0) / d).astype(F)
    fin = np.isfinite(inv).all(axis=-1)
    o = np.array(eye, F)
    skip = np.zeros(valid.shape, bool)
    for j in range(valid.shape[-1]):  # the j-th scanned leaf of every pixel
        m = valid[..., j]
        if not m.any():
            break
        k = lr[..., j]
        with np.errstate(all="ignore"):
            x0, x1 = (lo[k] - o) * inv, (hi[k] - o) * inv
            tn = np.fmin(x0, x1).max(axis=-1)
            tf = np.fmax(x0, x1).min(axis=-1)
            miss = np.where(flag[k] == 0, (tn > tf) | (tf < F(0.0)), flag[k] == 1)
        skip[..., j] = m & fin & miss
    before, after = valid.sum(axis=-1), (valid & ~skip).sum(axis=-1)
    hit = s.primary_hits(O.Camera(W, H))[0] != 0xFFFFFFFF
    last = np.take_along_axis(skip, np.maximum(before - 1, 0)[..., None], axis=-1)[..., 0]
    cb, ca = cells(before, H, W), cells(after, H, W)
    passes = lambda c, any_ray: int((np.maximum((c + K - 1) // K, any_ray.astype(c.dtype))).sum())  # noqa: E731
    entered = cells(valid[..., 0].astype(np.int64), H, W) > 0  # a ray of the cell got a leaf: a first pass
    out = {
        "frame": [W, H], "asset": a.asset, "leaf": a.leaf,
        "host": {
            "rays_with_a_leaf": int(valid[..., 0].sum()), "hit_rays": int(hit.sum()),
            "visits": int(before.sum()), "skipped_visits": int(skip.sum()),
            "skipped_share": round(float(skip.sum()) / max(1, int(before.sum())), 4),
            "hit_rays_whose_hit_leaf_is_skipped": int((hit & last & (before > 0)).sum()),
            "wave_leaf_steps": [int(cb.sum()), int(ca.sum())],
            "wave_passes": [passes(cb, entered), passes(ca, entered)],
            "rays_scanning_more_than_8": [int((before > K).sum()), int((after > K).sum())],
            "cells_with_steps": int((cb > 0).sum()),
        },
        "gpu_count_build": gpu,
    }
    txt = json.dumps(out, indent=1)
    print(txt)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write(txt + "\n")


if __name__ == "__main__":
    main()
