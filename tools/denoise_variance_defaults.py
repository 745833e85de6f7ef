"""The grid behind atr_denoise_variance's defaults, on the CPU reference: the two-plane
image of tests/test_denoise_variance_cpu.py (noise sd 0.02 and 0.2, true variance supplied), seeds 0, 1, 2.
Prints, per grid point, the whole-image and per-plane mean squared errors and whether the point meets
(a) each plane better than unfiltered and (b) the whole image better than atr_denoise at every
sigma_color in {0.01, 0.05, 0.2, 1} x passes {3, 5}; then the point with the lowest worst-seed error
among those that meet both on all seeds. With --monkey: the reference on the last accumulated frame of
tests/test_accumulate_cpu.py's Monkey orbit, beside the accumulated frame and atr_denoise.

    python tools/denoise_variance_defaults.py [--monkey]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import denoise_ref as DR  # noqa: E402
from tests import denoise_variance_ref as VR  # noqa: E402
from tests.test_denoise_variance_cpu import mse, two_plane_image  # noqa: E402

SEEDS = (0, 1, 2)
FIXED = dict(sigma_position=0.0, normal_power_log2=5, spatial_below=4)


def grid():
    data = {s: two_plane_image(s) for s in SEEDS}
    rivals, plain = {}, {}
    print("| seed | unfiltered: whole | quiet plane | noisy plane | atr_denoise: best (passes, sigma_color) | worst |")
    print("|---|---|---|---|---|---|")
    for s, (clean, noisy, var, (n, p, i), right) in data.items():
        rivals[s] = {(ps, sc): mse(DR.denoise(noisy, n, p, i, passes=ps, sigma_color=sc, sigma_position=0.0,
                                               normal_power_log2=5)[0], clean)
                     for ps in (3, 5) for sc in (0.01, 0.05, 0.2, 1.0)}
        plain[s] = (mse(noisy, clean), mse(noisy, clean, ~right), mse(noisy, clean, right))
        best = min(rivals[s], key=rivals[s].get)
        print(f"| {s} | {plain[s][0]:.3e} | {plain[s][1]:.3e} | {plain[s][2]:.3e} | {rivals[s][best]:.3e} {best} | "
              f"{max(rivals[s].values()):.3e} |")
    print()
    print("| passes | sigma_luminance | luminance_floor | whole image, seeds 0 / 1 / 2 | quiet plane | noisy plane | (a) | (b) |")
    print("|---|---|---|---|---|---|---|---|")
    ok = {}
    for passes in (3, 5):
        for sl in (1.0, 2.0, 4.0, 8.0):
            for fl in (1e-4, 1e-3, 1e-2):
                whole, quiet, loud, a, b = [], [], [], True, True
                for s, (clean, noisy, var, (n, p, i), right) in data.items():
                    out = VR.denoise_variance(noisy, var, n, p, i, passes=passes, sigma_luminance=sl, luminance_floor=fl,
                                              **FIXED)[0]
                    whole.append(mse(out, clean)), quiet.append(mse(out, clean, ~right)), loud.append(mse(out, clean, right))
                    a &= quiet[-1] < plain[s][1] and loud[-1] < plain[s][2]
                    b &= all(whole[-1] < e for e in rivals[s].values())
                fmt = lambda v: " / ".join(f"{x:.3e}" for x in v)  # noqa: E731
                print(f"| {passes} | {sl:g} | {fl:g} | {fmt(whole)} | {fmt(quiet)} | {fmt(loud)} | {'yes' if a else 'no'} | "
                      f"{'yes' if b else 'no'} |")
                if a and b:
                    ok[(passes, sl, fl)] = max(whole)
    print()
    if ok:
        best = min(ok, key=ok.get)
        print(f"lowest worst-seed whole-image error among the {len(ok)} points that meet (a) and (b): "
              f"passes {best[0]}, sigma_luminance {best[1]:g}, luminance_floor {best[2]:g}: {ok[best]:.3e}")
    else:
        print("no grid point meets (a) and (b) on all seeds")


def monkey():
    from oracle import oracle as O
    from tests import test_accumulate_cpu as TA
    e, r, _ = O.MODEL_MAT
    before, after, nhit, out = TA.monkey_orbit(72, 40, 8, 0.02, (e, r, 0.0))
    # the last frame's camera, guides and 256-spp render, as monkey_orbit made them
    from atray_amd import engine as E
    from atray_amd.assets import CENTERS, asset_path
    s = O.Scene(asset_path("Monkey"), center=CENTERS["Monkey"], materials=(O.SKY, (e, r, 0.0)))
    m = E.Mesh.load_obj(asset_path("Monkey"))
    m.translate_to(m.aabb(), CENTERS["Monkey"])
    arr = m.arrays()
    V, FV = arr[0], arr[3]
    v0, v1, v2 = (V[FV[:, k]] for k in range(3))
    fn = np.cross(v0 - v1, v0 - v2).astype(np.float32)
    fn = fn / np.sqrt((fn * fn).sum(1, keepdims=True)).astype(np.float32)
    eye, facing = TA.orbit(7, 0.02)
    _, (n, p, i), hit = TA.monkey_guides(s, fn, 72, 40, eye, facing)
    clean = s.render(O.Camera(72, 40, spp=256, bounces=3, eye=eye, facing=facing), 0x853C49E6748FEA9B)[0]
    err = lambda a: float(((a[hit].astype(np.float64) - clean[hit]) ** 2).mean())  # noqa: E731
    print(f"{nhit} hit pixels; lengths {np.bincount(out['length'].ravel())}")
    print(f"1-spp frame {before:.3e}; accumulated {after:.3e} ({err(out['color']):.3e})")
    got = VR.denoise_variance(out["color"], out["variance"], n, p, i, out["moments"], out["length"])[0]
    print(f"atr_denoise_variance, defaults: {err(got):.3e}")
    got = VR.denoise_variance(out["color"], out["variance"], n, p, i, out["moments"], out["length"], spatial_below=0)[0]
    print(f"atr_denoise_variance, defaults, no spatial estimate: {err(got):.3e}")
    for sc in (0.01, 0.05, 0.2):
        print(f"atr_denoise, defaults but sigma_color {sc}: {err(DR.denoise(out['color'], n, p, i, sigma_color=sc)[0]):.3e}")


if __name__ == "__main__":
    monkey() if "--monkey" in sys.argv[1:] else grid()
