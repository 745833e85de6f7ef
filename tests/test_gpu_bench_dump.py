"""bench.py's plain run and --dump-outputs on the GPU: the driver's command (c3, 20 timed frames
after 5 warmup frames) prints the headline line and nothing that --full measures, and the arrays
it dumps are the last timed frame (orbit position 24) as the oracle renders it
(tests/golden/fullframe.json). One bench process. Needs an MI355X (-m gpu)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.goldens import frame_digest, fullframe

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_the_last_timed_frame(tmp_path):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=110, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["unit"] == "Mrays/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == 20 and d["config"]["launches"] == [20] and d["config"]["rays_per_step"] == 1920 * 1080
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value is the timed frames' rays over their wall time, ms_per_step that wall time per frame
    assert d["value"] == pytest.approx(1920 * 1080 / d["ms_per_step"] / 1e3, rel=1e-3)
    for k in ("roofline", "cpu_baseline", "speedup_vs_cpu", "single_frame", "steady_state", "prep",
              "total_ray_casts_per_frame"):
        assert k not in d, k
    assert sorted(os.listdir(out)) == ["framebuffer.npy", "ray_casts.npy"]
    fb = np.load(out / "framebuffer.npy")
    casts = np.load(out / "ray_casts.npy")
    assert fb.dtype == np.float32 and fb.shape == (1080, 1920, 4)
    assert casts.dtype == np.float32 and casts.shape == (1080, 1920)
    assert d["dumped_outputs"] == {"framebuffer": [1080, 1920, 4], "ray_casts": [1080, 1920]}
    g = fullframe()["c3_orbit24"]
    assert frame_digest(fb.astype(np.uint8).view(np.uint32).reshape(1080, 1920)) == g["fb"]
    assert frame_digest(casts.astype(np.uint32)) == g["casts"]
