"""bench.py's command line on one GPU at the smallest config (C1: 256^2, 1k
VRLs): a plain run times exactly --steps steps and prints one result line
without the --full legs, and --dump-outputs writes the frame of the last timed
step.  A pass's frame depends only on the scene, the VRLs, the seed and the
pass index (counter RNG streams; the gathers accumulate per pixel in a fixed
order and the refinement is bit-exact), so the dumped frame must equal, bit
for bit, the frame a fresh integrator renders for that pass."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 2, 1


def test_plain_run_line_and_dump(gpu_ok, tmp_path):
    import torch
    import alvrl
    import bench
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "C1",
                        "--steps", str(STEPS), "--warmup", str(WARMUP), "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["metric"] == bench.METRIC and d["unit"] == "VRL contributions/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["n_gpus"] == 1
    assert d["steps"] == STEPS and d["warmup"] == WARMUP
    # value = contributions of the timed steps / their wall time, and
    # ms_per_step = that wall time / steps: the two and the counted pairs agree
    pairs = d["breakdown"]["render_pairs"] + d["breakdown"]["prepass_pairs"]
    assert pairs > 0 and d["ms_per_step"] > 0
    assert d["value"] * d["ms_per_step"] * 1e-3 * STEPS == pytest.approx(pairs, rel=1e-9)
    # the legs that take runs of their own stay behind --full
    assert d["cpu_baseline"] is None
    for k in ("pixel_rmse_vs_cpu", "records_mode", "pixel_rmse_vs_cpu_unconditional", "alt_decomposition"):
        assert k not in d, k

    assert sorted(os.listdir(out)) == ["framebuffer.npy"]
    frame = np.load(out / "framebuffer.npy")
    cfg = bench.CONFIGS["C1"]
    W, H = cfg["w"], cfg["h"]
    assert frame.dtype == np.float32 and frame.shape == (H, W, 3)
    assert np.isfinite(frame).all() and frame.max() > 0

    scene = alvrl.scene_default(W, H)
    vrls, pc = alvrl.trace_vrls(scene, cfg["nvrl"], seed=bench.SEED_VRL)
    it = alvrl.Integrator(cfg["props"] + (";" if cfg["props"] else "") + f"seed={bench.SEED_RNG}", device=0)
    it.set_vrls(vrls, pc)
    it.preprocess(scene)
    it.prepass(WARMUP + STEPS - 1)
    fb = torch.zeros(W * H * 3, dtype=torch.float32, device="cuda")
    it.render(fb)
    torch.cuda.synchronize()
    mine = fb.view(H, W, 3).cpu().numpy()
    it.close()
    assert np.array_equal(mine.view(np.uint32), frame.view(np.uint32))
