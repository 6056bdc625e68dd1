"""bench.py on one GPU in small: a plain run prints the headline line without the un-timed legs, and --dump-outputs writes what its last
timed step computed (the legs themselves, with --full: tests/test_gpu_dist.py for N = 2; the default workload: bench.py --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--size", "64", "--fb", "256", "--levels", "6", "--log2-hashmap-size", "14", "--hidden-layers", "2", "--train-steps", "120"]


@pytest.mark.gpu
def test_plain_bench_dumps_the_last_timed_frame(tmp_path):
    d = tmp_path / "out"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1"] + SMALL
                         + ["--dump-outputs", str(d)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-2500:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-1500:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["value"] > 0
    assert line["unit"] == "frames/s" and line["higher_is_better"] is True and line["dtype"] == "f16"
    assert abs(line["ms_per_step"] * line["value"] - 1e3) < 0.01 * 1e3     # both from the same timed region
    for key in ("cpu_baseline", "interactive"):                               # --full only
        assert key not in line, key
    assert line["psnr_db"] is None and line["image_vs_ground_truth"] is None and "alone" not in line["roofline"]
    assert sorted(os.listdir(d)) == ["frame.npy", "frame_stats.npy"]
    frame, stats = np.load(d / "frame.npy"), np.load(d / "frame_stats.npy")
    assert frame.shape == (256, 256, 4) and frame.dtype == np.float32 and np.isfinite(frame).all()
    assert frame[..., 3].min() >= 0.0 and frame[..., 3].max() <= 1.0 and (frame[..., 3] > 0).mean() > 0.1
    assert stats.dtype == np.float64 and stats.shape == (4,)
    assert stats[3] == line["rays_hit"] and stats[2] == line["iterations_per_frame"] and stats[0] > 0
