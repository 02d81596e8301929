"""The plain benchmark command (`python bench.py --gpus 1 --steps K --warmup W`): the headline alone -- none of the `--full` objects --, exactly K
timed steps in `ms_per_step`, and with `--dump-outputs DIR` the final x of the last timed step's batch as DIR/x_final.npy."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_plain_line_times_the_headline_alone_and_dumps_its_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--batch", "64", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path / "out")], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 2 and line["warmup"] == 1 and line["dtype"] == "bf16" and line["unit"] == "images/s" and line["higher_is_better"] is True
    assert line["value"] > 0 and abs(line["value"] - 2 * 64 / (2 * line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3
    for k in ("single_stream", "pipeline", "roofline", "cpu_baseline", "accuracy", "sd3", "sd3_fp8", "fid50k", "validate"):
        assert k not in line, k
    x = np.load(tmp_path / "out" / "x_final.npy")
    assert x.dtype == np.float32 and x.shape == (64, 3, 32, 32) and np.isfinite(x).all() and np.abs(x).max() > 0
