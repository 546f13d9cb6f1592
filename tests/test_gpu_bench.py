"""bench.py's plain run on one GPU: one JSON line with the headline fields and nothing of what --full adds, and --dump-outputs
writing what the last timed step computed (float32 / float64 .npy, below 64 MB)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_and_dump_outputs(hip, tmp_path):
    d = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--tile", "128",
           "--dump-outputs", str(d)]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert p.returncode == 0, (p.stdout[-500:], p.stderr[-1500:])
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, lines
    rec = json.loads(lines[0])
    assert rec["unit"] == "tiles/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32" and rec["steps"] == 3
    assert rec["value"] > 0 and rec["ms_per_step"] > 0
    assert abs(rec["value"] - 2 * 1e3 / rec["ms_per_step"]) < 0.01 * rec["value"]          # tiles/s and ms per step: the same timed steps
    assert rec["roofline"] is None and not {"extra", "cpu_baseline", "roofline_streaming", "roofline_lowest", "per_rank"} & set(rec)
    got = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert set(got) == {"loss_sum", "logits", "parameters", "running_stats"}
    assert got["loss_sum"].dtype == np.float64 and got["loss_sum"].shape == (1,)
    assert got["logits"].dtype == np.float32 and got["logits"].shape == (2, 1, 128, 128)
    assert got["parameters"].dtype == np.float32 and got["parameters"].shape == (6_629_233,)
    assert got["running_stats"].dtype == np.float32 and got["running_stats"].size > 0
    assert all(np.isfinite(a).all() for a in got.values())
    assert sum(os.path.getsize(d / f) for f in os.listdir(d)) < 64e6
    assert abs(float(got["loss_sum"][0]) / (2 * 128 * 128) - rec["config"]["final_loss"]) < 1e-6 * max(1.0, abs(rec["config"]["final_loss"]))
