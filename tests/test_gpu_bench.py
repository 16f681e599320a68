"""bench.py's plain run (no --full): one JSON line with the headline fields only, --steps timed updates, and with
--dump-outputs the arrays the last timed update handed back, from inputs that are the same for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

OUTPUTS = {"params": np.float32, "loss_acc": np.float32, "gae_adv": np.float64, "gae_target": np.float64,
           "gae_old_value": np.float32}


def _plain_run(tmp_path, tag, steps, warmup):
    out = os.path.join(str(tmp_path), tag)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--dump-outputs", out, "--detail-file", os.path.join(str(tmp_path), tag + "_detail.json")]
    proc = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert proc.returncode == 0, proc.stderr.decode()[-3000:]
    lines = [l for l in proc.stdout.decode().splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), {k: np.load(os.path.join(out, k + ".npy")) for k in OUTPUTS}


def test_plain_bench_run_times_steps_and_dumps_the_last_update(tmp_path):
    line, a = _plain_run(tmp_path, "a", 2, 1)
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert line["unit"] == "env-frames/s" and "bf16" in line["dtype"]
    for k in ("roofline", "cpu_baseline", "e2e", "secondary", "sustained"):
        assert k not in line, k                    # measured only with --full
    for k, dt in OUTPUTS.items():
        assert a[k].dtype == dt and np.isfinite(a[k]).all(), k
    assert a["gae_adv"].shape == (4096,) and sum(v.nbytes for v in a.values()) < 64 << 20
    # the same three updates split differently between warm-up and timed steps: the same inputs, the same outputs
    _, c = _plain_run(tmp_path, "c", 1, 2)
    for k in ("gae_adv", "gae_target", "gae_old_value"):
        assert np.array_equal(a[k], c[k]), k
    scale = np.linalg.norm(a["params"])
    assert np.linalg.norm(a["params"] - c["params"]) < 1e-5 * scale
    # one more timed step is one more update
    _, d = _plain_run(tmp_path, "d", 3, 1)
    assert np.linalg.norm(a["params"] - d["params"]) > 1e-4 * scale
