"""bench.py: a plain run carries the headline only; --full adds the measurements that take runs of their own, and its
--no-* options still leave single ones out."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ("kernel_launches_per_forward", "roofline", "secondary", "cpu_baseline")


def _bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *argv],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-4000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_carries_the_headline_only():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    j = _bench("--steps", "2", "--warmup", "1")
    assert j["metric"] == "encoder audio-frames/sec (B=32,T=1000,d=512,L=16)" and j["unit"] == "audio-frames/sec"
    assert j["higher_is_better"] is True and j["dtype"] == "f32" and j["steps"] == 2 and j["warmup"] == 1
    assert j["ms_per_step"] > 0 and j["value"] == pytest.approx(32 * 1000 / (j["ms_per_step"] * 1e-3), rel=1e-9)
    assert not [k for k in EXTRAS if k in j]


@pytest.mark.gpu
def test_full_run_adds_the_extras():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    j = _bench("--steps", "1", "--warmup", "0", "--full", "--no-cpu-baseline")
    assert j["ms_per_step"] > 0 and j["kernel_launches_per_forward"] > 0
    rows = j["roofline"]["all_gemm_sites"]
    assert rows and all(r["avg_ms"] > 0 for r in rows) and 0 < j["roofline"]["frac"] < 1
    assert set(j["secondary"]) == {"note", "f32x6", "f32x3", "bf16_autocast"}
    assert all(j["secondary"][k]["ms_per_step"] > 0 for k in ("f32x6", "f32x3", "bf16_autocast"))
    assert "cpu_baseline" not in j
