"""bench.py --dump-outputs: (CPU) the writer's dtypes and exactness; (GPU) one short headline run that dumps the encoder output
of its last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_writes_float32_and_exact_float64_lengths(tmp_path):
    y = torch.randn(3, 5, 8)
    lens = torch.tensor([249, 7, 2 ** 40], dtype=torch.int64)
    bench.dump_outputs(str(tmp_path / "d"), {"encoder_out": y, "encoder_out_lengths": lens})
    a = np.load(tmp_path / "d" / "encoder_out.npy")
    b = np.load(tmp_path / "d" / "encoder_out_lengths.npy")
    assert a.dtype == np.float32 and a.shape == (3, 5, 8) and np.array_equal(a, y.numpy())
    assert b.dtype == np.float64 and b.tolist() == [249.0, 7.0, float(2 ** 40)]


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--no-cpu-baseline", "--no-secondary", "--no-roofline", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    j = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert j["steps"] == 2 and j["ms_per_step"] > 0
    y = np.load(out / "encoder_out.npy")
    n = np.load(out / "encoder_out_lengths.npy")
    assert y.dtype == np.float32 and y.shape == (32, 249, 512) and np.isfinite(y).all() and float(np.abs(y).max()) > 0
    assert n.dtype == np.float64 and n.tolist() == [249.0] * 32
    assert sum(os.path.getsize(out / f) for f in os.listdir(out)) <= 64 << 20
