#!/usr/bin/env python3
"""Runs bench.py in a fresh child process with the Winograd conv2 on or off (CONFORMER_AMD_CONV2_WINOGRAD) and prints its
JSON line prefixed with the setting: the A/B driver for the path's opt-out, without changing bench.py."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
on = sys.argv[1]
assert on in ("0", "1"), "usage: bench_conv2_winograd.py 0|1 [bench.py arguments]"
env = dict(os.environ, CONFORMER_AMD_CONV2_WINOGRAD=on)
r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *sys.argv[2:]], env=env, capture_output=True, text=True)
lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
print(f"winograd={on} exit={r.returncode} {lines[-1] if lines else r.stdout[-2000:] + r.stderr[-2000:]}")
sys.exit(r.returncode)
