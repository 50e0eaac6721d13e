#!/usr/bin/env python3
"""The stem's fp32 implicit-GEMM conv2 (cfm_subsample_conv2_relu_f32) on each tile it can run on, timed with HIP events in
interleaved rounds in one process, at B = 32 and 64 (T = 1000 frames: T1 = 499, F1 = 39, C = 512).  Every tile's h2 is checked
bitwise against the 128x128 tile's.  Tiles are selected with cfm_debug_set_conv2_bk (see include/conformer_hip.h)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd import _lib, ops  # noqa: E402

TILES = {101: "128x128, 4 waves (gemm_f32_kernel)", 102: "256x256, 8 waves, all rows",
         100: "by shape: 256x256 on whole rounds + 128x128"}
ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=4)
ap.add_argument("--batch", type=int, nargs="+", default=[32, 64])
args = ap.parse_args()
ROUNDS, CALLS = args.rounds, args.calls

lib = _lib.load()
dev = torch.device("cuda:0")
T1, F1, C = 499, 39, 512
T2, F2 = (T1 - 1) // 2, (F1 - 1) // 2
st = torch.cuda.current_stream().cuda_stream
for B in args.batch:
    g = torch.Generator(device=dev).manual_seed(B)
    h1 = torch.randn(B, T1, F1, C, device=dev, generator=g).relu_()
    w2p = ops.pack_conv2_weight(torch.randn(C, C, 3, 3, device=dev, generator=g) / (9 * C) ** 0.5)
    b2 = torch.randn(C, device=dev, generator=g) * 0.1
    outs = {t: torch.empty(B, T2, F2, C, device=dev) for t in TILES}

    def run(t):
        _lib.check(lib.cfm_subsample_conv2_relu_f32(h1.data_ptr(), w2p.data_ptr(), b2.data_ptr(), outs[t].data_ptr(), B, F1,
                                                    T1, C, st), "conv2")

    for t in TILES:
        lib.cfm_debug_set_conv2_bk(t)
        run(t); run(t)
    torch.cuda.synchronize()
    same = {t: torch.equal(outs[t], outs[101]) for t in TILES}
    times = {t: [] for t in TILES}
    for _ in range(ROUNDS):
        for t in TILES:
            lib.cfm_debug_set_conv2_bk(t)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(CALLS):
                run(t)
            e1.record()
            torch.cuda.synchronize()
            times[t].append(e0.elapsed_time(e1) / CALLS)
    lib.cfm_debug_set_conv2_bk(100)
    fl = 2.0 * B * T2 * F2 * C * 9 * C
    base = statistics.median(times[101])
    print(f"B={B}: M={B * T2 * F2} N={C} K={9 * C}, {ROUNDS} interleaved rounds of {CALLS} calls")
    for t, name in TILES.items():
        med = statistics.median(times[t])
        print(f"  {name:42s} median {med:.3f} ms  [{min(times[t]):.3f}, {max(times[t]):.3f}]  {fl / med / 1e9:6.1f} TFLOP/s"
              f"  {base / med:.3f}x  bitwise equal to 128x128: {same[t]}")
