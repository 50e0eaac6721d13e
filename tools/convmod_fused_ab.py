#!/usr/bin/env python3
"""The middle of ConvolutionModule (fp32 inference, LayerNorm folded): (a) the GLU GEMM (cfm_gemm_lnfold_f32, epi 3) and the
depthwise kernel (cfm_dwconv_bn_swish_fwd_f32) back to back against (b) the one fused kernel (cfm_convmod_glu_dwconv_f32), timed
with HIP events in interleaved rounds in one process.  Also timed, to attribute the time: the GLU GEMM alone and the fused kernel
without its depthwise stage (cfm_debug_convmod_variant(1): wrong results, the same GEMM).  Asserts that (a) and (b) are
bit-identical; prints median and range per side in microseconds per call, and whether every fused round is below every
two-kernel round.  Default shapes: the sweep behind ops.convmod_fused_ok's row-efficiency threshold (B = 32, C = 512, K = 31)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd import _lib, ops  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--channels", type=int, default=512)
ap.add_argument("--taps", type=int, default=31)
ap.add_argument("--frames", type=int, nargs="+", default=[128, 160, 192, 224, 249, 256, 300, 467, 499])
args = ap.parse_args()

lib = _lib.load()
dev = torch.device("cuda:0")
B, C, K = args.batch, args.channels, args.taps
print(f"B={B} C={C} K={K}: {args.rounds} interleaved rounds of {args.calls} calls, microseconds per call")
print(f"{'T':>5} {'chunks':>6} {'row eff':>7} | {'GLU GEMM':>9} {'fused-dw':>9} | {'two kernels (a)':>24} | {'fused (b)':>24} | "
      f"{'a/b':>6} every round")
for T in args.frames:
    g = torch.Generator(device=dev).manual_seed(T)
    r = lambda *s, scale=1.0: torch.randn(*s, device=dev, generator=g) * scale
    x, stats = ops.linear_residual(r(B * T, C), r(C, C, scale=C ** -0.5), r(C, scale=0.1), r(B * T, C) + 3.0, 1.0, emit_stats=True)
    x = x.view(B, T, C)
    fold = ops.fold_layernorm(r(2 * C, C, 1, scale=C ** -0.5), r(2 * C, scale=0.1), 1 + r(C, scale=0.3), r(C, scale=0.2))
    dw = (r(C, 1, K, scale=0.2), r(C, scale=0.1), 1 + r(C, scale=0.2), r(C, scale=0.1), r(C, scale=0.2), r(C).abs() + 0.5)
    out = {}

    def run(k):
        if k in ("two", "gemm"):
            gl = ops.linear_lnfold(x, stats, *fold, 1e-5, glu=True)
            out[k] = ops.dwconv_bn_swish(gl, *dw, 1e-5) if k == "two" else gl
        else:
            out[k] = ops.convmod_glu_dwconv(x, stats, *fold, 1e-5, *dw, 1e-5)

    sides = ("two", "fused", "gemm", "fused-dw")
    times = {k: [] for k in sides}
    for k in sides:
        lib.cfm_debug_convmod_variant(1 if k == "fused-dw" else 0)
        run(k); run(k)
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for k in sides:
            lib.cfm_debug_convmod_variant(1 if k == "fused-dw" else 0)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                run(k)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(1e3 * e0.elapsed_time(e1) / args.calls)
    lib.cfm_debug_convmod_variant(0)
    run("two"); run("fused")
    torch.cuda.synchronize()
    assert torch.equal(out["two"], out["fused"]), f"T={T}: the fused kernel and the two kernels differ"
    chunks = ops.convmod_chunks(T, K)
    med = {k: statistics.median(t) for k, t in times.items()}
    span = lambda k: f"{med[k]:7.1f} [{min(times[k]):6.1f},{max(times[k]):6.1f}]"
    wins = max(times["fused"]) < min(times["two"])
    print(f"{T:5d} {chunks:6d} {T / (256 * chunks):7.3f} | {med['gemm']:9.1f} {med['fused-dw']:9.1f} | {span('two'):>24} | "
          f"{span('fused'):>24} | {med['two'] / med['fused']:6.3f} {'fused wins' if wins else 'no'}")
print("bit-identical at every shape")
