#!/usr/bin/env python3
"""The stem's fp32 conv2, direct implicit GEMM (cfm_subsample_conv2_relu_f32) against polyphase Winograd F(2x2,2x2)
(cfm_subsample_conv2_wino_relu_f32: pattern GEMMs + combine), timed with HIP events in interleaved rounds in one process at
B = 32 and 64 (T = 1000 frames: T1 = 499, F1 = 39, C = 512).  Prints medians and ranges, and the rel-L2 of both against a
float64 conv2d on two utterances."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd import _lib, ops  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--calls", type=int, default=4)
ap.add_argument("--batch", type=int, nargs="+", default=[32, 64])
args = ap.parse_args()

lib = _lib.load()
dev = torch.device("cuda:0")
T1, F1, C = 499, 39, 512
T2, F2 = (T1 - 1) // 2, (F1 - 1) // 2
st = torch.cuda.current_stream().cuda_stream
for B in args.batch:
    g = torch.Generator(device=dev).manual_seed(B)
    h1 = torch.randn(B, T1, F1, C, device=dev, generator=g).relu_()
    w2 = torch.randn(C, C, 3, 3, device=dev, generator=g) / (9 * C) ** 0.5
    b2 = torch.randn(C, device=dev, generator=g) * 0.1
    w2p, wwp = ops.pack_conv2_weight(w2), ops.pack_conv2_wino_weight(w2)
    planes = torch.empty(int(lib.cfm_conv2_wino_plane_elems(B, F1, T1, C)), device=dev)
    outs = {k: torch.empty(B, T2, F2, C, device=dev) for k in ("direct", "winograd")}

    def run(k):
        if k == "direct":
            _lib.check(lib.cfm_subsample_conv2_relu_f32(h1.data_ptr(), w2p.data_ptr(), b2.data_ptr(), outs[k].data_ptr(), B, F1,
                                                        T1, C, st), "direct")
        else:
            _lib.check(lib.cfm_subsample_conv2_wino_relu_f32(h1.data_ptr(), wwp.data_ptr(), b2.data_ptr(), planes.data_ptr(),
                                                             outs[k].data_ptr(), B, F1, T1, C, st), "winograd")

    for k in outs:
        run(k); run(k)
    torch.cuda.synchronize()
    times = {k: [] for k in outs}
    for _ in range(args.rounds):
        for k in outs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.calls):
                run(k)
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1) / args.calls)
    x = h1[:2].double().cpu().permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(x, w2.double().cpu().transpose(2, 3), b2.double().cpu(), stride=2).permute(0, 2, 3, 1).relu()
    fl = 2.0 * B * T2 * F2 * C * 9 * C
    base = statistics.median(times["direct"])
    print(f"B={B}: {B * T2 * F2} outputs x {C} channels, {args.rounds} interleaved rounds of {args.calls} calls")
    for k, t in times.items():
        med = statistics.median(t)
        err = float((outs[k][:2].double().cpu() - ref).norm() / ref.norm())
        print(f"  {k:9s} median {med:.3f} ms  [{min(t):.3f}, {max(t):.3f}]  {fl / med / 1e9:6.1f} direct-equivalent TFLOP/s"
              f"  {base / med:.3f}x  rel-L2 vs float64 {err:.2e}")
