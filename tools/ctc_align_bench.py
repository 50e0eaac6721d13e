#!/usr/bin/env python3
"""CTC forced alignment (conformer_amd.align.ctc_forced_align) at the model's decode shape: B = 32 utterances, T = 249 frames
(T = 1000 mel frames after the stem), V = 370 (the reference vocabulary), L = 60 labels, and at one long-form shape: B = 1,
T = 16384, L = 2048.  Beside the first it prints the forward of ConformerCriterion.ctc_loss on the same logits and targets:
the loss reads the same bytes and walks the same chain of T steps, so it is the yardstick (the loss stops at L = 1023, so
the long-form shape has none).  Device time per call from HIP events after a warm-up; one JSON line.  The share of each
kernel (chain, trace, frames, spans) comes from `rocprofv3 --kernel-trace --stats -- python tools/ctc_align_bench.py`.

    python tools/ctc_align_bench.py [--iters 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd.align import ctc_forced_align  # noqa: E402
from conformer_amd.evaluation import ConformerCriterion  # noqa: E402

SHAPES = {"headline": (32, 249, 370, 60), "long_form": (1, 16384, 370, 2048)}


def time_ms(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / iters, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_align_bench: no HIP device (the alignment only runs on the GPU; there is nothing to time here)")
    dev = torch.device("cuda:0")
    out = {"iters": args.iters, "shapes": {}}
    for name, (B, T, V, L) in SHAPES.items():
        g = torch.Generator().manual_seed(0)
        x = (torch.randn(B, T, V, generator=g) * 2).to(dev)
        y = torch.randint(1, V, (B, L), generator=g).to(dev)
        in_len = torch.full((B,), T, dtype=torch.int64, device=dev)
        tg_len = torch.full((B,), L, dtype=torch.int64, device=dev)
        res = {"B": B, "T": T, "V": V, "L": L}
        al = ctc_forced_align(x, y, 0, in_len, tg_len)
        assert bool(al.ok.all())
        res["align_ms"] = time_ms(lambda: ctc_forced_align(x, y, 0, in_len, tg_len), args.iters)
        res["align_us_per_frame"] = round(1e3 * res["align_ms"] / T, 4)
        if name == "headline":
            crit = ConformerCriterion(blank_id=0)
            with torch.no_grad():
                res["ctc_loss_fwd_ms"] = time_ms(lambda: crit.ctc_loss(x, y, in_len, tg_len), args.iters)
            res["align_over_loss_fwd"] = round(res["align_ms"] / res["ctc_loss_fwd_ms"], 3)
        out["shapes"][name] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
