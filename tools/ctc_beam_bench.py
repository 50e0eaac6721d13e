#!/usr/bin/env python3
"""CTC prefix beam search (conformer_amd.decode.beam_ctc_decode) at the model's decode shape: B = 32 utterances, T = 249
frames (T = 1000 mel frames after the stem), V = 370 (the reference vocabulary), for W in {1, 16, 100, 190, 256}, the other
knobs at their defaults (K = 16, token_min_logp = -5, beam_prune_logp = -10).  Device time per call from HIP events after a
warm-up; one JSON line.  Two kinds of logits: "random" (randn * 2: many candidates per frame, the beam always full) and
"peaky" (one id per frame 12 above the rest, as a trained model emits: few candidates survive pruning).

    python tools/ctc_beam_bench.py [--iters 20]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd.decode import beam_ctc_decode  # noqa: E402

B, T, V = 32, 249, 370
WIDTHS = (1, 16, 100, 190, 256)


def logits_for(kind: str, dev) -> torch.Tensor:
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, V, generator=g) * 2
    if kind == "peaky":
        ids = torch.randint(0, V, (B, T, 1), generator=g)
        ids[:, ::2] = 0                                              # every other frame blank
        x.scatter_(-1, ids, 12.0)
    return x.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_beam_bench: no HIP device (the decode only runs on the GPU; there is nothing to time here)")
    dev = torch.device("cuda:0")
    L = torch.full((B,), T, dtype=torch.int64, device=dev)
    out = {"B": B, "T": T, "V": V, "K": 16, "iters": args.iters, "ms": {}}
    for kind in ("random", "peaky"):
        x = logits_for(kind, dev)
        out["ms"][kind] = {}
        for W in WIDTHS:
            for _ in range(3):
                beam_ctc_decode(x, 0, L, beam_width=W)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.iters):
                beam_ctc_decode(x, 0, L, beam_width=W)
            e1.record()
            torch.cuda.synchronize()
            out["ms"][kind][str(W)] = round(e0.elapsed_time(e1) / args.iters, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
