#!/usr/bin/env python3
"""Forced alignment with wildcards (wildcard_penalty= of conformer_amd.align) beside the entries it extends, at the shapes of
tools/ctc_align_bench.py (B = 32, T = 249, L = 60 and B = 1, T = 16384, L = 2048: ctc_forced_align) and at the one-hour shape of
tools/ctc_align_long_bench.py ((T, L) = (90000, 30000), default tiling: ctc_forced_align_long).  V = 370.  Per shape:

    parent      the existing entry (wildcard_penalty=None)
    wild_free   the wildcard entry on the same wildcard-free target: the frame pass for w, one uniform load and one select
                per state and step more; every output equals the parent's
    wild        the wildcard entry with a wildcard every 20 tokens and at both ends
    cat         what the entry replaces: torch.cat of the column max - penalty, wildcards rewritten to the id V, then the
                parent entry on (B, T, V + 1) (its scores are NOT the feature's: every log_softmax is shifted); `cat_extra_mb`
                is the copy of the logits it allocates

Device time per call from HIP events after a warm-up, as those tools time; each figure is the median of `--repeats` such
timings and `spread` their max - min.  `wild_free_within_2_spreads`: |wild_free - parent| <= 2 * the parent's spread, the
expectation DESIGN.md "Forced alignment with wildcards" records.  Writes profiles/ctc_align_wild_bench.json and prints it as
one JSON line.

    python tools/ctc_align_wild_bench.py [--iters 10] [--repeats 7]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conformer_amd.align import WILDCARD, ctc_forced_align, ctc_forced_align_long  # noqa: E402

V = 370
PENALTY = 0.5
EVERY = 20
SHAPES = {"headline": (32, 249, 60, False), "long_form": (1, 16384, 2048, False), "hour_dense": (1, 90000, 30000, True)}


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
    return e0.elapsed_time(e1) / iters


def repeated(fn, iters, repeats):
    ts = [time_ms(fn, iters) for _ in range(repeats)]
    return {"ms": round(statistics.median(ts), 4), "spread": round(max(ts) - min(ts), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_align_wild_bench: no HIP device (the alignment only runs on the GPU; there is nothing to time here)")
    dev = torch.device("cuda:0")
    out = {"iters": args.iters, "repeats": args.repeats, "V": V, "penalty": PENALTY, "wildcard_every": EVERY, "shapes": {}}
    for name, (B, T, L, long) in SHAPES.items():
        g = torch.Generator().manual_seed(0)
        x = (torch.randn(B, T, V, generator=g) * 2).to(dev)
        y = torch.randint(1, V, (B, L), generator=g)
        yw = y.clone()
        yw[:, ::EVERY] = WILDCARD
        yw[:, -1] = WILDCARD
        y, yw = y.to(dev), yw.to(dev)
        yc = torch.where(yw == WILDCARD, torch.full_like(yw, V), yw)
        fn = ctc_forced_align_long if long else ctc_forced_align
        iters = max(args.iters // 2, 2) if long else args.iters

        def cat():
            xc = torch.cat([x, (x.max(dim=-1, keepdim=True).values - PENALTY)], dim=-1)
            return fn(xc, yc, 0)

        free, wild, via_cat = fn(x, y, 0, wildcard_penalty=PENALTY), fn(x, yw, 0, wildcard_penalty=PENALTY), cat()
        assert all(torch.equal(a, b) for a, b in zip(free, fn(x, y, 0)))
        assert bool(wild.ok.all()) and bool((wild.frame_tokens == WILDCARD).any())
        same_path = torch.equal(wild.frame_index, via_cat.frame_index)
        res = {"B": B, "T": T, "L": L, "entry": fn.__name__, "wildcards": int((yw[0] == WILDCARD).sum()),
               "wild_path_equals_cat_path": bool(same_path),
               "parent": repeated(lambda: fn(x, y, 0), iters, args.repeats),
               "wild_free": repeated(lambda: fn(x, y, 0, wildcard_penalty=PENALTY), iters, args.repeats),
               "wild": repeated(lambda: fn(x, yw, 0, wildcard_penalty=PENALTY), iters, args.repeats),
               "cat": repeated(cat, iters, args.repeats),
               "cat_extra_mb": round(B * T * (V + 1) * 4 / 2 ** 20, 1)}
        res["wild_free_over_parent"] = round(res["wild_free"]["ms"] / res["parent"]["ms"], 4)
        res["wild_over_parent"] = round(res["wild"]["ms"] / res["parent"]["ms"], 4)
        res["cat_over_wild"] = round(res["cat"]["ms"] / res["wild"]["ms"], 4)
        res["wild_free_within_2_spreads"] = abs(res["wild_free"]["ms"] - res["parent"]["ms"]) <= 2 * res["parent"]["spread"]
        out["shapes"][name] = res
        del x, y, yw, yc, free, wild, via_cat
        torch.cuda.empty_cache()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "ctc_align_wild_bench.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
