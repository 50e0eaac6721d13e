#!/usr/bin/env python3
"""Beam-search timestamps (beam_ctc_stream_init(times=True), INTEGRATION.md "Beam-search timestamps"): what they cost and where
they point.

  cost    S = 8 and 32 streams of --steps chunks of 160 logit frames (V = 30) through beam_ctc_stream_step in commit mode (W = 100,
          K = 16, max_pending = 64: cfg-5's search), device events around each step + commit.  The same chunks with times on and
          with times off, alternating, --repeats times each on the same build; times off runs the entries that do not know of
          timestamps.  Random logits (the search's upper end) and peaky ones (runs of 2 frames of one dominant token).
  offset  on the peaky logits, one-shot: frame[i] of the best hypothesis (the token's ENTRY into the surviving lineage) minus
          token_start[i] of ctc_forced_align of the same hypothesis (its Viterbi start), mean / min / max over the tokens.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd.align import ctc_forced_align  # noqa: E402
from conformer_amd.decode import beam_ctc_decode, beam_ctc_stream_init, beam_ctc_stream_step  # noqa: E402


def stats(xs):
    s = sorted(xs)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "n": len(s)}


def chunks(kind, S, k, V, steps, dev):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(steps, S, k, V, generator=g)
    if kind == "random":
        return (2.0 * x).to(dev)
    path = torch.randint(0, V, (steps, S, k // 2), generator=g).repeat_interleave(2, dim=2)     # runs of 2 frames
    return (x + 8.0 * torch.nn.functional.one_hot(path, V)).to(dev)


def run(x, W, K, M, times, warm):
    """ms per chunk (step + commit) after `warm` chunks, and the tokens committed"""
    steps, S, k, V = x.shape
    st = beam_ctc_stream_init(S, None, x.device, beam_width=W, max_candidates=K, max_pending=M, max_chunk_frames=k, times=times)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for i in range(steps):
        ev[i][0].record()
        beam_ctc_stream_step(st, x[i], 0)
        ev[i][1].record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev[warm:]], int(st.total.sum())


def cost(args, dev):
    out = {}
    for kind in ("random", "peaky"):
        for S in args.slots:
            x = chunks(kind, S, args.chunk, args.vocab, args.steps, dev)
            run(x, args.beam, args.cands, args.max_pending, True, 0)            # both paths' code objects loaded
            run(x, args.beam, args.cands, args.max_pending, False, 0)
            on, off = [], []
            for _ in range(args.repeats):                                       # alternating, on the same inputs
                a, ta = run(x, args.beam, args.cands, args.max_pending, True, args.warmup)
                b, tb = run(x, args.beam, args.cands, args.max_pending, False, args.warmup)
                assert ta == tb, "times on / off committed different tokens"
                on += a
                off += b
            so, sf = stats(on), stats(off)
            out[f"{kind}_S{S}"] = {"times_on_ms": so, "times_off_ms": sf, "median_ratio": so["median"] / sf["median"],
                                   "committed_tokens": ta}
    return out


def offset(args, dev):
    B, T, V = 8, 160, args.vocab
    x = chunks("peaky", B, T, V, 1, dev)[0]
    tokens, counts, _, _, (frames, _) = beam_ctc_decode(x, 0, beam_width=args.beam, max_candidates=args.cands, return_times=True)
    n = counts[:, 0].contiguous()
    al = ctc_forced_align(x, tokens[:, 0, :int(n.max())].clamp(min=0).contiguous(), 0, None, n)
    assert bool(al.ok.all())
    d = []
    for b in range(B):
        d += (frames[b, 0, :int(n[b])] - al.token_start[b, :int(n[b])]).tolist()
    return {"tokens": len(d), "mean": sum(d) / len(d), "min": min(d), "max": max(d), "zero_share": d.count(0) / len(d)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--slots", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--chunk", type=int, default=160)
    ap.add_argument("--vocab", type=int, default=30)
    ap.add_argument("--beam", type=int, default=100)
    ap.add_argument("--cands", type=int, default=16)
    ap.add_argument("--max-pending", type=int, default=64)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beam_times_bench.py needs the MI355X (there is no CPU path)")
    dev = torch.device("cuda:0")
    print(json.dumps({"tool": "beam_times_bench", "W": args.beam, "K": args.cands, "chunk": args.chunk, "V": args.vocab,
                      "max_pending": args.max_pending, "cost": cost(args, dev), "offset": offset(args, dev)}))


if __name__ == "__main__":
    main()
