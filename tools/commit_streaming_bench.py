#!/usr/bin/env python3
"""Committed-prefix streaming search (beam_ctc_stream_init(max_pending=...)): what the commit costs and what it saves.

  state   beam state bytes per slot at cfg-5 (W = 100, K = 16, 20000 mel frames = 4999 encoder frames, 160 per step) without
          max_pending (cfm_ctc_beam_stream_state_bytes) and with it (cfm_ctc_beam_commit_state_bytes)
  kernel  S streams of --steps chunks of 160 logit frames (V = 30) through beam_ctc_stream_step in commit mode; device events
          around each C entry give the step's own time (candidate rows + search) and the commit kernel's, per chunk.  Random
          logits (the search's upper end: every commit is forced and drops most of the beam) and peaky ones (runs of 1-3 frames
          of one dominant token: commits are natural).  The same chunks through a search without max_pending give the step
          time of the path that does not commit.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd import _lib  # noqa: E402
from conformer_amd.decode import beam_ctc_stream_init, beam_ctc_stream_step  # noqa: E402


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


def timed_run(x, W, K, M, warm):
    """step_us / commit_us per chunk (medians over the chunks after `warm`) from events around every C entry"""
    steps, S, k, V = x.shape
    dev = x.device
    st = beam_ctc_stream_init(S, None if M else steps * k, dev, beam_width=W, max_candidates=K,
                              max_pending=M, max_chunk_frames=k if M else None)
    spans, orig = [], _lib.call

    def call(name, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        orig(name, *a)
        e1.record()
        spans.append((name, e0, e1))

    _lib.call = call
    try:
        for i in range(steps):
            beam_ctc_stream_step(st, x[i], 0)
    finally:
        _lib.call = orig
    torch.cuda.synchronize()
    out = {}
    for name in ("cfm_ctc_beam_stream_step_f32", "cfm_ctc_beam_stream_commit"):
        us = [e0.elapsed_time(e1) * 1e3 for n, e0, e1 in spans if n == name][warm:]
        if us:
            out[name.replace("cfm_ctc_beam_stream_", "") + "_us"] = stats(us)
    if M:
        out["tokens_committed_per_stream"] = float(st.total.float().mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--beam", type=int, default=100)
    ap.add_argument("--max-pending", type=int, default=64)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warm", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lib = _lib.load()
    W, K, k, V, M = args.beam, 16, 160, 30, args.max_pending
    out = {"what": "committed-prefix streaming search: state size and the commit kernel's time", "beam_width": W,
           "max_candidates": K, "chunk_frames": k, "max_pending": M, "streams": args.streams,
           "state_bytes_per_slot": {"without_max_pending_4999_frames": int(lib.cfm_ctc_beam_stream_state_bytes(1, 4999, W, K, 0, 0)),
                                    "with_max_pending": int(lib.cfm_ctc_beam_commit_state_bytes(1, M, k, W, K, 0, 0))},
           "kernel": {}}
    dev = torch.device("cuda:0")
    for kind in ("random", "peaky"):
        x = chunks(kind, args.streams, k, V, args.steps, dev)
        res = {}
        for rep in range(2):                                   # alternate the two searches, keep both passes (the spread)
            res[f"commit_pass{rep}"] = timed_run(x, W, K, M, args.warm)
            res[f"plain_pass{rep}"] = timed_run(x, W, K, None, args.warm)
        out["kernel"][kind] = res
    text = json.dumps(out, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
