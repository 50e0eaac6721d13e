#!/usr/bin/env python3
"""Input sample rates (conformer_amd.resample.StreamingResampler): S slots, every slot fed the same chunk per step, mid-stream
(every slot carries a tail, no flush), beside the StreamingAudioFrontend step those samples feed.

Per (input rate, format), device events after warm-up, best of two alternated passes:
  resample_step_us   StreamingResampler.step whole (table copy + the one launch)
  resample_launch_us the launch of that step on its own, on the step's own buffers
  front_end_step_us  StreamingAudioFrontend.step at 16 kHz on the resampled chunk (what tools/stream_frontend_bench.py reports
                     as step_us)
  composed_step_us   StreamingAudioFrontend(input=...).step: both
  added_share        (composed_step_us - front_end_step_us) / front_end_step_us: what the resampler adds to the existing step"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd import _lib  # noqa: E402
from conformer_amd.frontend import ConformerAudioFrontend  # noqa: E402
from conformer_amd.resample import Resampler, StreamingResampler  # noqa: E402
from conformer_amd.stream_frontend import StreamingAudioFrontend  # noqa: E402
from tools.stream_frontend_bench import timed  # noqa: E402


def samples(S, n, fmt, dev):
    if fmt == "f32":
        return 0.3 * torch.randn(S, n, device=dev)
    return (6000 * torch.randn(S, n, 2, device=dev)).clamp(-32768, 32767).to(torch.int16)


def run(rate, fmt, S, seconds, iters, dev):
    base = ConformerAudioFrontend(device=dev)
    rs = Resampler(rate, base.sample_rate, device=dev)
    n = int(round(rate * seconds))
    n16 = int(round(base.sample_rate * seconds))
    x, x16, counts = samples(S, n, fmt, dev), 0.3 * torch.randn(S, n16, device=dev), [n] * S
    srs = StreamingResampler(rs, S, n)
    plain = StreamingAudioFrontend(base, S, n16)
    both = StreamingAudioFrontend(base, S, n, input=rs)
    for s in range(S):
        srs.open(s), plain.open(s), both.open(s)
    for _ in range(2):                                                    # from here on every slot is mid-stream
        y, out = srs.step(x, counts)
        plain.step(x16, [n16] * S)
        both.step(x, counts)
    C = 2 if fmt == "i16x2" else 1
    fns = {
        "resample_step": lambda: srs.step(x, counts),
        # the launch of the last step again (same table; the tail it reads is the next step's: the same amount of work)
        "resample_launch": lambda: rs.launch(x, C, n, (srs.tails[0], srs.tails[1]), srs.table, y),
        "front_end_step": lambda: plain.step(x16, [n16] * S),
        "composed_step": lambda: both.step(x, counts),
    }
    res = {"rate": rate, "format": fmt, "slots": S, "samples_per_step": n, "outputs_per_step": max(out), "taps": rs.K,
           "phases": rs.n}
    for _ in range(2):
        for name, fn in fns.items():
            us = timed(fn, iters)
            res[name + "_us"] = min(res.get(name + "_us", us), us)
    res["added_share"] = (res["composed_step_us"] - res["front_end_step_us"]) / res["front_end_step_us"]
    res["launch_GFLOPs"] = 2.0 * S * max(out) * rs.K / res["resample_launch_us"] * 1e-3
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=0.64, help="audio per slot and step")
    ap.add_argument("--rates", type=int, nargs="+", default=[8000, 44100, 48000])
    ap.add_argument("--formats", nargs="+", default=["f32", "i16x2"], choices=["f32", "i16x2"])
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    _lib.check(_lib.load().cfm_device_check(), "cfm_device_check")
    torch.manual_seed(0)
    out = {"what": "resampler step by launch, beside the streaming audio front end's step it feeds", "runs": []}
    with torch.no_grad():
        for rate in args.rates:
            for fmt in args.formats:
                r = run(rate, fmt, args.slots, args.seconds, args.iters, dev)
                out["runs"].append(r)
                print(json.dumps(r), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
