#!/usr/bin/env python3
"""Endpointing (conformer_amd.endpoint.StreamingEndpointer, SlotTranscriber(endpoint=...)): what one step costs.

Device events after warm-up, best of the alternated passes:
  launch_us   the cfm_endpoint_step_f32 launch alone on (S, k, V) logits, every slot taking all k rows
  step_us     StreamingEndpointer.step whole (argument checks and the call), on the same logits
per (k, V): k = the encoder frames of a --chunk mel-frame step, V = the bench model's vocabulary and --vocab, and
  transcriber_ms            SlotTranscriber.step (Conformer-L, beam W=100, no LM), S slots mid-stream fed --chunk mel frames,
  transcriber_endpoint_ms   the same object built with endpoint=EndpointConfig(),
each the mean of --steps back-to-back steps between two events (host work included: it is what a caller's loop sees), the two
arms alternated, and with_over_without their ratio.  Without endpoint= a step is the code of the commit before endpointing:
nothing is launched or allocated for it."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd import _lib, ops  # noqa: E402
from conformer_amd.endpoint import EndpointConfig, StreamingEndpointer  # noqa: E402
from conformer_amd.streaming import encoder_frames  # noqa: E402


def timed(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def endpointer(S, k, V, iters, dev):
    ep = StreamingEndpointer(S, 0, EndpointConfig(), 0.04, dev)
    x = torch.randn(S, k, V, device=dev)
    x[:, :, 0] += 4.0                                                       # the blank wins about half the frames
    kd = torch.full((S,), k, dtype=torch.int64, device=dev)
    stream = ops._stream()
    fns = {
        "launch": lambda: _lib.call("cfm_endpoint_step_f32", x.data_ptr(), k * V, V, kd.data_ptr(), k, V, ep.ids_dev.data_ptr(), 1,
                                    ep.log_threshold, ep.rules.data_ptr(), len(ep.rule_rows), ep.state.data_ptr(), S, stream),
        "step": lambda: ep.step(x, kd),
    }
    res = {"slots": S, "frames_per_step": k, "vocab": V, "logits_bytes": 4 * S * k * V}
    for _ in range(2):
        for name, fn in fns.items():
            us = timed(fn, iters)
            res[name + "_us"] = min(res.get(name + "_us", us), us)
    return res


def transcriber(m, dec, S, chunk, steps, passes, dev):
    from conformer_amd.slots import SlotTranscriber
    x = torch.randn(S, 80, chunk, device=dev)
    best = {}
    for p in range(passes + 1):                                             # the first pass warms up (packs, tables)
        for name, cfg in (("transcriber_ms", None), ("transcriber_endpoint_ms", EndpointConfig())):
            tr = SlotTranscriber(m, dec, S, chunk * (steps + 3), endpoint=cfg)
            for s in range(S):
                tr.open(s)
            for _ in range(2):                                              # every slot mid-stream
                tr.step(x, [chunk] * S)
            ms = timed(lambda: tr.step(x, [chunk] * S), steps, warm=0) * 1e-3
            if p:
                best[name] = min(best.get(name, ms), ms)
            del tr
            torch.cuda.empty_cache()
    best["with_over_without"] = best["transcriber_endpoint_ms"] / best["transcriber_ms"]
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--chunk", type=int, nargs="+", default=[64, 640], help="mel frames per slot and step")
    ap.add_argument("--vocab", type=int, nargs="+", default=[370, 5000], help="vocabulary sizes beside the bench model's")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--steps", type=int, default=10, help="transcriber steps per pass")
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--no-transcriber", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    _lib.check(_lib.load().cfm_device_check(), "cfm_device_check")
    torch.manual_seed(0)
    vocab = ["<pad>"] + [chr(ord("a") + i) for i in range(26)] + ["'", "|", "<unk>"]
    out = {"what": "endpointing: the launch, StreamingEndpointer.step and SlotTranscriber.step with and without endpoint=",
           "endpointer": [], "transcriber": []}
    with torch.no_grad():
        for chunk in args.chunk:
            for V in [len(vocab)] + args.vocab:
                run = endpointer(args.slots, encoder_frames(chunk), V, args.iters, dev)
                out["endpointer"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
        if not args.no_transcriber:
            from conformer_amd.decode import BeamCTCDecoder
            from model.conformer import Conformer
            m = Conformer(len(vocab), 80, 16, 512, 8, 31, 640, 1, 0.0).to(dev).eval()
            dec = BeamCTCDecoder(vocab, blank_id=0, skip_ids=(len(vocab) - 1,), beam_width=100)
            for chunk in args.chunk:
                run = {"slots": args.slots, "mel_frames_per_step": chunk, "frames_per_step": encoder_frames(chunk)}
                run.update(transcriber(m, dec, args.slots, chunk, args.steps, args.passes, dev))
                out["transcriber"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
