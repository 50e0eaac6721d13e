#!/usr/bin/env python3
"""Confidence (conformer_amd.confidence, SlotTranscriber(confidence=...)): what the frame pass and a step cost.

Device events after warm-up; every figure is the median of --passes alternated passes with their lowest and highest beside it:
  frames_us    the cfm_confidence_frames_f32 call alone (the frame kernel and the one that advances `total`) on (B, T, V) logits,
               offline form, per method
  torch_us     the same measure and the argmax written with stock PyTorch operators on the device (log_softmax, exp, sum, max):
               the yard-stick
per V = the bench model's vocabulary and --vocab, and
  transcriber_ms              SlotTranscriber.step (Conformer-L, beam W=100, no LM, times=True), S slots mid-stream fed --chunk
                              mel frames,
  transcriber_confidence_ms   the same object built with confidence=ConfidenceConfig(),
each the mean of --steps back-to-back steps between two events (host work included: it is what a caller's loop sees), the two
arms alternated, and with_over_without the ratio of the medians.  Without confidence= nothing is launched or allocated."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd import _lib, ops  # noqa: E402
from conformer_amd.confidence import METHODS, ConfidenceConfig  # noqa: E402
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


def spread(values):
    return {"median": statistics.median(values), "min": min(values), "max": max(values)}


def torch_measure(x, method, alpha):
    """The yard-stick: (conf, ids) of x (B, T, V) with stock operators."""
    V = x.shape[-1]
    lp = torch.log_softmax(x, dim=-1)
    if method == "max_prob":
        c = (V * lp.max(dim=-1).values.exp() - 1.0) / (V - 1.0)
    elif method == "entropy":
        c = 1.0 + torch.where(lp == -math.inf, 0.0, lp.exp() * lp).sum(-1) / math.log(V)
    elif method == "tsallis":
        c = 1.0 - ((alpha * lp).exp().sum(-1) - 1.0) / (V ** (1.0 - alpha) - 1.0)
    else:
        c = 1.0 + (alpha * lp).exp().sum(-1).log() / ((alpha - 1.0) * math.log(V))
    return c.clamp(0.0, 1.0), x.argmax(dim=-1)


def frames(B, T, V, iters, passes, dev):
    x = torch.randn(B, T, V, device=dev)
    x[:, :, 0] += 4.0
    k = torch.full((B,), T, dtype=torch.int64, device=dev)
    conf = torch.empty(B, T, device=dev)
    ids = torch.empty(B, T, dtype=torch.int64, device=dev)
    total = torch.zeros(B, dtype=torch.int64, device=dev)
    stream = ops._stream()
    res = {"batch": B, "frames": T, "vocab": V, "logits_bytes": 4 * B * T * V, "methods": {}}
    for method, alpha in (("max_prob", 0.33), ("entropy", 0.33), ("tsallis", 0.33), ("renyi", 2.0)):
        def ours():                                                         # (total runs on: the ring position turns, no more)
            _lib.call("cfm_confidence_frames_f32", x.data_ptr(), T * V, V, k.data_ptr(), T, V, METHODS[method], alpha,
                      conf.data_ptr(), ids.data_ptr(), total.data_ptr(), T, B, stream)
        got = {"frames_us": [], "torch_us": []}
        for _ in range(passes):
            got["frames_us"].append(timed(ours, iters))
            got["torch_us"].append(timed(lambda: torch_measure(x, method, alpha), iters))
        total.zero_()
        ours()
        ref, ref_ids = torch_measure(x, method, alpha)                      # the two arms compute the same thing
        run = {name: spread(v) for name, v in got.items()}
        run["alpha"] = alpha
        run["max_abs_diff_vs_torch"] = float((conf - ref).abs().max())
        run["ids_equal_torch"] = bool(torch.equal(ids, ref_ids))
        run["torch_over_ours"] = run["torch_us"]["median"] / run["frames_us"]["median"]
        res["methods"][method] = run
    return res


def transcriber(m, dec, S, chunk, steps, passes, dev):
    from conformer_amd.slots import SlotTranscriber
    x = torch.randn(S, 80, chunk, device=dev)
    got = {"transcriber_ms": [], "transcriber_confidence_ms": []}
    for p in range(passes + 1):                                             # the first pass warms up (packs, tables)
        for name, cfg in (("transcriber_ms", None), ("transcriber_confidence_ms", ConfidenceConfig())):
            tr = SlotTranscriber(m, dec, S, chunk * (steps + 3), times=True, confidence=cfg)
            for s in range(S):
                tr.open(s)
            for _ in range(2):                                              # every slot mid-stream
                tr.step(x, [chunk] * S)
            ms = timed(lambda: tr.step(x, [chunk] * S), steps, warm=0) * 1e-3
            if p:
                got[name].append(ms)
            del tr
            torch.cuda.empty_cache()
    res = {name: spread(v) for name, v in got.items()}
    res["with_over_without"] = res["transcriber_confidence_ms"]["median"] / res["transcriber_ms"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=250)
    ap.add_argument("--vocab", type=int, nargs="+", default=[370, 5000], help="vocabulary sizes beside the bench model's")
    ap.add_argument("--slots", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--chunk", type=int, default=64, help="mel frames per slot and step")
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=10, help="transcriber steps per pass")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--no-transcriber", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("confidence_bench: no GPU; a timing taken elsewhere says nothing")
    dev = torch.device("cuda:0")
    _lib.check(_lib.load().cfm_device_check(), "cfm_device_check")
    torch.manual_seed(0)
    vocab = ["<pad>"] + [chr(ord("a") + i) for i in range(26)] + ["'", "|", "<unk>"]
    out = {"what": "confidence: the frame pass against stock PyTorch operators, and SlotTranscriber.step with and without "
                   "confidence=", "frames": [], "transcriber": []}
    with torch.no_grad():
        for V in [len(vocab)] + args.vocab:
            run = frames(args.batch, args.frames, V, args.iters, args.passes, dev)
            out["frames"].append(run)
            print(json.dumps(run), file=sys.stderr, flush=True)
        if not args.no_transcriber:
            from conformer_amd.decode import BeamCTCDecoder
            from model.conformer import Conformer
            m = Conformer(len(vocab), 80, 16, 512, 8, 31, 640, 1, 0.0).to(dev).eval()
            dec = BeamCTCDecoder(vocab, blank_id=0, skip_ids=(len(vocab) - 1,), beam_width=100)
            for S in args.slots:
                run = {"slots": S, "mel_frames_per_step": args.chunk, "frames_per_step": encoder_frames(args.chunk)}
                run.update(transcriber(m, dec, S, args.chunk, args.steps, args.passes, dev))
                out["transcriber"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
