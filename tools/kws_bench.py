#!/usr/bin/env python3
"""Keyword spotting (conformer_amd.kws): what the two launches cost.  Run once; no threshold is asserted.  Writes --out
(profiles/kws_bench.json) and prints the same JSON.

Device events after warm-up, best of the alternated passes; V = --vocab (370):
  rowmax      cfm3_kws_rowmax_f32 over one recording of --frames encoder frames (one hour at 40 ms), with the GB/s of the logits
              it reads, beside copy_us, a plain device copy of the same bytes (GB/s of the bytes read); rowmax_cold_us: five
              single launches, each after 512 MiB were written, so that the logits come from HBM and not from the Infinity Cache
  scan        cfm3_kws_scan_f32 over that recording for K = 10, 100 and 1000 keywords of 8 tokens: scan_us and ns_per_frame, the
              time of one frame step of one wave (the waves of all groups run side by side)
  streaming   --slots slots x --chunk frames per step with 100 keywords: rowmax_us, scan_us and step_us (StreamingKeywordSpotter.
              step whole), beside slot_step_us, SlotTranscriber.step (Conformer-L, beam W=100) without keywords on 4 x --chunk mel
              frames per slot
  beam        the device beam search (W=100) over the first --beam-frames frames of the same logits: what a user would run
              otherwise, as ns per frame
The logits are synthetic: Gaussian, the blank 8 nats above on three frames of four, a random token on the fourth."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conformer_amd import _lib, ops  # noqa: E402
from conformer_amd.kws import Keywords, StreamingKeywordSpotter  # noqa: E402


def timed(fn, iters, warm=2):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def best(fns, iters):
    res = {}
    for _ in range(2):
        for name, fn in fns.items():
            us = timed(fn, iters)
            res[name + "_us"] = min(res.get(name + "_us", us), us)
    return res


def synthetic(S, T, V, dev):
    x = torch.randn(S, T, V, device=dev)
    top = torch.randint(1, V, (S, T), device=dev) * (torch.arange(T, device=dev) % 4 == 3)
    return x.scatter_add_(2, top.unsqueeze(2), torch.full((S, T, 1), 8.0, device=dev))


def keywords(K, V, tokens=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    seen, out = set(), []
    while len(out) < K:
        ids = (torch.randperm(V - 1, generator=g)[:tokens] + 1).tolist()
        if tuple(ids) not in seen:
            seen.add(tuple(ids))
            out.append(ids)
    return Keywords(out, blank_id=0, vocab_size=V, threshold=1.0)


def calls(sp, x, k):
    S, T, V = x.shape
    stream = ops._stream()
    sp.step(x, k)
    return {
        "rowmax": lambda: _lib.call("cfm3_kws_rowmax_f32", x.data_ptr(), T * V, V, k.data_ptr(), T, V, sp.rowmax.data_ptr(), T, S,
                                    stream),
        "scan": lambda: _lib.call("cfm3_kws_scan_f32", x.data_ptr(), T * V, V, sp.rowmax.data_ptr(), T, k.data_ptr(), T, V,
                                  sp.lanes.data_ptr(), sp.thresholds.data_ptr(), sp.G, len(sp.keywords), sp.state.data_ptr(),
                                  sp.detections.data_ptr(), sp.max_detections, sp.counts.data_ptr(), S, stream),
        "step": lambda: sp.step(x, k),
    }


def offline(T, V, iters, dev):
    x = synthetic(1, T, V, dev)
    k = torch.full((1,), T, dtype=torch.int64, device=dev)
    res = {"frames": T, "vocab": V, "logit_bytes": 4 * T * V}
    sp = StreamingKeywordSpotter(1, keywords(10, V), max_detections=4096, device=dev)
    fns = calls(sp, x, k)
    y = torch.empty_like(x)
    res.update(best({"rowmax": fns["rowmax"], "copy": lambda: y.copy_(x)}, iters))
    res["rowmax_GBps"] = res["logit_bytes"] / res["rowmax_us"] * 1e-3
    res["copy_GBps"] = res["logit_bytes"] / res["copy_us"] * 1e-3
    flush = torch.empty(1 << 27, dtype=torch.float32, device=dev)
    cold = []
    for _ in range(5):
        flush.fill_(1.0)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fns["rowmax"]()
        e1.record()
        torch.cuda.synchronize()
        cold.append(e0.elapsed_time(e1) * 1e3)
    res["rowmax_cold_us"] = sorted(cold)
    res["rowmax_cold_GBps"] = res["logit_bytes"] / sorted(cold)[2] * 1e-3              # (the median)
    del flush, y
    res["scan"] = []
    for K in (10, 100, 1000):
        sp = StreamingKeywordSpotter(1, keywords(K, V), max_detections=4096, device=dev)
        us = best({"scan": calls(sp, x, k)["scan"]}, max(2, iters // 4))["scan_us"]
        res["scan"].append({"keywords": K, "groups": sp.G, "scan_us": us, "ns_per_frame": us * 1e3 / T})
    return res, x


def streaming(S, chunk, V, iters, dev):
    x = synthetic(S, chunk, V, dev)
    k = torch.full((S,), chunk, dtype=torch.int64, device=dev)
    sp = StreamingKeywordSpotter(S, keywords(100, V), max_detections=4096, max_chunk_frames=chunk, device=dev)
    res = {"slots": S, "frames_per_step": chunk, "keywords": 100, "groups": sp.G}
    res.update(best(calls(sp, x, k), iters))
    return res


def slot_step(S, chunk, iters, dev):
    from conformer_amd.decode import BeamCTCDecoder
    from conformer_amd.slots import SlotTranscriber
    from model.conformer import Conformer
    vocab = ["<pad>"] + [chr(ord("a") + i) for i in range(26)] + ["'", "|", "<unk>"]
    m = Conformer(len(vocab), 80, 16, 512, 8, 31, 640, 1, 0.0).to(dev).eval()
    dec = BeamCTCDecoder(vocab, blank_id=0, skip_ids=(len(vocab) - 1,), beam_width=100)
    mel = 4 * chunk
    x = torch.randn(S, 80, mel, device=dev)
    tr = SlotTranscriber(m, dec, S, mel * (2 * iters + 8))
    for s in range(S):
        tr.open(s)
    return min(timed(lambda: tr.step(x, [mel] * S), iters) for _ in range(2))


def beam(x, frames, dev):
    from conformer_amd.decode import BeamCTCDecoder
    V = x.shape[2]
    vocab = ["<pad>"] + [chr(0x100 + i) for i in range(1, V - 2)] + ["|", "<unk>"]
    dec = BeamCTCDecoder(vocab, blank_id=0, skip_ids=(V - 1,), beam_width=100)
    part = x[:, :frames].contiguous()
    us = min(timed(lambda: dec(part), 2, warm=1) for _ in range(2))
    return {"frames": frames, "beam_width": 100, "decode_us": us, "ns_per_frame": us * 1e3 / frames}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=90000, help="encoder frames of the offline recording (one hour at 40 ms)")
    ap.add_argument("--vocab", type=int, default=370)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=16, help="encoder frames per slot and streaming step")
    ap.add_argument("--beam-frames", type=int, default=1500)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kws_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    _lib.check(_lib.load().cfm_device_check(), "cfm_device_check")
    torch.manual_seed(0)
    out = {"what": "keyword spotting: the row-maximum and scan launches over one hour of logits and per streaming step, beside a "
                   "copy, a SlotTranscriber step and the beam search"}

    def case(name, fn):
        try:
            out[name] = fn()
        except Exception as e:                                             # (a case that cannot run is reported, not hidden)
            out[name] = {"error": f"{type(e).__name__}: {e}"}
        print(json.dumps({name: out[name]}), file=sys.stderr, flush=True)

    with torch.no_grad():
        out["offline"], x = offline(args.frames, args.vocab, args.iters, dev)
        print(json.dumps(out["offline"]), file=sys.stderr, flush=True)
        case("beam", lambda: beam(x, args.beam_frames, dev))
        del x
        case("streaming", lambda: streaming(args.slots, args.chunk, args.vocab, args.iters * 5, dev))
        case("slot_step_us", lambda: slot_step(args.slots, args.chunk, args.iters, dev))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
