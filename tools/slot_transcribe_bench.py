#!/usr/bin/env python3
"""Independent streams (conformer_amd.slots.SlotTranscriber): Conformer-L width, S slots fed 640-frame chunks, resumable CTC
beam search at W=100 with and without a synthetic word n-gram LM.

  staggered  seeded utterance lengths, slots opened at staggered steps and reopened with a new utterance as soon as theirs
             ends, so the slots sit at different positions: per-step latency (median, max; closes included) and aggregate
             audio-seconds per second (10 ms per mel frame)
  lockstep   every slot opened together and given the same frames: StreamingTranscriber (eager) and SlotTranscriber at the
             same S and chunk, per-step latency side by side
  attention  relpos_attention_slots against relpos_attention_rows with identical offsets in every slot (the new rows of a
             640-frame chunk against caches of growing length), device events after warm-up; with --dtype bf16 / fp16 both run
             under that autocast: the 16-bit slots kernel on the fp32 and on the 16-bit cache, with the key split of
             ops._key_split and with keys_hint=1 (no split), against the 16-bit rows kernel (which has no split)

--dtype bf16 | fp16: the slot objects are built with dtype= (16-bit K/V caches, every step under their own autocast) and the
lockstep StreamingTranscriber steps under torch.autocast of that type.
--left-context L: bounded history (ring K/V caches sized for --chunk); --max-pending M (with it; L defaults to 256): the search
commits after every step and its buffers no longer scale with --max-mel (fp32 only).  Random weights, so the logits are not peaky: the beam search runs at its random-logit cost (the upper end)."""
import argparse
import contextlib
import json
import os
import random
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd import ops  # noqa: E402
from conformer_amd.decode import BeamCTCDecoder  # noqa: E402
from conformer_amd.lm import write_synthetic_arpa  # noqa: E402
from conformer_amd.slots import SlotTranscriber  # noqa: E402
from conformer_amd.transcribe import StreamingTranscriber  # noqa: E402
from model.conformer import Conformer  # noqa: E402


def stats(xs):
    s = sorted(xs)
    return {"median": s[len(s) // 2], "max": s[-1], "n": len(s)}


def staggered(tr, S, chunk, steps, max_mel, seed, dev):
    """Open slot s at step s % 4 (staggered), feed every open slot `chunk` frames per step (its remainder at the end), close it
    when its utterance is done and open it again with a new one in the next step."""
    rng = random.Random(seed)
    x = torch.randn(S, 80, chunk, device=dev)
    left = [0] * S
    open_at = [s % 4 for s in range(S)]
    lat, frames_total = [], 0
    torch.cuda.synchronize()
    t_all = time.perf_counter()
    for step in range(steps):
        t0 = time.perf_counter()
        for s in range(S):
            if tr.encoder.is_open[s] and left[s] == 0:
                tr.close(s)
            if not tr.encoder.is_open[s] and step >= open_at[s]:
                tr.open(s)
                left[s] = rng.randint(max_mel // 4, max_mel)
        frames = [min(chunk, left[s]) if tr.encoder.is_open[s] else 0 for s in range(S)]
        tr.step(x, frames)
        torch.cuda.synchronize()
        lat.append((time.perf_counter() - t0) * 1e3)
        for s in range(S):
            left[s] -= frames[s]
        frames_total += sum(frames)
    total = time.perf_counter() - t_all
    for s in range(S):
        if tr.encoder.is_open[s]:
            tr.close(s)
    return {"step_ms": stats(lat[1:]), "audio_s_per_s": frames_total * 0.010 / total, "steps": steps,
            "mel_frames": frames_total}


def _autocast(dt):
    return contextlib.nullcontext() if dt is None else torch.autocast("cuda", dtype=dt)


def lockstep(m, dec, S, chunk, steps, dev, dt=None, kw=None):
    kw = kw or {}
    x = torch.randn(S, 80, chunk, device=dev)
    out = {}

    def stream_step(tr):
        with _autocast(dt):
            return tr.step(x)

    for name in ("streaming", "slots"):
        best = None
        for _ in range(2):                                     # the first pass warms up (packs, tables)
            if name == "streaming":
                tr = StreamingTranscriber(m, dec, S, chunk * steps, **kw)
                run = lambda: stream_step(tr)                   # noqa: E731
            else:
                tr = SlotTranscriber(m, dec, S, chunk * steps, dtype=dt, **kw)
                for s in range(S):
                    tr.open(s)
                run = lambda: tr.step(x, [chunk] * S)           # noqa: E731
            lat = []
            torch.cuda.synchronize()
            for _ in range(steps):
                t0 = time.perf_counter()
                run()
                torch.cuda.synchronize()
                lat.append((time.perf_counter() - t0) * 1e3)
            del tr, run
            torch.cuda.empty_cache()
            if best is None or sorted(lat)[len(lat) // 2] < best["median"]:
                best = stats(lat)
        out[name] = best
    out["slots_over_streaming_median"] = out["slots"]["median"] / out["streaming"]["median"]
    return out


def attention_ab(S, dev, dt=None, iters=50):
    H, dh, t_max, k = 8, 64, 4999, 160                          # Conformer-L, T = 20000 mel frames, a 640-frame chunk
    d = H * dh
    qkv = torch.randn(S, t_max, 3 * d, device=dev)
    qkv16 = None if dt is None else qkv.to(dt)
    pos = torch.randn(2 * t_max - 1, d, device=dev) * 0.5
    u, v = torch.randn(d, device=dev) * 0.3, torch.randn(d, device=dev) * 0.3
    ctx = torch.empty(S, t_max, d, device=dev)
    rows = []
    for n0 in (640, 2400, t_max - k) if dt is None else (0, 640, 1440, 2400, t_max - k):
        L = torch.full((S,), n0 + k, device=dev, dtype=torch.int64)
        qb = torch.full((S,), n0, device=dev, dtype=torch.int64)
        qc = torch.full((S,), k, device=dev, dtype=torch.int64)
        cc = torch.empty(S, k, d, device=dev)
        slots = lambda cache, hint: ops.relpos_attention_slots(cache, pos, u, v, L, H, qb, qc, k, cc, keys_hint=hint)  # noqa: E731
        fns = {"rows": lambda: ops.relpos_attention_rows(qkv, pos, u, v, L, H, n0, k, ctx, keys_hint=n0 + k),
               "slots": lambda: slots(qkv, n0 + k)}
        res = {"keys": n0 + k, "nsplit": (ops._key_split if dt is None else ops._key_split16)(S, H, k, t_max, n0 + k)}
        if dt is not None:
            fns.update({"slots_nosplit": lambda: slots(qkv, 1), "slots_cache16": lambda: slots(qkv16, n0 + k),
                        "slots_cache16_nosplit": lambda: slots(qkv16, 1)})
        with _autocast(dt):
            for _ in range(2):                                  # alternate them, keep each one's best
                for name, fn in fns.items():
                    for _ in range(5):
                        fn()
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    us = e0.elapsed_time(e1) * 1e3 / iters
                    res[name + "_us"] = min(res.get(name + "_us", us), us)
        res["slots_over_rows"] = res["slots_us"] / res["rows_us"]
        rows.append(res)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, nargs="+", default=[8, 32])
    ap.add_argument("--chunk", type=int, default=640)
    ap.add_argument("--beam", type=int, default=100)
    ap.add_argument("--steps", type=int, default=24, help="steps of the staggered run")
    ap.add_argument("--lockstep-steps", type=int, default=10)
    ap.add_argument("--max-mel", type=int, default=20000)
    ap.add_argument("--lm-ngrams", type=int, default=100000, help="n-grams per order (2..5) of the synthetic ARPA model")
    ap.add_argument("--no-lm", action="store_true")
    ap.add_argument("--dtype", choices=["fp32", "bf16", "fp16"], default="fp32",
                    help="precision of the slot objects (dtype=) and autocast type of the lockstep and attention comparisons")
    ap.add_argument("--attention-only", action="store_true", help="only the attention section")
    ap.add_argument("--no-attention", action="store_true", help="skip the attention section")
    ap.add_argument("--left-context", type=int, default=None, help="bounded history: encoder frames a query looks back on")
    ap.add_argument("--max-pending", type=int, default=None,
                    help="commit mode: uncommitted tokens the best hypothesis may hold (left context 256 unless given)")
    args = ap.parse_args()
    if args.max_pending is not None and args.left_context is None:
        args.left_context = 256
    kw = {}
    if args.left_context is not None:
        kw = dict(left_context=args.left_context, max_chunk_mel_frames=args.chunk)
        if args.max_pending is not None:
            kw["max_pending"] = args.max_pending
    dt = {"fp32": None, "bf16": torch.bfloat16, "fp16": torch.float16}[args.dtype]
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    vocab = ["<pad>"] + [chr(ord("a") + i) for i in range(26)] + ["'", "|", "<unk>"]
    m = Conformer(len(vocab), 80, 16, 512, 8, 31, 640, 1, 0.0).to(dev).eval()
    out = {"what": "independent streams (slots): Conformer-L, 640-frame chunks, beam W=100", "chunk": args.chunk,
           "beam_width": args.beam, "dtype": args.dtype, "left_context": args.left_context, "max_pending": args.max_pending,
           "runs": [], "attention_ab": {}}
    with torch.no_grad():
        for S in [] if args.no_attention else args.slots:
            out["attention_ab"][f"S{S}"] = attention_ab(S, dev, dt)
            print(json.dumps({f"attention_ab S{S}": out["attention_ab"][f"S{S}"]}), file=sys.stderr, flush=True)
    if args.attention_only:
        print(json.dumps(out))
        return
    with tempfile.TemporaryDirectory() as tmp:
        lms = [("no_lm", None)]
        if not args.no_lm:
            arpa = os.path.join(tmp, "bench.arpa")
            write_synthetic_arpa(arpa, vocab[1:28], 20000, [0] + [args.lm_ngrams] * 4, seed=1, max_tokens_per_word=6)
            lms.append(("lm_5gram", arpa))
        for name, lm in lms:
            dec = BeamCTCDecoder(vocab, blank_id=0, skip_ids=(len(vocab) - 1,), beam_width=args.beam, lm=lm)
            for S in args.slots:
                tr = SlotTranscriber(m, dec, S, args.max_mel, dtype=dt, **kw)
                staggered(tr, S, args.chunk, 3, args.max_mel, 0, dev)          # warm-up
                del tr
                tr = SlotTranscriber(m, dec, S, args.max_mel, dtype=dt, **kw)
                run = {"decoder": name, "slots": S, "staggered": staggered(tr, S, args.chunk, args.steps, args.max_mel, 1, dev)}
                del tr
                torch.cuda.empty_cache()
                run["lockstep"] = lockstep(m, dec, S, args.chunk, args.lockstep_steps, dev, dt, kw)
                out["runs"].append(run)
                print(json.dumps(run), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
