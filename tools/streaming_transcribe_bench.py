#!/usr/bin/env python3
"""BASELINE cfg-5 with text out: streaming transcription (conformer_amd.transcribe.StreamingTranscriber), B=8, T=20000 mel
frames in 640-frame chunks, Conformer-L, resumable CTC beam search at W=100, with and without a word n-gram LM.  Reports the
per-chunk latency split into encoder step, decoder LSTM + projection, and beam step (each part synchronised and timed on its
own), the whole-stream time with the parts back to back, and the real-time factor per stream.  --left-context L: bounded
history; --max-pending M (with it; L defaults to 256): the beam step commits, its buffers no longer scale with --frames.
Random weights, so the
logits are not peaky: the beam search runs at its random-logit cost (the upper end)."""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd.decode import BeamCTCDecoder  # noqa: E402
from conformer_amd.lm import write_synthetic_arpa  # noqa: E402
from conformer_amd.transcribe import StreamingTranscriber  # noqa: E402
from model.conformer import Conformer  # noqa: E402


def percentiles(xs):
    s = sorted(xs)
    return {"first": xs[0], "median": s[len(s) // 2], "max": s[-1], "total": sum(xs)}


def run(tr, x, chunk, repeats):
    best = None
    for _ in range(repeats + 1):                          # the first pass warms up (packs, tables, caches)
        tr.reset()
        torch.cuda.synchronize()
        enc_ms, dec_ms, beam_ms = [], [], []
        t0 = time.perf_counter()
        for t in range(0, x.shape[2], chunk):
            a = time.perf_counter()
            h = tr.encoder.step(x[:, :, t:t + chunk])
            torch.cuda.synchronize()
            b = time.perf_counter()
            if h.shape[1]:
                logits = tr.decode_frames(h)
                torch.cuda.synchronize()
                c = time.perf_counter()
                tr.beam.step(logits)
                torch.cuda.synchronize()
                d = time.perf_counter()
            else:
                c = d = b
            enc_ms.append((b - a) * 1e3)
            dec_ms.append((c - b) * 1e3)
            beam_ms.append((d - c) * 1e3)
        tr.finish()
        total = time.perf_counter() - t0
        if best is None or total < best[0]:
            best = (total, enc_ms, dec_ms, beam_ms)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--frames", type=int, default=20000)
    ap.add_argument("--chunk", type=int, default=640)
    ap.add_argument("--beam", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--lm-ngrams", type=int, default=200000, help="n-grams per order (2..5) of the synthetic ARPA model")
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
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    vocab = ["<pad>"] + [chr(ord("a") + i) for i in range(26)] + ["'", "|", "<unk>"]
    m = Conformer(len(vocab), 80, 16, 512, 8, 31, 640, 1, 0.0).to(dev).eval()
    x = torch.randn(args.batch, 80, args.frames, device=dev)
    audio_s = args.frames * 0.010
    out = {"what": "cfg-5 streaming transcription: encoder step + carried-state decoder + resumable beam step",
           "batch": args.batch, "mel_frames": args.frames, "chunk": args.chunk, "beam_width": args.beam,
           "left_context": args.left_context, "max_pending": args.max_pending, "runs": []}
    with tempfile.TemporaryDirectory() as tmp:
        arpa = os.path.join(tmp, "bench.arpa")
        write_synthetic_arpa(arpa, vocab[1:28], 20000, [0] + [args.lm_ngrams] * 4, seed=1, max_tokens_per_word=6)
        for name, lm in (("no_lm", None), ("lm_5gram", arpa)):
            dec = BeamCTCDecoder(vocab, blank_id=0, skip_ids=(len(vocab) - 1,), beam_width=args.beam, lm=lm)
            tr = StreamingTranscriber(m, dec, args.batch, args.frames, **kw)
            total, enc_ms, dec_ms, beam_ms = run(tr, x, args.chunk, args.repeats)
            out["runs"].append({"decoder": name, "stream_ms": total * 1e3, "chunks": len(enc_ms),
                                "realtime_factor_per_stream": audio_s / total,
                                "encoder_ms": percentiles(enc_ms), "decoder_lstm_proj_ms": percentiles(dec_ms),
                                "beam_step_ms": percentiles(beam_ms)})
            del tr
    print(json.dumps(out))


if __name__ == "__main__":
    main()
