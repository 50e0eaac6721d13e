#!/usr/bin/env python3
"""CTC prefix beam search with and without hotword boosting at the model's decode shape: B = 32 utterances, T = 249 frames,
V = 370 tokens (blank, the delimiter "|", <unk> and 367 graphemes), W in {100, 190}, K = 16, token_min_logp = -5,
beam_prune_logp = -10, hotword_weight = 9.  The hotwords are 20 synthetic phrases of 1 to 3 words drawn from the words of
the synthetic 5-gram of tools/ctc_beam_lm_bench.py (about 1 M n-grams over 20 000 words, fixed seeds).  Device time per
call from HIP events after a warm-up: the boosted search (beam_ctc_hotword_decode) beside the same search without hotwords,
LM-free (beam_ctc_decode) and fused with the 5-gram (beam_ctc_lm_decode, alpha = 2.1, beta = 9.2), on the same logits; one
JSON line.  Logits as in tools/ctc_beam_bench.py: "random" (randn * 2) and "peaky" (one id per frame 12 above the rest,
every other frame blank).

    python tools/ctc_beam_hotword_bench.py [--iters 20] [--no-lm]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd.decode import beam_ctc_decode, beam_ctc_hotword_decode, beam_ctc_lm_decode  # noqa: E402
from conformer_amd.hotwords import Hotwords  # noqa: E402
from conformer_amd.lm import NgramLanguageModel, write_synthetic_arpa  # noqa: E402

B, T = 32, 249
WIDTHS = (100, 190)
COUNTS = [0, 300_000, 330_000, 250_000, 120_000]          # + 20 003 unigrams: ~1.02 M n-grams
N_PHRASES = 20


def graphemes(n: int):
    letters = [chr(ord("A") + i) for i in range(26)]
    out = list(letters)
    for a in letters:
        for b in letters:
            if len(out) == n:
                return out
            out.append(a + b)
    return out


def logits_for(kind: str, V: int, dev) -> torch.Tensor:
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, V, generator=g) * 2
    if kind == "peaky":
        ids = torch.randint(0, V, (B, T, 1), generator=g)
        ids[:, ::2] = 0
        x.scatter_(-1, ids, 12.0)
    return x.to(dev)


def timed(fn, iters: int) -> float:
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / iters, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-lm", action="store_true", help="skip the runs fused with the 5-gram")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ctc_beam_hotword_bench: no HIP device (the decode only runs on the GPU; there is nothing to time here)")
    dev = torch.device("cuda:0")
    toks = graphemes(367)
    vocab = ["<pad>", "|", "<unk>"] + toks
    t0 = time.time()
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "synthetic5.arpa")
        words = write_synthetic_arpa(path, toks, 20_000, COUNTS if not args.no_lm else [0, 10], seed=0)
        lm = None if args.no_lm else NgramLanguageModel.from_arpa(path)
    rng = np.random.default_rng(1)
    phrases = [" ".join(rng.choice(words, size=int(rng.integers(1, 4)))) for _ in range(N_PHRASES)]
    hw = Hotwords(phrases)
    hw.device_tables(vocab, "|", (2,), dev)
    if lm is not None:
        lm.device_tables(vocab, "|", (2,), dev)
    setup_s = round(time.time() - t0, 1)
    L = torch.full((B,), T, dtype=torch.int64, device=dev)
    out = {"B": B, "T": T, "V": len(vocab), "K": 16, "iters": args.iters, "phrases": len(hw), "hotword_weight": 9.0,
           "lm_ngrams": None if lm is None else sum(lm.counts), "setup_s": setup_s, "ms": {}}
    kw = dict(vocab=vocab, skip_ids=(2,))
    for kind in ("random", "peaky"):
        x = logits_for(kind, len(vocab), dev)
        out["ms"][kind] = {}
        for W in WIDTHS:
            r = {}
            free = timed(lambda: beam_ctc_decode(x, 0, L, beam_width=W), args.iters)
            boosted = timed(lambda: beam_ctc_hotword_decode(x, 0, hw, L, beam_width=W, **kw), args.iters)
            r["lm_free"] = {"plain": free, "hotwords": boosted, "ratio": round(boosted / free, 3)}
            if lm is not None:
                fused = timed(lambda: beam_ctc_lm_decode(x, 0, lm, L, beam_width=W, **kw), args.iters)
                both = timed(lambda: beam_ctc_hotword_decode(x, 0, hw, L, lm=lm, beam_width=W, **kw), args.iters)
                r["lm"] = {"plain": fused, "hotwords": both, "ratio": round(both / fused, 3)}
            out["ms"][kind][str(W)] = r
    print(json.dumps(out))


if __name__ == "__main__":
    main()
