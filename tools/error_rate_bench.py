#!/usr/bin/env python3
"""Error rates on the device (conformer_amd.error_rate.ErrorRateMeter) against ConformerMetric on the decoded strings.

On random token rows over a grapheme vocabulary of 1-3 code points per token, two sizes: B = 32 greedy rows of about 100 tokens,
and B = 32 utterances x N = 8 beam rows of about 250 tokens.  Per size, after warm-up, best of the alternated passes:
  device_ms    ErrorRateMeter.update + compute (two extraction launches, one distance launch for words, characters and tokens
               and the oracle, the sums, one copy of the totals), a host clock around work that ends in compute()'s copy
  kernels_us   the three launches alone between two device events (mean of --iters back-to-back rounds)
  host_ms      the same numbers the way they were scored before: tokens.cpu(), BeamCTCDecoder.text per row, then
               ConformerMetric.wer_score and cer_score (and, for n-best rows, the oracle WER: wer_score per row, the minimum);
               no token error rate, which the host side never had
and the totals of both sides, which must agree."""
import argparse
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from conformer_amd import _lib  # noqa: E402
from conformer_amd import error_rate as er  # noqa: E402
from conformer_amd.decode import BeamCTCDecoder  # noqa: E402
from conformer_amd.evaluation import ConformerMetric, _edit_distance  # noqa: E402


def vocabulary(rng, n=96):
    """<pad>, |, <unk>, then n distinct graphemes of 1-3 code points (Latin letters with combining marks)"""
    base = [chr(c) for c in range(ord("a"), ord("z") + 1)] + list("ăâêôơưđ")
    marks = ["́", "̀", "̉", "̃", "̣"]
    seen, out = set(), []
    while len(out) < n:
        g = rng.choice(base) + "".join(rng.sample(marks, rng.choice([0, 0, 1, 1, 2])))
        if g not in seen:
            seen.add(g)
            out.append(g)
    return ["<pad>", "|", "<unk>"] + out


def rows(rng, V, n, mean_len, width):
    """n rows of about mean_len tokens: words of 1-6 graphemes between delimiters, a stray <unk> now and then"""
    out = []
    for _ in range(n):
        L = min(width, max(1, int(rng.gauss(mean_len, mean_len / 8))))
        row = []
        while len(row) < L:
            row += [rng.randrange(3, V) for _ in range(rng.randint(1, 6))] + [1]
            if rng.random() < 0.05:
                row.append(2)
        out.append(row[:L])
    return out


def noisy(rng, V, row, rate, width):
    out = []
    for t in row:
        r = rng.random()
        if r < rate / 3:
            continue
        out.append(rng.randrange(3, V) if r < 2 * rate / 3 else t)
        if r > 1 - rate / 3:
            out.append(rng.randrange(1, V))
    return out[:width]


def padded(rws, width, dev):
    t = torch.full((len(rws), width), -1, dtype=torch.int64)
    for i, r in enumerate(rws):
        t[i, :len(r)] = torch.tensor(r, dtype=torch.int64)
    return t.to(dev), torch.tensor([len(r) for r in rws], dtype=torch.int64, device=dev)


def host_score(dec, metric, ht, hc, rt, rc, N):
    """what a validation pass did before: ids to the host, strings, ConformerMetric"""
    tk, ct = ht.cpu().tolist(), hc.cpu().tolist()
    rk, rn = rt.cpu().tolist(), rc.cpu().tolist()
    refs = [dec.text(r[:n]) for r, n in zip(rk, rn)]
    if N == 1:
        hyps = [dec.text(r[:n]) for r, n in zip(tk, ct)]
        return {"wer": float(metric.wer_score(hyps, refs)), "cer": float(metric.cer_score(hyps, refs))}
    best = [dec.text(tk[b][0][:ct[b][0]]) for b in range(len(refs))]
    errors = total = 0
    for b, ref in enumerate(refs):
        words = ref.split()
        errors += min(_edit_distance(words, dec.text(tk[b][n][:ct[b][n]]).split()) for n in range(N) if n == 0 or ct[b][n] > 0)
        total += len(words)
    return {"wer": float(metric.wer_score(best, refs)), "cer": float(metric.cer_score(best, refs)),
            "oracle_wer": errors / total if total else float("nan")}


def run(name, B, N, mean_len, width, args, dev, rng, vocab):
    V = len(vocab)
    tables = er.ErrorRateTables(vocab, "|", (0, 2))
    dec = BeamCTCDecoder(vocab, blank_id=0, skip_ids=(0, 2))
    metric = ConformerMetric()
    refs = rows(rng, V, B, mean_len, width)
    hyps = [noisy(rng, V, r, 0.1 + 0.05 * n, width) for r in refs for n in range(N)]
    ht, hc = padded(hyps, width, dev)
    rt, rc = padded(refs, width, dev)
    if N > 1:
        ht, hc = ht.reshape(B, N, width), hc.reshape(B, N)

    def device():
        m = er.ErrorRateMeter(tables)
        m.update(ht, hc, rt, rc)
        return m.compute()

    def kernels():
        er._counts(ht, hc, rt, rc, tables, 3, "bench")

    res = {"case": name, "utterances": B, "n_best": N, "row_width": width,
           "mean_tokens": sum(map(len, refs)) / B, "mean_ref_chars": None}
    for _ in range(3):
        kernels()
        got = device()
    torch.cuda.synchronize()
    res["mean_ref_chars"] = got["ref_chars"] / B
    for _ in range(args.passes):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = device()
        ms = (time.perf_counter() - t0) * 1e3
        res["device_ms"] = min(res.get("device_ms", ms), ms)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.iters):
            kernels()
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / args.iters
        res["kernels_us"] = min(res.get("kernels_us", us), us)
        t0 = time.perf_counter()
        want = host_score(dec, metric, ht, hc, rt, rc, N)
        ms = (time.perf_counter() - t0) * 1e3
        res["host_ms"] = min(res.get("host_ms", ms), ms)
    res["host_over_device"] = res["host_ms"] / res["device_ms"]
    res["device"] = {k: got[k] for k in ("wer", "cer", "ter", "oracle_wer", "oracle_cer", "oracle_ter")}
    res["host"] = want
    for k, v in want.items():                                                 # the host side rounds its ratio to float32
        assert float(torch.tensor(got[k])) == float(torch.tensor(v)), (name, k, got[k], v)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=3)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    _lib.check(_lib.load().cfm_device_check(), "cfm_device_check")
    rng = random.Random(args.seed)
    vocab = vocabulary(rng)
    out = {"what": "ErrorRateMeter.update + compute against ConformerMetric on the decoded strings", "runs": []}
    for name, B, N, mean_len, width in (("greedy", 32, 1, 100, 160), ("beam", 32, 8, 250, 400)):
        res = run(name, B, N, mean_len, width, args, dev, rng, vocab)
        out["runs"].append(res)
        print(json.dumps(res), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
