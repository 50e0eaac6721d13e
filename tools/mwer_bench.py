#!/usr/bin/env python3
"""MWER training (conformer_amd.ops.ctc_nbest_*, ConformerCriterion.mwer_loss): what the n-best scores and their gradient cost
beside the only route the parent had.  Run once; no threshold is asserted.  Writes --out (profiles/mwer_bench.json) and prints the
same JSON.

Device events after warm-up, best of the alternated passes, B = --batch (64), T' = --frames (249), hypotheses of about --labels
(40) labels, for V in {370, 4096} and N in {2, 4, 8}:
  score         cfm3_ctc_nbest_score_f32 (workspace allocation included): ll (B, N)
  score_grad    ... followed by cfm3_ctc_nbest_grad_f32 with random weights: dlogits (B, T', V)
  repeat        the parent's route to the same numbers: logits.repeat_interleave(N, 0), cfm_ctc_loss_fwd_f32 and _bwd_f32 on the
                (B N, T', V) copy, and the sum of the N gradient blocks.  (Its per-row values come with the loss's own
                normalisation; the cost is what is compared.)
  shared_bytes / repeat_bytes   what each route moves through HBM by construction: the logits reads and gradient writes of
                (B, T', V) blocks, the (B, N, T') lattice rows, the label log-probabilities
  mwer_step     ConformerCriterion.mwer_loss(...).backward() whole (beam search W = --beam, edit distances, scores, risk, gradient),
                beside ctc_step, ctc_loss(...).backward() alone
The logits are synthetic: Gaussian, with 6 nats on the frames of a random alignment of the reference; the n-best rows are the
reference with one label changed per row, as the rows of a real list differ."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conformer_amd import ops  # noqa: E402
from conformer_amd.error_rate import ErrorRateTables  # noqa: E402
from conformer_amd.evaluation import ConformerCriterion  # noqa: E402


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
            res[name + "_us"] = round(min(res.get(name + "_us", us), us), 1)
    return res


def synthetic(B, T, V, L, N, dev, seed=0):
    """(logits, refs (B, L), ref_len (B), hyps (B, N, L), hyp_len (B, N), in_len (B))"""
    g = torch.Generator().manual_seed(seed)
    refs = torch.randint(1, V - 2, (B, L), generator=g)
    ref_len = torch.randint(max(1, L - 8), L + 1, (B,), generator=g)
    x = torch.randn(B, T, V, generator=g)
    in_len = torch.randint(max(2 * L + 1, T - 40), T + 1, (B,), generator=g)
    for b in range(B):                              # label i on frame (2 i + 1) * Tb / (2 L + 1), blank elsewhere
        Tb, Lb = int(in_len[b]), int(ref_len[b])
        x[b, :Tb, 0] += 6.0
        for i in range(Lb):
            t = (2 * i + 1) * Tb // (2 * Lb + 1)
            x[b, t, 0] -= 6.0
            x[b, t, refs[b, i]] += 6.0
    hyps = refs[:, None, :].repeat(1, N, 1)
    for n in range(1, N):
        hyps[:, n, (5 * n) % L] = torch.randint(1, V - 2, (B,), generator=g)
    hyp_len = ref_len[:, None].repeat(1, N)
    return [t.to(dev) for t in (x, refs, ref_len, hyps, hyp_len, in_len)]


def pairs(L):
    p = 1
    while 64 * p < L + 1:
        p *= 2
    return p


def traffic(B, N, T, V, L):
    """bytes through HBM by construction: (shared route, repeat route) for score + gradient"""
    block = B * T * V * 4
    lattice = B * N * T * 2 * 64 * pairs(L) * 4
    per_row = 2 * 2 * lattice + 3 * B * N * T * L * 4            # alpha and beta written and read; lpl written, read twice + once
    shared = 2 * block + block + per_row                        # logits read by prepare and grad, dlogits written once
    repeat = (block + N * block) + 2 * N * block + N * block + (N * block + block) + per_row
    return shared, repeat


def one_shape(B, T, V, L, N, dev, iters):
    x, refs, ref_len, hyps, hyp_len, in_len = synthetic(B, T, V, L, N, dev)
    w = torch.randn(B, N, device=dev)
    one = torch.ones((), device=dev)
    flat, flat_len, flat_in = hyps.reshape(B * N, L), hyp_len.reshape(-1), in_len.repeat_interleave(N)

    def score():
        return ops.ctc_nbest_forward(x, hyps, hyp_len, in_len, 0)

    def score_grad():
        _, ctx = ops.ctc_nbest_forward(x, hyps, hyp_len, in_len, 0)
        return ops.ctc_nbest_backward(ctx, w)

    def repeat_score():
        return ops.ctc_loss_forward(x.repeat_interleave(N, 0), flat, flat_in, flat_len, 0)

    def repeat():
        _, ctx = ops.ctc_loss_forward(x.repeat_interleave(N, 0), flat, flat_in, flat_len, 0)
        return ops.ctc_loss_backward(ctx, one).view(B, N, T, V).sum(1)

    res = dict(B=B, T=T, V=V, N=N, labels=L)
    res.update(best({"score": score, "score_grad": score_grad, "repeat_score": repeat_score, "repeat": repeat}, iters))
    res["shared_bytes"], res["repeat_bytes"] = traffic(B, N, T, V, L)
    res["repeat_over_shared_time"] = round(res["repeat_us"] / res["score_grad_us"], 3)
    return res


def whole_step(B, T, V, L, N, beam, dev, iters):
    x, refs, ref_len, hyps, hyp_len, in_len = synthetic(B, T, V, L, N, dev)
    vocab = ["<pad>"] + [f"t{i}" for i in range(V - 3)] + ["|", "<unk>"]
    tables = ErrorRateTables(vocab, "|", (0, V - 1))
    crit = ConformerCriterion(0)
    refs = refs.clone()
    refs[:, 5::6] = V - 2                           # a word every six tokens

    def mwer_step():
        xg = x.clone().requires_grad_(True)
        crit.mwer_loss(xg, refs, in_len, ref_len, tables, n_best=N, beam_width=beam).backward()

    def mwer_given():
        xg = x.clone().requires_grad_(True)
        crit.mwer_loss(xg, refs, in_len, ref_len, tables, hyp_tokens=hyps, hyp_counts=hyp_len).backward()

    def ctc_step():
        xg = x.clone().requires_grad_(True)
        crit.ctc_loss(xg, refs, in_len, ref_len).backward()

    res = dict(B=B, T=T, V=V, N=N, beam=beam)
    res.update(best({"mwer_step": mwer_step, "mwer_given_list": mwer_given, "ctc_step": ctc_step}, iters))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--labels", type=int, default=40)
    ap.add_argument("--beam", type=int, default=100)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mwer_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "mwer_bench needs the MI355X"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "shapes": [], "steps": []}
    for V in (370, 4096):
        for N in (2, 4, 8):
            out["shapes"].append(one_shape(a.batch, a.frames, V, a.labels, N, dev, a.iters))
        out["steps"].append(whole_step(a.batch, a.frames, V, a.labels, 4, a.beam, dev, max(2, a.iters // 3)))
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
