#!/usr/bin/env python3
"""Self-supervised pretraining (conformer_amd.pretrain, model.wav2vec2.Wav2Vec2, ConformerCriterion.pretrain_loss): what the Gumbel
quantizer and the contrastive loss cost beside the same objective written in stock PyTorch-ROCm operators, in the same process.
Run once; no threshold is asserted.  Writes --out (profiles/pretrain_bench.json) and prints the same JSON.

Device events after warm-up, best of the alternated passes.  B = --batch (32), T' = --frames (249), D = 256, K = 100 negatives,
G = 2 groups of V = 320 codes of dg = 128, about half the frames masked (span_mask, p = 0.065, span = 10).
  quant_fwd / quant_fwd_bwd         ops.quantize_forward (+ ops.quantize_backward), workspace allocation included
  stock_quant_fwd / _fwd_bwd        the reference's formulation: hard Gumbel-softmax by the straight-through one-hot, the
                                    (N G V, dg) product with the one-hot rows, the perplexity of the masked mean softmax; autograd
  con_fwd / con_fwd_bwd             ops.contrastive_forward (+ ops.contrastive_backward, the stable sort of the draws included)
  stock_con_fwd / _fwd_bwd          gather of the (M, K + 1, D) candidates of the M masked frames, F.cosine_similarity,
                                    F.cross_entropy (sum); autograd
  *_peak_bytes                      torch.cuda.max_memory_allocated over one call, above what was allocated before it
  pretrain_step / ctc_step          Wav2Vec2 forward + pretrain_loss + backward beside Conformer forward + ctc_loss + backward:
                                    Conformer-L (16 blocks, d = 512), fp32, B x 1000 mel frames, no dropout, no optimiser
Both formulations get the same inputs, noise, mask and negatives; their results are compared before anything is timed."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from conformer_amd import ops, pretrain  # noqa: E402
from conformer_amd.evaluation import ConformerCriterion  # noqa: E402


def timed(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def best(fns, iters, passes=3):
    res = {}
    for _ in range(passes):
        for name, fn in fns.items():
            us = timed(fn, iters)
            res[name + "_us"] = round(min(res.get(name + "_us", us), us), 1)
    return res


def peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    del out
    return int(rise)


def quantizer(N, G, V, dg, tau, dev, iters, mask):
    g = torch.Generator().manual_seed(0)
    logits = (2 * torch.randn(N, G, V, generator=g)).to(dev)
    noise = -torch.empty(N, G, V).exponential_(generator=g).log().to(dev)
    cv = torch.rand(G * V, dg, generator=g).to(dev)
    dout = torch.randn(N, G * dg, generator=g).to(dev)
    one = torch.ones((), device=dev)
    rows = mask.reshape(-1)

    def ours_fwd():
        return ops.quantize_forward(logits, cv, tau, noise, rows)

    def ours():
        *_, ctx = ops.quantize_forward(logits, cv, tau, noise, rows)
        return ops.quantize_backward(ctx, dout, one)

    def stock_fwd(lg=logits, c=cv):
        x = lg.view(N * G, V)
        y = torch.softmax((x + noise.view(N * G, V)) / tau, dim=-1)
        hard = torch.zeros_like(y).scatter_(-1, y.argmax(dim=-1, keepdim=True), 1.0)
        probs = (hard - y.detach() + y).view(N, G * V)
        soft = torch.softmax(lg, dim=-1)
        marginal = torch.where(rows[:, None, None], soft, torch.zeros_like(soft)).sum(0) / rows.sum()
        perplexity = torch.exp(-torch.sum(marginal * torch.log(marginal + 1e-7), dim=-1)).sum()
        per_group = probs.unsqueeze(-1) * c.unsqueeze(0)                               # (N, G V, dg)
        return per_group.view(N, G, V, -1).sum(-2).view(N, -1), perplexity

    def stock():
        lg, c = logits.detach().requires_grad_(True), cv.detach().requires_grad_(True)
        out, perplexity = stock_fwd(lg, c)
        ((out * dout).sum() + perplexity).backward()
        return lg.grad, c.grad

    out, _, perp, _, _ = ours_fwd()
    sout, sperp = stock_fwd()
    (dl, dc), (sl, sc) = ours(), stock()
    agree = dict(out=float((out - sout).abs().max()), perplexity=abs(float(perp) - float(sperp)),
                 dlogits=float((dl - sl).abs().max() / sl.abs().max()), dcodevectors=float((dc - sc).abs().max() / sc.abs().max()))
    res = dict(N=N, G=G, V=V, dg=dg, max_difference=agree)
    res.update(best({"quant_fwd": ours_fwd, "quant_fwd_bwd": ours, "stock_quant_fwd": stock_fwd, "stock_quant_fwd_bwd": stock}, iters))
    res["quant_fwd_bwd_peak_bytes"], res["stock_quant_fwd_bwd_peak_bytes"] = peak(ours), peak(stock)
    res["stock_over_ours_fwd"] = round(res["stock_quant_fwd_us"] / res["quant_fwd_us"], 2)
    res["stock_over_ours_fwd_bwd"] = round(res["stock_quant_fwd_bwd_us"] / res["quant_fwd_bwd_us"], 2)
    return res


def contrastive(B, T, D, K, temp, dev, iters, mask):
    g = torch.Generator().manual_seed(1)
    context, targets = torch.randn(B, T, D, generator=g).to(dev), torch.randn(B, T, D, generator=g).to(dev)
    negatives = pretrain.sample_negatives(mask, K, torch.Generator(device=dev).manual_seed(2))
    gframe = torch.ones(B, T, device=dev)
    bidx, tidx = mask.nonzero(as_tuple=True)
    cand_idx = torch.cat([tidx[:, None], negatives[bidx, tidx].long()], dim=1)           # (M, K + 1), built once, outside the timing
    label = torch.zeros(len(bidx), dtype=torch.long, device=dev)

    def ours_fwd():
        return ops.contrastive_forward(context, targets, mask, negatives, None, temp)

    def ours():
        *_, ctx = ops.contrastive_forward(context, targets, mask, negatives, None, temp)
        return ops.contrastive_backward(ctx, gframe)

    def stock_fwd(c=context, t=targets):
        cand = t[bidx[:, None], cand_idx]                                                # (M, K + 1, D)
        z = F.cosine_similarity(c[bidx, tidx][:, None, :], cand, dim=-1) / temp
        return F.cross_entropy(z, label, reduction="sum")

    def stock():
        c, t = context.detach().requires_grad_(True), targets.detach().requires_grad_(True)
        stock_fwd(c, t).backward()
        return c.grad, t.grad

    loss = ours_fwd()[0]
    sloss = stock_fwd()
    (dc, dt), (sc, st) = ours(), stock()
    agree = dict(loss=abs(float(loss) - float(sloss)) / abs(float(sloss)), dcontext=float((dc - sc).abs().max() / sc.abs().max()),
                 dtargets=float((dt - st).abs().max() / st.abs().max()))
    res = dict(B=B, T=T, D=D, K=K, masked=int(mask.sum()), max_relative_difference=agree)
    res.update(best({"con_fwd": ours_fwd, "con_fwd_bwd": ours, "stock_con_fwd": stock_fwd, "stock_con_fwd_bwd": stock}, iters))
    res["con_fwd_bwd_peak_bytes"], res["stock_con_fwd_bwd_peak_bytes"] = peak(ours), peak(stock)
    res["stock_over_ours_fwd"] = round(res["stock_con_fwd_us"] / res["con_fwd_us"], 2)
    res["stock_over_ours_fwd_bwd"] = round(res["stock_con_fwd_bwd_us"] / res["con_fwd_bwd_us"], 2)
    return res


def whole_step(B, mel_frames, D, K, G, V, dev, iters):
    from model.conformer import Conformer
    from model.wav2vec2 import Wav2Vec2
    torch.manual_seed(0)
    w2v = Wav2Vec2(16, 80, 512, 8, 31, D, G, V, time_augment=10, time_mask_ratio=0.065).to(dev).train()
    asr = Conformer(370, 80, 16, 512, 8, 31, 640, 1, 0.0).to(dev).train()
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, 80, mel_frames, generator=g).to(dev)
    lengths = torch.full((B,), mel_frames, dtype=torch.int64, device=dev)
    tokens = torch.randint(1, 370, (B, 40), generator=g).to(dev)
    tlen = torch.full((B,), 40, dtype=torch.int64, device=dev)
    crit = ConformerCriterion(0)
    gen = torch.Generator(device=dev).manual_seed(4)

    def pretrain_step():
        w2v.zero_grad(set_to_none=True)
        context, target, perplexity, mask = w2v(x, lengths, generator=gen)
        crit.pretrain_loss(context, target, perplexity, mask, codes=w2v.quantization.last_codes, num_negatives=K, generator=gen,
                           num_codevectors=G * V).backward()

    def ctc_step():
        asr.zero_grad(set_to_none=True)
        logits, out_len = asr(x, lengths)
        crit.ctc_loss(logits, tokens, out_len, tlen).backward()

    res = dict(B=B, mel_frames=mel_frames, blocks=16, d_model=512, dtype="fp32")
    res.update(best({"pretrain_step": pretrain_step, "ctc_step": ctc_step}, iters, passes=2))
    res["pretrain_over_ctc"] = round(res["pretrain_step_us"] / res["ctc_step_us"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--frames", type=int, default=249)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-step", action="store_true", help="skip the whole-step comparison")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pretrain_bench.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "pretrain_bench needs the MI355X"
    dev = torch.device("cuda:0")
    B, T, D, K, G, V, dg = a.batch, a.frames, 256, 100, 2, 320, 128
    lengths = torch.full((B,), T, dtype=torch.int64, device=dev)
    mask = pretrain.span_mask(lengths, T, 0.065, 10, torch.Generator(device=dev).manual_seed(0))
    out = {"device": torch.cuda.get_device_name(0), "masked_share": round(float(mask.float().mean()), 3)}
    out["quantizer"] = quantizer(B * T, G, V, dg, 2.0, dev, a.iters, mask)
    out["contrastive"] = contrastive(B, T, D, K, 0.1, dev, a.iters, mask)
    if not a.no_step:
        out["step"] = whole_step(B, 4 * T + 4, D, K, G, V, dev, max(3, a.iters // 5))
    text = json.dumps(out, indent=1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
