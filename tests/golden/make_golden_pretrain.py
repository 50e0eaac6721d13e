#!/usr/bin/env python3
"""Generate pretrain_quantizer.npz by running the REFERENCE's Quantization (model/modules/quantization.py) on the CPU, imported
the way make_golden.py imports the reference:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pretrain.py

Per shape (B, T, G, V, dg) the file holds the inputs (hidden_states, weight_proj, codevectors, a mask), the Gumbel tensor
F.gumbel_softmax drew (reproduced by re-seeding: it is the first and only draw of the forward), and per variant -- train with
the mask, train without, eval with the mask -- the reference's codevectors output, perplexity and codes, and in training the
autograd gradients of out.sum() * A + perplexity * B with respect to hidden_states, codevectors and weight_proj.  Only data is
stored.  Every recorded row keeps a gap above GAP between the largest and second-largest logits + noise (eval: logits), orders
of magnitude above fp32 GEMM drift, so a code cannot flip between the CPU and the device; a draw that misses it is repeated with
the next seed.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path = [p for p in sys.path if os.path.abspath(p or ".") != ROOT]
sys.path.insert(0, "/root/reference")

from model.modules.quantization import Quantization  # noqa: E402  (reference)

torch.set_num_threads(4)
GAP, A, B_ = 1e-3, 0.7, 1.3
D_MODEL, N_MEL = 2, 20                       # hidden width d_model * 4 = 8
SHAPES = [(2, 5, 2, 7, 4), (2, 9, 2, 320, 8)]


def npy(t):
    return t.detach().cpu().numpy()


def gap_of(x):
    top = x.topk(2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min())


def one_shape(i, shape, out):
    B, T, G, V, dg = shape
    seed = 1000 * (i + 1)
    while True:
        torch.manual_seed(seed)
        q = Quantization(D_MODEL, N_MEL, G, V, G * dg)
        with torch.no_grad():
            q.codevectors.uniform_()                      # the reference leaves it uninitialised
        x = torch.randn(B, T, D_MODEL * 4)
        mask = torch.rand(B, T) < 0.5
        mask[0, 0], mask[0, 1] = True, False
        logits = q.weight_proj(x).view(B * T * G, V).detach()
        torch.manual_seed(seed + 1)
        gumbel = -torch.empty_like(logits, memory_format=torch.legacy_contiguous_format).exponential_().log()
        if min(gap_of(logits + gumbel), gap_of(logits)) > GAP:
            break
        seed += 2
    p = f"s{i}_"
    out.update({p + "x": npy(x), p + "mask": npy(mask), p + "gumbel": npy(gumbel.view(B * T, G, V)),
                p + "weight": npy(q.weight_proj.weight), p + "bias": npy(q.weight_proj.bias),
                p + "codevectors": npy(q.codevectors)})
    for name, train, m in (("train_mask", True, mask), ("train_all", True, None), ("eval_mask", False, mask)):
        q.train(train)
        q.zero_grad()
        xi = x.clone().requires_grad_(True)
        torch.manual_seed(seed + 1)
        cvec, perp = q(xi, m)
        choice = (logits + gumbel if train else logits).argmax(-1).view(B * T, G)
        rows = q.codevectors[0].view(G, V, dg)
        want = torch.stack([rows[g][choice[:, g]] for g in range(G)], 1).view(B, T, G * dg)
        assert float((cvec - want).abs().max()) <= 2.0 ** -22 * float(want.abs().max()), name     # it forms 1 - p + p
        v = p + name + "_"
        out.update({v + "out": npy(cvec), v + "perplexity": npy(perp), v + "codes": npy(choice).astype(np.int32)})
        if train:
            (cvec.sum() * A + perp * B_).backward()
            out.update({v + "dx": npy(xi.grad), v + "dcodevectors": npy(q.codevectors.grad),
                        v + "dweight": npy(q.weight_proj.weight.grad), v + "dbias": npy(q.weight_proj.bias.grad)})
    return seed


def main():
    out, seeds = {}, []
    for i, shape in enumerate(SHAPES):
        seeds.append(one_shape(i, shape, out))
    meta = dict(shapes=SHAPES, seeds=seeds, gap=GAP, a=A, b=B_, d_model=D_MODEL, n_mel=N_MEL, tau=2,
                variants=["train_mask", "train_all", "eval_mask"])
    path = os.path.join(HERE, "pretrain_quantizer.npz")
    np.savez_compressed(path, meta=np.array(json.dumps(meta)), **out)
    print(f"pretrain_quantizer: {os.path.getsize(path) / 1024:.1f} KiB, seeds {seeds}")
    assert os.path.getsize(path) < 200 * 1024


if __name__ == "__main__":
    main()
