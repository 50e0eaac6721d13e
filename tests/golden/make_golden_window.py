#!/usr/bin/env python3
"""Generate the bounded-history goldens (stream_window_mhsa_*.npz) by running the REFERENCE itself on CPU.

Run once in the build container (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_window.py

As make_golden.py::stream_mask_case -- same weights, same inputs, MultiHeadSelfAttentionModule under a (1, 1, T', T') bool
mask -- but the mask is BANDED: row i hides the keys at or past the end of its own chunk AND the keys more than `left` frames
behind it, (j >= visible_end[i]) | (j < i - left): the windowed prefix rule of conformer_amd/streaming.py.
"""
import numpy as np
import torch

# (make_golden puts the reference on sys.path and loads the oracle by file path)
from make_golden import MultiHeadSelfAttentionModule, O, RelativePositionalEncoding, npy, save, sub


def stream_window_case(tag, d, H, B, T, chunk_ends, left, seed):
    cfg = dict(vocab=11, n_mel=80, n_blocks=1, d=d, n_heads=H, ksize=15, lstm_hidden=16, seed=seed)
    P = O.make_params(**cfg)
    g = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(B, T, d, generator=g)
    rel = RelativePositionalEncoding(d)
    rel.load_state_dict({"div_term": P["encoder.rel_pe.div_term"]})
    pe = rel(x)
    visible_end = torch.empty(T, dtype=torch.long)
    start = 0
    for e in chunk_ends:
        visible_end[start:e] = e
        start = e
    assert start == T
    i, j = torch.arange(T)[:, None], torch.arange(T)[None, :]
    mask = ((j >= visible_end[:, None]) | (j < i - left))[None, None]          # (1, 1, T, T), True = hidden
    m = MultiHeadSelfAttentionModule(d, H).eval()
    m.load_state_dict(sub(P, "encoder.layers.0.attention."))
    with torch.no_grad():
        y = m(x, pe, mask)
    save(f"stream_window_mhsa_{tag}_l{left}", dict(cfg, B=B, T=T, left=left), x=npy(x),
         chunk_ends=np.array(chunk_ends, dtype=np.int64), mhsa_y=npy(y))


if __name__ == "__main__":
    torch.manual_seed(0)
    # the inputs and weights of stream_mhsa_d64_t70 / stream_mhsa_d144_t49 (same seeds): the siblings differ by the mask alone
    stream_window_case("d64_t70", d=64, H=4, B=2, T=70, chunk_ends=[9, 10, 33, 34, 57, 70], left=24, seed=51)
    stream_window_case("d144_t49", d=144, H=4, B=1, T=49, chunk_ends=[5, 21, 22, 40, 49], left=7, seed=52)
