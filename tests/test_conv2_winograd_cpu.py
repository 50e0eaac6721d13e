"""The polyphase Winograd F(2x2,2x2) conv2 restated in float64 against conv2d (no GPU)."""
import pytest
import torch

from tests import conv2_winograd_restatement as W


def test_term_count_is_25():
    assert sum(len(W.pattern_terms(p)) for p in range(9)) == 25
    assert [len(W.pattern_terms(p)) for p in range(9)] == [4, 2, 4, 2, 1, 2, 4, 2, 4]


@pytest.mark.parametrize("B,T1,F1,C", [(2, 9, 11, 32), (1, 10, 12, 32), (3, 3, 5, 32), (1, 5, 3, 64), (2, 13, 8, 32)])
def test_winograd_matches_conv2d(B, T1, F1, C):
    g = torch.Generator().manual_seed(B * 1000 + T1 * 10 + F1)
    h1 = torch.randn(B, T1, F1, C, generator=g, dtype=torch.float64)
    w2 = torch.randn(C, C, 3, 3, generator=g, dtype=torch.float64)
    b2 = torch.randn(C, generator=g, dtype=torch.float64)
    # the direct conv on the stem's layout, checked against an explicit sum for one output
    ref = W.conv2_direct(h1, w2, b2)
    t2, f2 = ref.shape[1] - 1, ref.shape[2] - 1
    pre = b2.clone()
    for kf in range(3):
        for kt in range(3):
            pre += w2[:, :, kf, kt] @ h1[0, 2 * t2 + kt, 2 * f2 + kf]
    assert torch.allclose(ref[0, t2, f2], torch.relu(pre), rtol=0, atol=1e-12)
    got = W.conv2_winograd(h1, w2, b2)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) < 1e-11


def test_pixels_beyond_the_edge_feed_only_unwritten_outputs():
    # the kernel reads pixels past T1 / F1 without a select: they must not reach any valid output
    g = torch.Generator().manual_seed(5)
    B, T1, F1, C = 2, 9, 11, 32
    h1 = torch.randn(B, T1, F1, C, generator=g, dtype=torch.float64)
    w2 = torch.randn(C, C, 3, 3, generator=g, dtype=torch.float64)
    b2 = torch.zeros(C, dtype=torch.float64)
    T2, F2 = (T1 - 1) // 2, (F1 - 1) // 2
    TI, TJ = (T2 + 1) // 2, (F2 + 1) // 2
    big = torch.randn(B, 4 * TI + 1, 4 * TJ + 1, C, generator=g, dtype=torch.float64) * 1e6
    big[:, :T1, :F1] = h1
    y = W.combine(W.planes(big, w2), b2, T2, F2)
    assert float((y - W.conv2_winograd(h1, w2, b2)).abs().max()) < 1e-9


def test_pack_layout():
    C = 64
    w2 = torch.arange(C * C * 9, dtype=torch.float64).reshape(C, C, 3, 3)
    pk = W.pack(w2)
    assert pk.numel() == 25 * C * C
    # pattern 4 (centre) is the last but four blocks: offset 4+2+4+2 = 12 blocks; one term: w0+w2 in both dimensions
    blk = pk[12 * C * C: 13 * C * C].reshape(C, C)
    co, ci = 5, 37
    want = sum(w2[co, ci, kf, kt] for kf in (0, 2) for kt in (0, 2))
    assert blk[co, ci] == want
    # pattern 0 term u=1 (time term 0, frequency term 1): taps kt=0, kf=1; column 4*32*(ci//32) + 32 + ci%32
    blk0 = pk[:4 * C * C].reshape(C, 4 * C)
    assert blk0[co, 4 * 32 * (ci // 32) + 32 + ci % 32] == w2[co, ci, 1, 0]
