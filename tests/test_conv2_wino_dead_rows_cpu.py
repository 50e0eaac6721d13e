"""The Winograd conv2's per-pattern row map restated (csrc/conv2_wino_f32.hip, "Dead rows"): a pattern with b = 2 runs over
TJ - 1 frequency blocks when F2 is odd, one with a = 2 over TI - 1 time blocks when T2 is odd, and its rows sit densely at the
head of its plane.  Shown here in float64, without a GPU: every valid output still finds exactly its four planes, no row
that a pattern skips is read, and the GEMM's tile list names every row tile of every pattern once."""
import pytest
import torch

from tests import conv2_winograd_restatement as W

GROUPS = [(0, 2, 6, 8), (1, 7, 3, 5), (4,)]        # launch groups: corners, edges, centre


def grid(p, TI, TJ, T2, F2):
    """Pattern p's block grid (TI_p, TJ_p)."""
    a, b = divmod(p, 3)
    return TI - (a == 2 and T2 % 2), TJ - (b == 2 and F2 % 2)


def row_to_block(p, m, TI, TJ, T2, F2):
    """GEMM side: row m of pattern p -> (bb, ib, jb)."""
    TIp, TJp = grid(p, TI, TJ, T2, F2)
    bb, r = divmod(m, TIp * TJp)
    return (bb,) + divmod(r, TJp)


def block_to_row(p, bb, ib, jb, TI, TJ, T2, F2):
    """Combine side: the row of block (bb, ib, jb) in pattern p's plane, None where the plane has none."""
    TIp, TJp = grid(p, TI, TJ, T2, F2)
    return (bb * TIp + ib) * TJp + jb if ib < TIp and jb < TJp else None


SHAPES = [(2, 9, 11), (2, 11, 11), (2, 9, 13), (1, 13, 13), (3, 3, 3), (2, 4, 9), (2, 9, 4), (2, 3, 11), (1, 23, 3)]


@pytest.mark.parametrize("B,T1,F1", SHAPES)
def test_every_valid_output_gets_its_four_planes(B, T1, F1):
    C = 8
    g = torch.Generator().manual_seed(100 * T1 + F1)
    h1 = torch.randn(B, T1, F1, C, generator=g, dtype=torch.float64)
    w2 = torch.randn(C, C, 3, 3, generator=g, dtype=torch.float64)
    b2 = torch.randn(C, generator=g, dtype=torch.float64)
    T2, F2 = (T1 - 1) // 2, (F1 - 1) // 2
    TI, TJ = (T2 + 1) // 2, (F2 + 1) // 2
    full = W.planes(h1, w2)                                     # (9, B, TI, TJ, C)
    M = B * TI * TJ
    store = torch.full((9, M, C), float("nan"), dtype=torch.float64)   # what the GEMMs leave: plane stride M, short planes dense
    for p in range(9):
        TIp, TJp = grid(p, TI, TJ, T2, F2)
        Mp = B * TIp * TJp
        seen = set()
        for m in range(Mp):
            bb, ib, jb = row_to_block(p, m, TI, TJ, T2, F2)
            assert bb < B and ib < TIp and jb < TJp
            assert block_to_row(p, bb, ib, jb, TI, TJ, T2, F2) == m
            seen.add((bb, ib, jb))
            store[p, m] = full[p, bb, ib, jb]
        assert len(seen) == Mp
    y = torch.empty(B, T2, F2, C, dtype=torch.float64)
    for bb in range(B):
        for t2 in range(T2):
            for f2 in range(F2):
                ib, r = divmod(t2, 2)
                jb, s = divmod(f2, 2)
                rows = [(3 * a + b, block_to_row(3 * a + b, bb, ib, jb, TI, TJ, T2, F2)) for a in (r, r + 1) for b in (s, s + 1)]
                assert all(m is not None for _, m in rows), (t2, f2, rows)
                y[bb, t2, f2] = sum(store[p, m] for p, m in rows)
    y = torch.relu(y + b2)
    assert not torch.isnan(y).any()
    ref = W.conv2_direct(h1, w2, b2)
    assert float((y - ref).abs().max()) < 1e-11
    # the rows a short plane lacks are exactly those of blocks whose pattern-2 output does not exist
    for p in range(9):
        a, b = divmod(p, 3)
        for ib in range(TI):
            for jb in range(TJ):
                dead = (a == 2 and 2 * ib + 1 >= T2) or (b == 2 and 2 * jb + 1 >= F2)
                assert (block_to_row(p, 0, ib, jb, TI, TJ, T2, F2) is None) == dead


def tile_list(nb, TI, TJ, T2, F2, tiles_n, BM=256):
    """The pattern GEMM's launch restated: per group the patterns sorted by row tiles (ascending, stable); row tiles
    [tm[k - 1], tm[k]) are run by the patterns k .. 3 of that order; the list is cut into 8 per-XCD ranges."""
    out = []
    for pats in GROUPS:
        pats = [None] * (4 - len(pats)) + list(pats)
        tiles = []
        for p in pats:
            TIp, TJp = (0, 0) if p is None else grid(p, TI, TJ, T2, F2)
            tiles.append((nb * TIp * TJp + BM - 1) // BM)
        order = sorted(range(4), key=lambda i: tiles[i])        # (stable)
        tm_sorted = [tiles[i] for i in order]
        pat_sorted = [pats[i] for i in order]
        total = sum(tiles) * tiles_n
        blocks = (total + 7) // 8 * 8
        per_xcd = blocks // 8
        for local in range(blocks):
            tile = (local & 7) * per_xcd + (local >> 3)
            k, lo = 0, 0
            while k < 4:
                seg = (tm_sorted[k] - lo) * (4 - k) * tiles_n
                if tile < seg:
                    break
                tile -= seg
                lo = tm_sorted[k]
                k += 1
            if k == 4:
                continue
            tn, rest = tile % tiles_n, tile // tiles_n
            out.append((pat_sorted[k + rest % (4 - k)], lo + rest // (4 - k), tn))
    return out


@pytest.mark.parametrize("nb,T1,F1,tiles_n", [(32, 499, 39, 2), (16, 19, 15, 1), (3, 499, 39, 1), (2, 3, 3, 1), (2, 4, 9, 1),
                                               (5, 23, 3, 2), (7, 21, 13, 2), (64, 499, 39, 2)])
def test_tile_list_covers_every_pattern_once(nb, T1, F1, tiles_n):
    T2, F2 = (T1 - 1) // 2, (F1 - 1) // 2
    TI, TJ = (T2 + 1) // 2, (F2 + 1) // 2
    got = tile_list(nb, TI, TJ, T2, F2, tiles_n)
    want = set()
    for p in range(9):
        TIp, TJp = grid(p, TI, TJ, T2, F2)
        for tm in range((nb * TIp * TJp + 255) // 256):
            want |= {(p, tm, tn) for tn in range(tiles_n)}
    assert len(got) == len(set(got)) and set(got) == want


def test_bench_shape_counts():
    # B = 32, T1 = 499, F1 = 39: the b = 2 patterns go from 157 row tiles to 141, (2, 2) to 140
    T2, F2, TI, TJ = 249, 19, 125, 10
    tiles = {p: (32 * grid(p, TI, TJ, T2, F2)[0] * grid(p, TI, TJ, T2, F2)[1] + 255) // 256 for p in range(9)}
    assert tiles == {0: 157, 1: 157, 2: 141, 3: 157, 4: 157, 5: 141, 6: 155, 7: 155, 8: 140}


def test_even_shapes_keep_the_full_list_order():
    # even T2 and F2: every pattern has all rows, and a group's list is (tm, pattern, tn) in the group's own order
    nb, T1, F1, tiles_n = 40, 21, 13, 2                       # T2 = 10, F2 = 6
    T2, F2 = (T1 - 1) // 2, (F1 - 1) // 2
    TI, TJ = (T2 + 1) // 2, (F2 + 1) // 2
    got = tile_list(nb, TI, TJ, T2, F2, tiles_n)
    tiles_m = (nb * TI * TJ + 255) // 256
    assert tiles_m > 1
    want = []
    for pats in GROUPS:
        total = len(pats) * tiles_m * tiles_n
        per_xcd = ((total + 7) // 8 * 8) // 8
        for local in range(per_xcd * 8):
            tile = (local & 7) * per_xcd + (local >> 3)
            if tile < total:
                want.append((pats[(tile // tiles_n) % len(pats)], tile // tiles_n // len(pats), tile % tiles_n))
    assert got == want
