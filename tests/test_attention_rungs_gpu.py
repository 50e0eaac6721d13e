"""Every rung of the head-dimension ladder (attn_tile::for_head_dim, csrc/attention_tile_f32.h) through the fp32 attention entries.

dh in {8, 16, 32, 40, 64} <-> (NC, ND) in {(1,1), (2,1), (4,1), (5,2), (8,2)}: each value is the largest head dimension of its rung,
so a ladder that sends it one rung too low drops head dims from the scores or the output.  B = 1, H = 2, T = 40: two key tiles with
a ragged last one, query rows in two waves.

What other files already hold, and what is therefore NOT repeated here:
  * full entry:   test_ops_gpu.ATT_CASES has every rung (dh 8, 16, 32, 36, 64) but dh = 40 itself, T = 40 only for dh = 8, and more
                  than 128 rows only for dh 32 / 36 / 64.  Here: T = 40 for the other four, T = 160 (the launcher picks the 8-wave
                  form itself) at dh = 40.
  * slots entry:  test_stream_slots_gpu.test_attention_slots_vs_float64 runs all five values with 4 and 8 waves forced, with and
                  without the key split.  Here only q_max = 160 > 128 at dh = 40: the launcher's own 8-wave choice.
  * rows entry:   dh = 16 (test_streaming_gpu) and the probe table's geometries.  Here all five.
  * train entry:  the probe table and dh = 64 (test_dropout_sites_gpu).  Here all five, context and log-sum-exp.
  * window entry: test_window_gpu runs dh 16, 36, 64 with left = 32.  Here 8, 32, 40, left = 32, a stream position past the ring.
References and tolerances are those of the entry's existing test: the float64 oracle at 2e-5 (test_ops_gpu.TOL) for the full and
train contexts, |lse - ref| < 2.5e-5 (test_attention_bwd_gpu, f32), the float64 row restatements at 2e-6 for slots and window
(test_stream_slots_gpu, test_window_gpu), 2e-6 for the rows entry (test_streaming_gpu).
"""
import math

import pytest
import torch

from oracle import conformer_oracle as O
from tests import test_stream_slots_gpu as S
from tests import test_window_gpu as W
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
RUNGS = [8, 16, 32, 40, 64]
H = 2


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_cache = {}


def _case(T, dh):
    """Seeded inputs of one (T, dh) on the CPU, the float64 context (1, T, d) and log-sum-exp (1, H, T): computed once, shared"""
    if (T, dh) not in _cache:
        d = H * dh
        g = torch.Generator().manual_seed(100 * T + dh)
        qkv = torch.randn(1, T, 3 * d, generator=g)
        pos = torch.randn(2 * T - 1, d, generator=g) * 0.5
        u, v = torch.randn(H, dh, generator=g) * 0.3, torch.randn(H, dh, generator=g) * 0.3
        q, k, vv = (t.reshape(1, T, H, dh).double() for t in qkv.split(d, dim=-1))
        pp = pos.double().view(2 * T - 1, H, dh)
        ref = O.relpos_attention_core(q, k, vv, pp, u.double(), v.double(), None)
        # the oracle's scores once more, for the log-sum-exp it does not return
        content = torch.einsum("bihc,bkhc->bhik", q + u.double(), k)
        band = torch.einsum("bihc,jhc->bhij", q + v.double(), pp)
        j = (T - 1) - (torch.arange(T)[:, None] - torch.arange(T)[None, :])
        lse = torch.logsumexp((content + band.gather(-1, j.expand(1, H, T, T))) / math.sqrt(dh), dim=-1)
        _cache[(T, dh)] = (qkv, pos, u, v, ref, lse)
    return _cache[(T, dh)]


def _on(dev, *ts):
    return [t.to(dev) for t in ts]


@pytest.mark.parametrize("T,dh", [(40, 16), (40, 32), (40, 40), (40, 64), (160, 40)])
def test_full_entry(dev, T, dh):
    from conformer_amd import ops
    qkv, pos, u, v, ref, _ = _case(T, dh)
    ctx = ops.relpos_attention(*_on(dev, qkv, pos, u, v), None, H)
    err = rel_l2(ctx, ref)
    print(f"full T={T} dh={dh}: {err:.3g}")
    assert err < 2e-5


@pytest.mark.parametrize("dh", RUNGS)
def test_train_entry(dev, dh):
    from conformer_amd import ops
    T = 40
    qkv, pos, u, v, ref, lse_ref = _case(T, dh)
    ctx, lse = ops.relpos_attention_train(*_on(dev, qkv, pos, u, v), torch.tensor([T], device=dev), H)
    err, lerr = rel_l2(ctx, ref), float((lse.double().cpu() - lse_ref).abs().max())
    print(f"train dh={dh}: ctx {err:.3g} lse {lerr:.3g}")
    assert err < 2e-5
    assert lerr < 2.5e-5


@pytest.mark.parametrize("dh", RUNGS)
def test_rows_entry(dev, dh):
    """rows 3 .. 39 of the cache (37 rows: two waves, counted from the first row) against all 40 keys; the others stay untouched"""
    from conformer_amd import ops
    T, q_begin, q_count = 40, 3, 37
    qkv, pos, u, v, ref, _ = _case(T, dh)
    ctx = torch.full((1, T, H * dh), float("nan"), device=dev)
    ops.relpos_attention_rows(*_on(dev, qkv, pos, u, v), torch.tensor([T], device=dev), H, q_begin, q_count, ctx, keys_hint=1)
    err = rel_l2(ctx[:, q_begin:], ref[:, q_begin:])
    print(f"rows dh={dh}: {err:.3g}")
    assert err < 2e-6
    assert torch.isnan(ctx[:, :q_begin]).all()


def test_slots_entry_more_than_128_rows(dev):
    """q_max = 160 without a key split: the launcher itself picks 8 waves.  Slot 0 fills every compact row, slot 1 only 131."""
    from conformer_amd import ops
    T, dh, q_max = 160, 40, 160
    qkv, pos, u, v = S._inputs(2, T, H, dh, dev, seed=5)
    qb, qc = [0, 20], [160, 131]
    L = [b + c for b, c in zip(qb, qc)]
    t = lambda x: torch.tensor(x, dtype=torch.int64, device=dev)
    with torch.no_grad():
        got = ops.relpos_attention_slots(qkv, pos, u, v, t(L), H, t(qb), t(qc), q_max, keys_hint=1).cpu()
    for b in range(2):
        assert torch.all(got[b, qc[b]:] == 0.0), b
        err = rel_l2(got[b, :qc[b]], S._restate(qkv, pos, u, v, H, b, range(qb[b], qb[b] + qc[b]), L[b]))
        print(f"slots slot {b}: {err:.3g}")
        assert err < 2e-6, (b, err)


@pytest.mark.parametrize("dh", [8, 32, 40])
def test_window_entry(dev, dh):
    """left = 32, 40 rows from stream position 70: R = 96, so the window's frames 38 .. 109 wrap the ring (109 mod 96 = 13)"""
    q_max, left, qb, qc = 40, 32, [70], [40]
    R, P = 32 * ((left + q_max + 31) // 32), max(left + 1, q_max)
    lin, pos, u, v = W._inputs(1, qb[0] + qc[0], H, dh, P, seed=dh)
    got = W._window(W._ring(lin, [qb[0] + qc[0]], R), pos, u, v, H, qb, qc, q_max, left, dev)
    err = rel_l2(got[0], W._restate(lin, pos, u, v, H, 0, qb[0], qc[0], left))
    print(f"window dh={dh}: {err:.3g}")
    assert torch.isfinite(got).all() and err < 2e-6
