"""Per-element softmax-mass probes of every 16-bit route of the attention forward (csrc/attention_mfma16.hip), with the fp32
kernels as the control group.  Inputs, reference and bound are those of tests/attention_probe.py: exact operands and 0/1 values
leave the one rounding of P as the only inexact step, so every output element -- the softmax mass of a known key set -- is held to
(u_t + F) * ref + floor on its own, where one lost key, a positional row off by one, a mask one key too wide or two keys exchanged
are tens to thousands of times outside (tests/test_attention_probe_cpu.py).  Each test runs both value patterns and asserts through
tests.util.Calls that the intended library entry ran; a failure names batch, query row, head, column and the column's keys."""
import pytest
import torch

from tests import attention_probe as AP
from tests.util import Calls

pytestmark = pytest.mark.gpu

CASES = list(AP.CASES.items())
IDS = [n for n, _ in CASES]
DT = pytest.mark.parametrize("dt", AP.DT16, ids=["bf16", "fp16"])
TABLE = pytest.mark.parametrize("name,case", CASES, ids=IDS)
F32 = torch.float32


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _report(route, name, dt, worst):
    print(f"probe {route} {name} {str(dt).replace('torch.', '')}: worst element at {worst:.3f} of the bound")


def _L(lengths, dev):
    return None if lengths is None else torch.tensor(lengths, dtype=torch.int64, device=dev)


# ---- full-utterance inference under autocast: fp32 or 16-bit q|k|v, fp32 or 16-bit context (no case of the table is excluded:
#      every d is a multiple of 8, the dh = 36, H = 4 case included)
@DT
@pytest.mark.parametrize("qkv16,ctx16", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["qkv32_ctx32", "qkv16_ctx32", "qkv32_ctx16", "qkv16_ctx16"])
@TABLE
def test_probe_inference_routes(dev, name, case, qkv16, ctx16, dt):
    from conformer_amd import ops
    B, T, H, dh, lengths = case
    entry = "cfm_relpos_attention_io16_mfma16_f32" if (qkv16 or ctx16) else "cfm_relpos_attention_mfma16_f32"
    worst = 0.0
    for pattern in AP.PATTERNS:
        op = AP.operands(B, T, H, dh, pattern)
        qkv, pos, u, v = AP.device_inputs(op, dev, dt if qkv16 else F32)
        with Calls("cfm_relpos_attention_io16_mfma16_f32", "cfm_relpos_attention_mfma16_f32",
                   "cfm_relpos_attention_fwd_f32") as seen, torch.autocast("cuda", dtype=dt):
            ctx = ops.relpos_attention(qkv, pos, u, v, _L(lengths, dev), H, for_gemm=ctx16)
        assert seen == {entry}, seen
        assert ctx.dtype == (dt if ctx16 else F32)
        worst = max(worst, AP.check(ctx, AP.reference(op, lengths), op, dt, ctx16, what=f"{entry} {name}"))
    _report(f"inference qkv16={int(qkv16)} ctx16={int(ctx16)}", name, dt, worst)


# ---- training forward under autocast: context and log-sum-exp
@DT
@TABLE
def test_probe_train_route(dev, name, case, dt):
    from conformer_amd import ops
    B, T, H, dh, lengths = case
    worst = worst_lse = 0.0
    for pattern in AP.PATTERNS:
        op = AP.operands(B, T, H, dh, pattern)
        qkv, pos, u, v = AP.device_inputs(op, dev)
        with Calls("cfm_relpos_attention_mfma16_f32", "cfm_relpos_attention_train_f32") as seen, torch.autocast("cuda", dtype=dt):
            ctx, lse = ops.relpos_attention_train(qkv, pos, u, v, _L(lengths, dev), H)
        assert seen == {"cfm_relpos_attention_mfma16_f32"}, seen
        worst = max(worst, AP.check(ctx, AP.reference(op, lengths), op, dt, what=f"train {name}"))
        worst_lse = max(worst_lse, AP.check_lse(lse, op, lengths, what=f"train {name}"))
    _report("train ctx", name, dt, worst)
    _report("train lse", name, dt, worst_lse)


def _rows_chunks(ops, dev, op, ends, dt, entry, keys_hint=None):
    """The streaming call sequence: chunk by chunk into one NaN-filled ctx, lengths == the chunk end.  After every call the rows
    of the chunk are checked and every row the stream has not reached is still NaN; earlier rows are left as they were."""
    import contextlib
    B, T, H, dh = op["B"], op["T"], op["H"], op["dh"]
    qkv, pos, u, v = AP.device_inputs(op, dev)
    ctx = torch.full((B, T, H * dh), float("nan"), device=dev)
    ref = AP.reference(op, None, ends)
    worst, start = 0.0, 0
    for e in ends:
        before = ctx[:, :start].clone()
        L = torch.full((B,), e, dtype=torch.int64, device=dev)
        with Calls("cfm_relpos_attention_rows_mfma16_f32", "cfm_relpos_attention_rows_f32") as seen, \
                (torch.autocast("cuda", dtype=dt) if dt != F32 else contextlib.nullcontext()):
            ops.relpos_attention_rows(qkv, pos, u, v, L, H, start, e - start, ctx, keys_hint=keys_hint)
        assert seen == {entry}, seen
        assert torch.isnan(ctx[:, e:]).all(), f"rows >= {e} written by the chunk [{start}, {e})"
        assert torch.equal(ctx[:, :start], before), f"rows < {start} rewritten by the chunk [{start}, {e})"
        worst = max(worst, AP.check(ctx, ref, op, dt, rows=(start, e), what=f"{entry} T={T} chunk [{start}, {e})"))
        start = e
    return worst


# ---- streaming rows form under autocast.  The table's geometries with lengths == the chunk end, as the streaming path calls it
#      (so its own lengths column, the length-0 utterance included, does not apply: that case is the plain T = 40, dh = 8 geometry)
@DT
@TABLE
def test_probe_rows_route(dev, name, case, dt):
    from conformer_amd import ops
    B, T, H, dh, _ = case
    worst = 0.0
    for pattern in AP.PATTERNS:
        op = AP.operands(B, T, H, dh, pattern)
        worst = max(worst, _rows_chunks(ops, dev, op, AP.CHUNK_ENDS[T], dt, "cfm_relpos_attention_rows_mfma16_f32"))
    _report("rows", name, dt, worst)


# ---- control group: the fp32 kernels, already held at 2e-6, against the same probes with F alone.  If they fail, the probe is wrong.
@TABLE
def test_probe_control_fp32_forward_and_train(dev, name, case):
    from conformer_amd import _lib, ops
    B, T, H, dh, lengths = case
    lib = _lib.load()
    worst = worst_lse = 0.0
    for pattern in AP.PATTERNS:
        op = AP.operands(B, T, H, dh, pattern)
        qkv, pos, u, v = AP.device_inputs(op, dev)
        ref = AP.reference(op, lengths)
        prev = lib.cfm_debug_set_attention_waves(0)
        try:
            for nw in (4, 8, 9):
                lib.cfm_debug_set_attention_waves(nw)
                with Calls("cfm_relpos_attention_fwd_f32") as seen:
                    ctx = ops.relpos_attention(qkv, pos, u, v, _L(lengths, dev), H)
                assert seen == {"cfm_relpos_attention_fwd_f32"}
                worst = max(worst, AP.check(ctx, ref, op, F32, what=f"fp32 forward, waves {nw}, {name}"))
        finally:
            lib.cfm_debug_set_attention_waves(prev)
        with Calls("cfm_relpos_attention_train_f32") as seen:
            ctx, lse = ops.relpos_attention_train(qkv, pos, u, v, _L(lengths, dev), H)
        assert seen == {"cfm_relpos_attention_train_f32"}
        worst = max(worst, AP.check(ctx, ref, op, F32, what=f"fp32 train {name}"))
        worst_lse = max(worst_lse, AP.check_lse(lse, op, lengths, what=f"fp32 train {name}"))
    _report("control fp32 forward/train ctx", name, F32, worst)
    _report("control fp32 train lse", name, F32, worst_lse)


@TABLE
def test_probe_control_fp32_rows(dev, name, case):
    from conformer_amd import ops
    B, T, H, dh, _ = case
    worst = 0.0
    for pattern in AP.PATTERNS:
        op = AP.operands(B, T, H, dh, pattern)
        worst = max(worst, _rows_chunks(ops, dev, op, AP.CHUNK_ENDS[T], F32, "cfm_relpos_attention_rows_f32", keys_hint=1))
    _report("control fp32 rows", name, F32, worst)


def test_probe_control_fp32_rows_key_split(dev):
    from conformer_amd import ops
    B, T, H, dh = AP.SPLIT_CASE
    ends = AP.CHUNK_ENDS[T]
    assert all(ops._key_split(B, H, e - s, T, None) == 2 for s, e in zip([0] + ends, ends))
    worst = 0.0
    for pattern in AP.PATTERNS:
        op = AP.operands(B, T, H, dh, pattern)
        worst = max(worst, _rows_chunks(ops, dev, op, ends, F32, "cfm_relpos_attention_rows_f32"))
    _report("control fp32 rows, 2 key slices", f"T={T}", F32, worst)


def test_probe_control_fp32_slots(dev):
    """Ragged q_begin / q_count on the T = 300 case: slot b's rows against its keys < lengths[b], compact output rows."""
    from conformer_amd import ops
    B, T, H, dh, _ = AP.CASES["three_blocks_last_partial"]
    qb, qc = [33, 190], [31, 67]
    lengths = tuple(b + c for b, c in zip(qb, qc))
    worst = 0.0
    for pattern in AP.PATTERNS:
        op = AP.operands(B, T, H, dh, pattern)
        qkv, pos, u, v = AP.device_inputs(op, dev)
        ref = AP.reference(op, lengths)
        with Calls("cfm_relpos_attention_slots_f32") as seen:
            ctx = ops.relpos_attention_slots(qkv, pos, u, v, _L(lengths, dev), H, _L(qb, dev), _L(qc, dev), max(qc), keys_hint=1)
        assert seen == {"cfm_relpos_attention_slots_f32"}
        got = ref.clone()                                  # the compact rows put back at their cache rows; the rest is not under test
        for b in range(B):
            got[b, qb[b]:qb[b] + qc[b]] = ctx[b, :qc[b]].double().cpu()
            assert torch.all(ctx[b, qc[b]:] == 0.0)
        worst = max(worst, AP.check(got, ref, op, F32, what="fp32 slots"))
    _report("control fp32 slots", "T=300", F32, worst)
