"""The per-element probe bound of tests/attention_probe.py discriminates: a torch model of the 16-bit kernel's arithmetic (fp32
scores, fp32 exp, row sum from the unrounded probabilities, P rounded before P.V) stays inside the bound at every probe case, and
every structural fault injected into it -- one (row, key) pair lost, the positional index of one key tile off by one, a padding
mask that admits key L, two keys of a tile exchanged in P.V -- exceeds it at least 4x on some element, in bf16 and in fp16, while
the whole-tensor rel_l2 that the other 16-bit attention tests use stays under their 6e-3 bar for the local ones.  Also pins F, the
probe's allowance for the fp32 parts, to its measurement on the float64 / float32 reference.  No GPU."""
import math

import pytest
import torch

from tests import attention_probe as AP
from tests.util import rel_l2

CASES = list(AP.CASES.items())
IDS = [n for n, _ in CASES]


def test_F_is_the_reference_measurement_with_its_margin():
    measured = AP.measure_F()
    print(f"F measured {measured:.3e}, recorded {AP.F_MEASURED:.3e}, allowance {AP.F:.3e}")
    assert AP.F == AP.F_MARGIN * AP.F_MEASURED and AP.F_MARGIN == 8
    assert AP.F >= measured                                   # the allowance covers what the reference itself shows
    assert AP.F_MEASURED <= 2 * measured                      # and is this measurement, not a looser number
    assert AP.F < AP.U[torch.float16] / 8                     # F can never swallow the bound it sits beside


@pytest.mark.parametrize("name,case", CASES, ids=IDS)
def test_probe_scores_and_sets_restate_the_reference(name, case):
    """The helper's own scores / visibility / key sets give the reference's context and the exact operands give exact fp32 scores."""
    B, T, H, dh, lengths = case
    for pattern in AP.PATTERNS:
        op = AP.operands(B, T, H, dh, pattern)
        assert AP.n_set(op) == max(int((op["col"][:, 0] == c).sum()) for c in range(dh))
        variants = [(lengths, None)] + ([(None, AP.CHUNK_ENDS[T])] if lengths is None or min(lengths) > 0 else [])
        for L, ends in variants:
            s = AP.scores_log2(op) * math.log(2.0)
            if L is not None:
                s = torch.where((AP.lengths_tensor(L) <= 0)[:, None, None, None], torch.zeros_like(s), s)
            s = s.masked_fill(~AP.key_visible(op, L, ends), -math.inf)
            mine = torch.einsum("bhik,bkhc->bihc", torch.softmax(s, -1), op["v"]).reshape(B, T, H * dh)
            ref = AP.reference(op, L, ends)
            assert (mine - ref).abs().max() < 1e-14
            assert ((ref == 0) == (mine == 0)).all()
            assert abs(float(ref.sum()) - B * T * H) < 1e-9 * B * T * H           # every key in exactly one set: the masses of a row sum to 1
        unscaled32 = AP.scores_log2(op, torch.float32) / (torch.tensor(1 / math.sqrt(dh)) * torch.tensor(1.4426950408889634))
        unscaled64 = AP.scores_log2(op) / (1 / math.sqrt(dh) * 1.4426950408889634)
        assert (unscaled32.double() - unscaled64).abs().max() < 1e-5 and float(unscaled64.abs().max()) / math.sqrt(dh) < 6.0


@pytest.mark.parametrize("dt", AP.DT16, ids=["bf16", "fp16"])
@pytest.mark.parametrize("name,case", CASES, ids=IDS)
def test_clean_model_is_inside_the_bound(name, case, dt):
    B, T, H, dh, lengths = case
    worst = 0.0
    for pattern in AP.PATTERNS:
        op = AP.operands(B, T, H, dh, pattern)
        for ctx16 in (False, True):
            got = AP.kernel_model(op, lengths, dt, ctx16)
            worst = max(worst, AP.check(got, AP.reference(op, lengths), op, dt, ctx16, what=f"model {name} ctx16={ctx16}"))
        if lengths is None or min(lengths) > 0:
            ends = AP.CHUNK_ENDS[T]
            got = AP.kernel_model(op, None, dt, ends=ends)
            worst = max(worst, AP.check(got, AP.reference(op, None, ends), op, dt, what=f"model {name} chunked"))
    print(f"{name} {dt}: clean model at {worst:.3f} of the bound")
    assert 0.0 < worst <= 1.0 or T == 1                       # (T == 1: p == 1, nothing to round)


def _excess(op, lengths, dt, fault):
    got = AP.kernel_model(op, lengths, dt, fault=fault)
    if got is None:
        return None, None
    ref = AP.reference(op, lengths)
    frac, _ = AP.worst_fraction(got, ref, AP.bound(ref, dt, False, AP.n_set(op)))
    return frac, rel_l2(got, ref)


@pytest.mark.parametrize("dt", AP.DT16, ids=["bf16", "fp16"])
@pytest.mark.parametrize("fault", AP.FAULTS)
def test_every_fault_exceeds_the_bound_4x(fault, dt):
    """At every case where the fault exists, under the pattern that can see it (keys 5 and 13 share a column under pattern A at
    dh == 8: that is what pattern B is for)."""
    seen = 0
    for name, (B, T, H, dh, lengths) in CASES:
        for pattern in AP.PATTERNS:
            op = AP.operands(B, T, H, dh, pattern)
            frac, _ = _excess(op, lengths, dt, fault)
            if frac is None:
                continue
            blind = fault == "keys_exchanged" and int(op["col"][5, 0]) == int(op["col"][13, 0])
            print(f"{fault} {name} pattern {pattern} {dt}: {frac:.1f}x the bound" + (" (blind by construction)" if blind else ""))
            if blind:
                assert pattern == "A" and dh == 8
                continue
            seen += 1
            assert frac >= 4.0, (fault, name, pattern, frac)
    assert seen >= 8


@pytest.mark.parametrize("fault", ["dropped_pair", "keys_exchanged"])
def test_whole_tensor_rel_l2_is_blind_to_the_local_faults(fault):
    """The metric of the other 16-bit attention tests (rel_l2 < 6e-3 in bf16) passes the same faulty contexts that the per-element
    bound rejects, at the shapes of those tests (T >= 161)."""
    seen = 0
    for name, (B, T, H, dh, lengths) in CASES:
        if T < 161:
            continue
        for pattern in AP.PATTERNS:
            op = AP.operands(B, T, H, dh, pattern)
            frac, rl2 = _excess(op, lengths, torch.bfloat16, fault)
            print(f"{fault} {name} pattern {pattern}: rel_l2 {rl2:.2e}, {frac:.1f}x the per-element bound")
            assert rl2 < 6e-3 and frac >= 4.0
            seen += 1
    assert seen == 6


def test_check_names_the_failing_element():
    B, T, H, dh, lengths = AP.CASES["dh16_zero_fill_mask_in_tile"]
    op = AP.operands(B, T, H, dh, "A")
    got = AP.kernel_model(op, lengths, torch.bfloat16, fault="dropped_pair")
    with pytest.raises(AssertionError, match=r"batch 0 query row 48 head 0 column 8 \(keys \[8, 24, 40, 56, 72, 88\]\)"):
        AP.check(got, AP.reference(op, lengths), op, torch.bfloat16, what="dropped")
    lse = AP.reference_lse(op, lengths).clone()
    AP.check_lse(lse, op, lengths)
    lse[1, 0, 5] += 1e-4
    with pytest.raises(AssertionError, match="lse batch 1 head 0 query row 5"):
        AP.check_lse(lse, op, lengths)
