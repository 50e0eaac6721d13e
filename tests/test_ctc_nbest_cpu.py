"""The n-best CTC scores and the MWER risk without a GPU: the float64 restatement against F.ctc_loss, the closed-form weights
against autograd, the header as the open table discovers it, and every refusal of conformer_hip3_ctc_nbest.h through the built
library (the argument checks return before any HIP call, as in test_abi_open_cpu.py)."""
import ctypes
import math
import os
import re

import pytest
import torch

from conformer_amd import _lib
from tests import ctc_nbest_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conformer_amd", "csrc")
HEADER = "conformer_hip3_ctc_nbest.h"
ENTRIES = ("cfm3_ctc_nbest_workspace_floats", "cfm3_ctc_nbest_score_f32", "cfm3_ctc_nbest_grad_f32", "cfm3_mwer_risk_f32")


@pytest.fixture(scope="module")
def lib():
    from conformer_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(11)
    logits = torch.randn(3, 37, 29, generator=g, dtype=torch.float64)
    hyps, hyp_len, in_len = R.hand_built(29)
    ll, dll = R.scores(logits, hyps, hyp_len, in_len, 0)
    return logits, hyps, hyp_len, in_len, ll, dll


def test_restatement_agrees_with_double_ctc_loss(case):
    logits, hyps, hyp_len, in_len, ll, dll = case
    ref = R.ll_ctc_loss(logits, hyps, hyp_len, in_len, 0)
    assert torch.equal(torch.isfinite(ll), torch.isfinite(ref))
    fin = torch.isfinite(ref)
    assert fin.sum() == 10 and not fin[1, 3] and not fin[2, 1]              # the unused row and the infeasible one
    assert float((ll[fin] - ref[fin]).abs().max()) <= 1e-10
    assert ll[2, 2] < 0 and float(dll[2, 1].abs().max()) == 0.0            # the empty row at one frame; the infeasible one
    # the gradient is the one autograd takes of F.ctc_loss
    x = logits.clone().requires_grad_(True)
    lp = x.log_softmax(-1)
    nll = torch.nn.functional.ctc_loss(lp[0, :, None, :], torch.tensor([hyps[0][0]]), torch.tensor([37]), torch.tensor([4]),
                                       blank=0, reduction="none")
    (g,) = torch.autograd.grad(-nll[0], x)
    assert float((g[0] - dll[0, 0]).abs().max()) <= 1e-10
    assert float(dll[1, 0, 20:].abs().max()) == 0.0                         # behind in_len


def test_closed_form_weights_equal_autograd(case):
    ll, hyp_len = case[4], case[2]
    errors = [[3, 0, 1, 6], [2, 5, 4, 0], [1, 2, 1, 0]]
    loss, g, r, _ = R.risk_weights(ll, errors, hyp_len)
    w = R.closed_form_weights(ll, errors, hyp_len)
    assert float((g - w).abs().max()) <= 1e-14
    assert float(w.abs().max()) > 1e-3
    assert float(w.sum(1).abs().max()) <= 1e-15                             # the weights of a list sum to zero
    assert float(w[1, 3]) == 0.0 and float(w[2, 1]) == 0.0                  # dead rows
    assert abs(float(loss) - float(r.mean())) <= 1e-15
    one = [[0, -1, -1, -1]] * 3                                             # a single live row: no risk, no weight
    loss1, g1, r1, _ = R.risk_weights(ll, errors, one)
    assert float(loss1) == 0.0 and float(g1.abs().max()) == 0.0


def test_a_constant_added_to_every_error_changes_nothing(case):
    ll, hyp_len = case[4], case[2]
    errors = [[3, 0, 1, 6], [2, 5, 4, 0], [1, 2, 1, 0]]
    shifted = [[e + 7 for e in row] for row in errors]
    a, b = R.risk_weights(ll, errors, hyp_len), R.risk_weights(ll, shifted, hyp_len)
    assert abs(float(a[0]) - float(b[0])) <= 1e-13
    assert float((a[1] - b[1]).abs().max()) <= 1e-14
    assert float((R.closed_form_weights(ll, errors, hyp_len) - R.closed_form_weights(ll, shifted, hyp_len)).abs().max()) <= 1e-14


def test_the_header_is_discovered():
    path = os.path.join(CSRC, HEADER)
    assert path in _lib.OPEN_HEADERS and _lib.OPEN_CONSTANTS[HEADER] == {"CFM3_CTC_NBEST_MAX": 64}
    assert tuple(_lib.OPEN[path].signatures) == ENTRIES and all(n.startswith("cfm3_") for n in ENTRIES)
    src = open(os.path.join(CSRC, "ctc_nbest.hip")).read()
    found = dict(re.findall(r'extern\s+"C"[^;{()]*?\b(cfm3_\w+)\s*\(([^()]*)\)\s*\{', src))
    assert set(found) == set(ENTRIES)
    for name, args in found.items():
        assert len(args.split(",")) == len(_lib.OPEN_ENTRIES[name][1]) == len(_lib.OPEN_PARAMS[name]), name
    assert _lib.OPEN_ENTRIES["cfm3_ctc_nbest_workspace_floats"][0] is ctypes.c_int64
    assert _lib.OPEN_PARAMS["cfm3_ctc_nbest_score_f32"][4:10] == ["B", "N", "T", "V", "Lmax", "blank"]
    assert _lib.OPEN_PARAMS["cfm3_ctc_nbest_grad_f32"][:11] == _lib.OPEN_PARAMS["cfm3_ctc_nbest_score_f32"][:11]
    assert _lib.OPEN_ENTRIES["cfm3_mwer_risk_f32"][1][5] is ctypes.c_float
    # the closed tables did not move
    assert (len(_lib.ENTRIES), len(_lib.EXTRA_ENTRIES)) == (162, 4)
    from conformer_amd import ops
    assert ops.CTC_NBEST_MAX == 64


def pairs(L):
    p = 1
    while 64 * p < L + 1:
        p *= 2
    return p


def test_workspace_floats(lib):
    ws = lib.cfm3_ctc_nbest_workspace_floats
    for B, N, T, L in [(1, 1, 1, 1), (3, 4, 37, 6), (2, 8, 64, 20), (64, 8, 249, 40), (1, 2, 133, 64), (1, 64, 5, 1023)]:
        frames, rows = B * T, B * N
        rt = rows * T
        assert ws(B, N, T, L) == 2 * (2 * rt + rows) + 2 * frames + rt * L + 2 * rt * 2 * 64 * pairs(L), (B, N, T, L)
    for bad in ((0, 4, 8, 3), (2, 0, 8, 3), (2, 4, 0, 3), (2, 4, 8, 0), (2, 65, 8, 3), (2, 4, 8, 1024), (-1, 4, 8, 3),
                (1 << 20, 4, 1 << 12, 3)):
        assert ws(*bad) == -1, bad
    # nothing of B N T V elements: at the shape of the memory test the workspace is a fraction of the expanded logits
    assert ws(2, 8, 64, 20) * 4 < 2 * 8 * 64 * 4096 * 4 // 8


def test_refusals_before_any_hip_call(lib):
    buf = (ctypes.c_double * 65536)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    NULL, SHAPE, UNSUPPORTED, ALIGN = (_lib.CONSTANTS[k] for k in ("CFM_ERR_NULL", "CFM_ERR_BAD_SHAPE", "CFM_ERR_UNSUPPORTED",
                                                                   "CFM_ERR_ALIGN"))
    assert 0 < lib.cfm3_ctc_nbest_workspace_floats(2, 4, 8, 3) * 4 < 65536 * 8 - 16

    def call(entry, base, **kw):
        args = list(base)
        for k, v in kw.items():
            args[int(k[1:])] = v
        return entry(*args)

    # logits, hyps, hyp_len, in_len, B, N, T, V, Lmax, blank, workspace, ll | (weight, dlogits), stream
    score = (lib.cfm3_ctc_nbest_score_f32, [a, a, a, a, 2, 4, 8, 5, 3, 0, a, a, None])
    grad = (lib.cfm3_ctc_nbest_grad_f32, [a, a, a, a, 2, 4, 8, 5, 3, 0, a, a, a, None])
    for entry, good in (score, grad):
        for i in (0, 1, 2, 3, 10, 11) + ((12,) if len(good) == 14 else ()):
            assert call(entry, good, **{f"a{i}": None}) == NULL, i
        for i in (4, 5, 6, 7, 8):                                           # B, N = 0, T, V, Lmax
            assert call(entry, good, **{f"a{i}": 0}) == SHAPE, i
        assert call(entry, good, a5=-1) == SHAPE
        assert call(entry, good, a9=-1) == SHAPE and call(entry, good, a9=5) == SHAPE
        assert call(entry, good, a5=65) == UNSUPPORTED                      # N above CFM3_CTC_NBEST_MAX
        assert call(entry, good, a8=1024) == UNSUPPORTED                    # Lmax above CFM_CTC_MAX_TARGET
        assert call(entry, good, a4=1 << 20, a6=1 << 12) == UNSUPPORTED
        assert call(entry, good, a10=a + 4) == ALIGN                        # a misaligned workspace
        # the order: NULL, shape, the limits, the alignment
        assert call(entry, good, a0=None, a5=0) == NULL and call(entry, good, a5=0, a8=1024) == SHAPE
        assert call(entry, good, a8=1024, a10=a + 4) == UNSUPPORTED
    assert call(*score, a11=a + 4) == ALIGN
    # V too large for LDS: (V + 2 * 64 * P) floats per frame against 64 KB.  The score entry has no such limit, and is not
    # called at that size here: it would launch.
    assert call(*grad, a7=16384 - 128 + 1) == UNSUPPORTED
    assert call(*grad, a7=20000, a10=a + 4) == ALIGN
    # loss: ll, errors, hyp_len, B, N, grad_scale, risk, loss, weight, stream
    risk = (lib.cfm3_mwer_risk_f32, [a, a, a, 2, 4, 1.0, a, a, a, None])
    for i in (0, 1, 2, 6, 7, 8):
        assert call(*risk, **{f"a{i}": None}) == NULL, i
    assert call(*risk, a3=0) == SHAPE and call(*risk, a4=0) == SHAPE and call(*risk, a4=65) == UNSUPPORTED
    assert call(*risk, a0=a + 4) == ALIGN and call(*risk, a0=None, a4=0) == NULL and call(*risk, a4=65, a0=a + 4) == UNSUPPORTED


def test_host_checks_refuse_cpu_tensors():
    from conformer_amd import decode
    from conformer_amd.evaluation import ConformerCriterion
    x = torch.zeros(1, 4, 5)
    tk, ct = torch.zeros(1, 2, 3, dtype=torch.int64), torch.zeros(1, 2, dtype=torch.int64)
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        decode.ctc_nbest_scores(x, tk, ct, 0, max_len=3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ConformerCriterion(0).mwer_loss(x, tk[:, 0], torch.tensor([4]), torch.tensor([3]), None)
    p = R.posterior(torch.tensor([[0.0, -math.inf, math.log(3.0)]], dtype=torch.float64), [[1, 1, 2]])
    assert torch.allclose(p, torch.tensor([[0.25, 0.0, 0.75]], dtype=torch.float64), atol=1e-15)
