"""The transducer without a GPU: the float64 restatement (tests/rnnt_restatement.py) against enumeration of every path and
against autograd of itself, the header as the open table discovers it, every refusal of conformer_hip3_rnnt.h through the built
library (the argument checks return before any HIP call, as in test_abi_open_cpu.py), the workspace layout, and the precondition
of the greedy-decode fixture the GPU test compares exactly."""
import ctypes
import math
import os
import re

import pytest
import torch

from conformer_amd import _lib
from tests import rnnt_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conformer_amd", "csrc")
HEADER = "conformer_hip3_rnnt.h"
ENTRIES = ("cfm3_rnnt_workspace_floats", "cfm3_rnnt_loss_fwd_f32", "cfm3_rnnt_loss_bwd_f32", "cfm3_rnnt_joint_fwd_f32",
           "cfm3_rnnt_joint_bwd_f32", "cfm3_rnnt_greedy_decide", "cfm3_rnnt_greedy_commit")


@pytest.fixture(scope="module")
def lib():
    from conformer_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


# (T, U1, V, blank, targets, in_len, tg_len): every lattice of T <= 4, U <= 3 is small enough to enumerate
SMALL = [
    (4, 4, 5, 0, [1, 2, 3], 4, 3),
    (4, 4, 5, 0, [1, 0, 3], 4, 3),            # a label equal to blank
    (4, 4, 5, 4, [4, 4, 1], 3, 3),            # blank = V - 1, two labels equal to it, in_len < T
    (4, 4, 5, 0, [1, 2, 3], 4, 0),            # tg_len = 0: blanks only
    (3, 3, 4, 2, [1, 3], 1, 2),               # one frame
    (4, 3, 6, 1, [9, -3], 9, 7),              # everything clamps: labels to V - 1 and 0, in_len to T, tg_len to U1 - 1
    (1, 1, 3, 0, [], 1, 0),                   # U1 = 1
]


@pytest.mark.parametrize("case", SMALL)
def test_restatement_equals_enumeration_and_autograd(case):
    T, U1, V, blank, targets, in_len, tg_len = case
    g = torch.Generator().manual_seed(T * 100 + U1 * 10 + V)
    x = torch.randn(1, T, U1, V, generator=g, dtype=torch.float64)
    tg = torch.tensor([targets + [0] * (U1 - 1 - len(targets))], dtype=torch.int64) if U1 > 1 else None
    nll, grad, terms = R.loss_and_grad(x, tg, [in_len], [tg_len], blank)
    Tb, Ub, y = R.geometry(T, U1, V, targets, in_len, tg_len)
    assert Tb == min(in_len, T) and Ub == min(tg_len, U1 - 1)
    lp = torch.log_softmax(x[0], -1)
    ll = R.ll_by_enumeration(lp.tolist(), y, Tb, Ub, blank)
    assert abs(float(nll[0]) + ll) <= 1e-13 * max(1.0, abs(ll))
    xa = x[0].clone().requires_grad_(True)
    (ga,) = torch.autograd.grad(-R.ll_autograd(xa, y, Tb, Ub, blank), xa)
    assert float((grad[0] - ga).abs().max()) <= 1e-14
    assert float(grad[0].sum(-1).abs().max()) <= 1e-14                          # gamma == eb + el in every cell
    assert float(grad[0, Tb:].abs().max() if Tb < T else 0.0) == 0.0 and float(grad[0, :, Ub + 1:].abs().sum()) == 0.0
    assert float((terms[0] - grad[0].abs()).min()) >= -1e-15                    # the terms bound what they sum to


def test_restatement_dead_utterance_and_batch():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 3, 4, generator=g, dtype=torch.float64)
    tg = torch.tensor([[1, 2], [3, 1]])
    nll, grad, terms = R.loss_and_grad(x, tg, [0, 3], [2, 1], 0)
    assert float(nll[0]) == math.inf and float(grad[0].abs().max()) == 0.0 and float(terms[0].abs().max()) == 0.0
    assert math.isfinite(float(nll[1])) and float(grad[1].abs().max()) > 0


def test_the_header_is_discovered():
    path = os.path.join(CSRC, HEADER)
    assert path in _lib.OPEN_HEADERS and _lib.OPEN_CONSTANTS[HEADER] == {"CFM3_RNNT_MAX_U1": 1024}
    assert _lib.OPEN_CONSTANTS[HEADER]["CFM3_RNNT_MAX_U1"] >= _lib.CONSTANTS["CFM_CTC_MAX_TARGET"] + 1
    assert tuple(_lib.OPEN[path].signatures) == ENTRIES and all(n.startswith("cfm3_") for n in ENTRIES)
    src = open(os.path.join(CSRC, "rnnt.hip")).read()
    found = dict(re.findall(r'extern\s+"C"[^;{()]*?\b(cfm3_\w+)\s*\(([^()]*)\)\s*\{', src))
    assert set(found) == set(ENTRIES)
    for name, args in found.items():
        assert len(args.split(",")) == len(_lib.OPEN_ENTRIES[name][1]) == len(_lib.OPEN_PARAMS[name]), name
    E, P = _lib.OPEN_ENTRIES, _lib.OPEN_PARAMS
    assert E["cfm3_rnnt_workspace_floats"] == (ctypes.c_int64, [ctypes.c_int] * 3)
    assert P["cfm3_rnnt_loss_fwd_f32"] == ["logits", "targets", "in_len", "tg_len", "B", "T", "U1", "V", "blank", "workspace", "nll",
                                           "stream"]
    assert P["cfm3_rnnt_loss_bwd_f32"] == P["cfm3_rnnt_loss_fwd_f32"][:10] + ["weight", "dlogits", "stream"]
    res, args = E["cfm3_rnnt_loss_fwd_f32"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3    # double* nll: a pointer
    assert E["cfm3_rnnt_loss_bwd_f32"][1] == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 4
    assert P["cfm3_rnnt_joint_fwd_f32"] == ["e", "p", "frames", "h", "B", "Te", "T", "U1", "J", "stream"]
    assert E["cfm3_rnnt_joint_fwd_f32"][1] == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    assert P["cfm3_rnnt_joint_bwd_f32"] == ["h", "dh", "de", "dp", "B", "T", "U1", "J", "stream"]
    assert P["cfm3_rnnt_greedy_decide"][2:7] == ["B", "V", "T", "blank", "max_symbols"]
    assert E["cfm3_rnnt_greedy_decide"][1] == [ctypes.c_void_p] * 2 + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 8
    assert E["cfm3_rnnt_greedy_commit"][1] == [ctypes.c_void_p] * 5 + [ctypes.c_int] * 4 + [ctypes.c_void_p] * 2
    # the closed tables did not move
    assert (len(_lib.ENTRIES), len(_lib.EXTRA_ENTRIES)) == (162, 4) and _lib.ABI_VERSION == 4
    from conformer_amd import ops
    assert ops.RNNT_MAX_U1 == 1024


def test_workspace_floats(lib):
    """float64 {alpha (n), beta (n), ll (B)}, then fp32 {lse (n), lpb (n), lpl (n)}, n = B T U1: as the header states"""
    ws = lib.cfm3_rnnt_workspace_floats
    for B, T, U1 in [(1, 1, 1), (3, 37, 12), (32, 249, 51), (1, 5, 1024), (2, 65, 3), (7, 1, 129)]:
        n = B * T * U1
        assert ws(B, T, U1) == 2 * (n + n + B) + n + n + n, (B, T, U1)
    for bad in ((0, 8, 3), (2, 0, 3), (2, 8, 0), (-1, 8, 3), (2, 8, 1025), (1 << 20, 1 << 12, 2), (1 << 16, 1 << 16, 1)):
        assert ws(*bad) == -1, bad


def test_refusals_before_any_hip_call(lib):
    buf = (ctypes.c_double * 65536)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    NULL, SHAPE, UNSUPPORTED, ALIGN = (_lib.CONSTANTS[k] for k in ("CFM_ERR_NULL", "CFM_ERR_BAD_SHAPE", "CFM_ERR_UNSUPPORTED",
                                                                   "CFM_ERR_ALIGN"))
    assert 0 < lib.cfm3_rnnt_workspace_floats(2, 8, 3) * 4 < 65536 * 8 - 16

    def call(entry, base, **kw):
        args = list(base)
        for k, v in kw.items():
            args[int(k[1:])] = v
        return entry(*args)

    # logits, targets, in_len, tg_len, B, T, U1, V, blank, workspace, nll | (weight, dlogits), stream
    fwd = (lib.cfm3_rnnt_loss_fwd_f32, [a, a, a, a, 2, 8, 3, 5, 0, a, a, None])
    bwd = (lib.cfm3_rnnt_loss_bwd_f32, [a, a, a, a, 2, 8, 3, 5, 0, a, a, a, None])
    for entry, good in (fwd, bwd):
        for i in (0, 1, 2, 3, 9, 10) + ((11,) if len(good) == 13 else ()):
            assert call(entry, good, **{f"a{i}": None}) == NULL, i
        for i in (4, 5, 6, 7):                                              # B, T, U1, V
            assert call(entry, good, **{f"a{i}": 0}) == SHAPE, i
            assert call(entry, good, **{f"a{i}": -1}) == SHAPE, i
        assert call(entry, good, a8=-1) == SHAPE and call(entry, good, a8=5) == SHAPE
        assert call(entry, good, a6=1025) == UNSUPPORTED                    # U1 above CFM3_RNNT_MAX_U1
        assert call(entry, good, a4=1 << 20, a5=1 << 12) == UNSUPPORTED     # B T U1 beyond 2^31 - 1
        assert call(entry, good, a9=a + 4) == ALIGN                         # a misaligned workspace
        # the order: NULL, shape, the limits, the alignment
        assert call(entry, good, a0=None, a4=0) == NULL and call(entry, good, a4=0, a6=1025) == SHAPE
        assert call(entry, good, a6=1025, a9=a + 4) == UNSUPPORTED
    assert call(*fwd, a10=a + 4) == ALIGN                                   # a misaligned nll
    # joint forward: e, p, frames, h, B, Te, T, U1, J, stream (frames may be null)
    jf = (lib.cfm3_rnnt_joint_fwd_f32, [a, a, a, a, 2, 5, 5, 4, 8, None])
    for i in (0, 1, 3):
        assert call(*jf, **{f"a{i}": None}) == NULL, i
    for i in (4, 5, 6, 7, 8):
        assert call(*jf, **{f"a{i}": 0}) == SHAPE, i
    assert call(*jf, a2=None, a6=6) == SHAPE                                # more rows than frames, and no frame pointer
    assert call(*jf, a4=1 << 20, a5=1 << 12, a6=1 << 12) == UNSUPPORTED and call(*jf, a0=None, a4=0) == NULL
    assert call(*jf, a7=1 << 16, a8=1 << 15) == UNSUPPORTED                # U1 J beyond 2^31 - 1
    # joint backward: h, dh, de, dp, B, T, U1, J, stream
    jb = (lib.cfm3_rnnt_joint_bwd_f32, [a, a, a, a, 2, 5, 4, 8, None])
    for i in (0, 1, 2, 3):
        assert call(*jb, **{f"a{i}": None}) == NULL, i
    for i in (4, 5, 6, 7):
        assert call(*jb, **{f"a{i}": 0}) == SHAPE, i
    assert call(*jb, a4=1 << 20, a6=1 << 12) == UNSUPPORTED and call(*jb, a4=1 << 20, a5=1 << 12) == UNSUPPORTED
    assert call(*jb, a6=1 << 16, a7=1 << 15) == UNSUPPORTED                # U1 J beyond 2^31 - 1
    # decide: logits, in_len, B, V, T, blank, max_symbols, tokens, frames, count, last, t, nsym, emit, stream
    dec = (lib.cfm3_rnnt_greedy_decide, [a, a, 3, 29, 23, 0, 2, a, a, a, a, a, a, a, None])
    for i in (0, 1, 7, 8, 9, 10, 11, 12, 13):
        assert call(*dec, **{f"a{i}": None}) == NULL, i
    for i in (2, 3, 4, 6):
        assert call(*dec, **{f"a{i}": 0}) == SHAPE, i
    assert call(*dec, a5=-1) == SHAPE and call(*dec, a5=29) == SHAPE
    assert call(*dec, a4=1 << 20, a6=1 << 12) == UNSUPPORTED and call(*dec, a0=None, a5=29) == NULL
    # commit: state_new, state_cur, emit, t, in_len, planes, B, H, T, active, stream
    com = (lib.cfm3_rnnt_greedy_commit, [a, a, a, a, a, 2, 3, 16, 23, a, None])
    for i in (0, 1, 2, 3, 4, 9):
        assert call(*com, **{f"a{i}": None}) == NULL, i
    for i in (5, 6, 7, 8):
        assert call(*com, **{f"a{i}": 0}) == SHAPE, i


def test_the_greedy_fixture_is_decided_by_a_margin():
    """What the GPU test compares exactly must not hang on a rounding: at every decision the float64 restatement visits, top-1
    minus top-2 logit is at least 1e-3.  An fp32 dot product over K <= 640 terms of order 1 is wrong by at most about
    K 2^-24 = 4e-5, more than 20 times less.  The fixture also has to hold what the test is about."""
    s = R.GREEDY_SHAPE
    assert max(s["d"], s["H"], s["J"]) <= 640
    ref = R.greedy_reference()
    margins = [m for r in ref for m in r[2]]
    assert len(margins) >= sum(min(n, s["T"]) for n in s["in_len"]) and min(margins) >= 1e-3, min(margins)
    assert ref[0][3] >= 1 and ref[1][3] >= 1                                # the cap of max_symbols cuts emission
    assert s["in_len"][1] < s["T"] and all(f < s["in_len"][1] for f in ref[1][1])
    assert ref[2][0] == [] and len(ref[2][2]) == s["T"]                     # the silent utterance emits nothing
    per_frame = [ref[0][1].count(t) for t in range(s["T"])]
    assert {0, 1, 2} <= set(per_frame) and max(per_frame) == s["max_symbols"]
    assert all(len(r[0]) <= s["T"] * s["max_symbols"] for r in ref)


def test_host_checks_refuse_cpu_tensors():
    from conformer_amd import ops
    from conformer_amd.evaluation import ConformerCriterion
    x = torch.zeros(1, 4, 3, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ConformerCriterion(0).rnnt_loss(x, torch.zeros(1, 2, dtype=torch.int64), torch.tensor([4]), torch.tensor([2]))
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        ops.rnnt_loss_forward(x, torch.zeros(1, 2, dtype=torch.int64), torch.tensor([4]), torch.tensor([2]))
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        ops.rnnt_joint_forward(torch.zeros(1, 4, 8), torch.zeros(1, 3, 8))
    from model.transducer import ConformerTransducer
    from model.modules.transducer import Joiner, Predictor
    m = ConformerTransducer(11, n_conformer_blocks=1, d_model=32, pred_hidden_dim=24, n_pred_layers=2, joint_dim=20)
    assert isinstance(m.predictor, Predictor) and isinstance(m.joiner, Joiner)
    from model.conformer import Conformer
    enc_keys = {k for k in Conformer(11, 80, 1, 32, 4, 31, 24, 1, 0.0).state_dict() if k.startswith("encoder.")}
    assert enc_keys == {k for k in m.state_dict() if k.startswith("encoder.")}
