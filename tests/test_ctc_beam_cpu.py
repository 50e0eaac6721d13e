"""CTC prefix beam search without a GPU: the float64 restatement (tests/ctc_beam_restatement.py) against brute force in the
exact regime, hand-made cases of pruning, the K cap, ties and length 0, and the argument checks of the C entries."""
import ctypes
import math
import os

import numpy as np
import pytest

from tests import ctc_beam_restatement as R

INF = math.inf


def exact(logits, blank=0, length=None, W=64):
    """The restatement with nothing pruned: every candidate, every prefix kept."""
    V = logits.shape[1]
    return R.beam_search(logits, blank, W, max_candidates=V - 1, token_min_logp=-INF, beam_prune_logp=-INF, n_best=W,
                         length=length)


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("blank", [0, 2])
def test_restatement_equals_brute_force_in_the_exact_regime(T, blank):
    rng = np.random.default_rng(100 * T + blank)
    x = (rng.standard_normal((T, 3)) * 2).astype(np.float32)
    bf = R.brute_force(x, blank)
    out, _ = exact(x, blank)
    # without pruning, zero-probability prefixes (an extension by the last token from pb = -inf) are kept too
    got = {seq: sc for seq, sc in out if sc > -INF}
    assert set(got) == set(bf)
    for seq, sc in bf.items():
        assert abs(got[seq] - sc) <= 1e-12, (seq, got[seq], sc)
    assert [s for _, s in out] == sorted((s for _, s in out), reverse=True)


def test_brute_force_collapses_by_the_ctc_rule():
    assert R.collapse([1, 0, 1], 0) == (1, 1)                   # a blank separates repeats
    assert R.collapse([1, 1, 0, 0, 2, 2], 0) == (1, 2)
    assert R.collapse([0, 0], 0) == ()


def test_length_zero_returns_the_empty_prefix():
    x = np.zeros((4, 5), dtype=np.float32)
    out, m = R.beam_search(x, 0, 8, n_best=8, length=0)
    assert out == [((), 0.0)]
    assert R.min_margin(m) == INF
    out, _ = R.beam_search(x, 0, 8, n_best=8, length=-3)      # clamped to 0
    assert out == [((), 0.0)]


def test_length_limits_the_frames_consumed():
    rng = np.random.default_rng(5)
    x = rng.standard_normal((6, 4)).astype(np.float32)
    a, _ = R.beam_search(x, 0, 16, n_best=4, length=3)
    b, _ = R.beam_search(x[:3], 0, 16, n_best=4)
    assert a == b
    c, _ = R.beam_search(x, 0, 16, n_best=4, length=60)       # clamped to T
    d, _ = R.beam_search(x, 0, 16, n_best=4)
    assert c == d


def logits_from_probs(p):
    return np.log(np.asarray(p, dtype=np.float64)).astype(np.float32)


def test_token_min_logp_drops_unlikely_tokens():
    # token 2 has p = 0.005 < e^-5 in every frame: it never enters C_t, so no hypothesis holds it
    x = logits_from_probs([[0.5, 0.495, 0.005]] * 3)
    out, _ = R.beam_search(x, 0, 64, n_best=64, beam_prune_logp=-INF)
    assert out and all(2 not in seq for seq, _ in out)
    out, _ = R.beam_search(x, 0, 64, n_best=64, token_min_logp=-INF, beam_prune_logp=-INF)
    assert any(2 in seq for seq, _ in out)


def test_max_candidates_caps_the_extensions():
    x = logits_from_probs([[0.1, 0.4, 0.3, 0.2]])
    out, m = R.beam_search(x, 0, 8, max_candidates=1, n_best=8, beam_prune_logp=-INF)
    assert [seq for seq, _ in out] == [(1,), ()]               # only the best non-blank token extends
    assert m["cand"] == pytest.approx(math.log(0.4) - math.log(0.3))
    out, _ = R.beam_search(x, 0, 8, max_candidates=2, n_best=8, beam_prune_logp=-INF)
    assert [seq for seq, _ in out] == [(1,), (2,), ()]


def test_beam_prune_logp_drops_far_hypotheses():
    x = logits_from_probs([[0.97, 0.02, 0.01]])
    out, m = R.beam_search(x, 0, 8, token_min_logp=-INF, beam_prune_logp=-4.0, n_best=8)
    # log(0.02 / 0.97) = -3.88 survives, log(0.01 / 0.97) = -4.57 does not
    assert [seq for seq, _ in out] == [(), (1,)]
    assert m["prune"] == pytest.approx(min(abs(math.log(0.02 / 0.97) + 4.0), abs(math.log(0.01 / 0.97) + 4.0)))


def test_keep_w_keeps_the_best():
    x = logits_from_probs([[0.1, 0.5, 0.25, 0.15]])
    out, m = R.beam_search(x, 0, 2, token_min_logp=-INF, beam_prune_logp=-INF, n_best=2)
    assert [seq for seq, _ in out] == [(1,), (2,)]
    assert m["cut"] == pytest.approx(math.log(0.25) - math.log(0.15))


def test_ties_go_to_the_origin_key():
    # uniform logits: every candidate of frame 0 ties.  The stay of the empty prefix (rank 0, token -1) comes first, then
    # the extensions in token order; the K cap keeps the lower ids.
    x = np.zeros((1, 5), dtype=np.float32)
    out, m = R.beam_search(x, 0, 8, max_candidates=3, token_min_logp=-INF, beam_prune_logp=-INF, n_best=8)
    assert [seq for seq, _ in out] == [(), (1,), (2,), (3,)]
    assert m["cand"] == 0.0 and m["order"] == 0.0             # the ties are reported
    out, _ = R.beam_search(x, 2, 3, max_candidates=4, token_min_logp=-INF, beam_prune_logp=-INF, n_best=3)
    assert [seq for seq, _ in out] == [(), (0,), (1,)]         # blank 2 is never a candidate; keep-W cuts by key


def test_merged_hypothesis_takes_the_smaller_origin_key():
    # frame 0 keeps (1,) at rank 0 and () at rank 1.  In frame 1, () extended by 1 merges into the stay of (1,): keys
    # (0, -1) and (1, 1) -> (0, -1).  Its score sums both paths: "1 <any of blank, 1>" and "<blank> 1".
    x = np.array([[0.0, 3.0], [0.0, 0.0]], dtype=np.float32)
    out, _ = R.beam_search(x, 0, 4, max_candidates=1, token_min_logp=-INF, beam_prune_logp=-INF, n_best=4)
    lp0 = R.log_softmax64(x[0])
    want = np.logaddexp(lp0[1], lp0[0] + math.log(0.5))
    assert out[0][0] == (1,) and out[0][1] == pytest.approx(want, abs=1e-12)


@pytest.fixture(scope="module")
def lib():
    from conformer_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


def test_beam_entries_validate_their_arguments_without_gpu(lib):
    """cfm_ctc_beam_decode_f32 refuses bad arguments with a negative status BEFORE any HIP call (so this runs without a GPU)."""
    buf = (ctypes.c_float * 4096)()
    a = (ctypes.addressof(buf) + 255) // 256 * 256
    B, T, V, W, K = 2, 7, 5, 8, 4
    need = lib.cfm_ctc_beam_workspace_bytes(B, T, W, K)
    assert need >= B * (1 + T * W) * 8
    assert lib.cfm_ctc_beam_workspace_bytes(B, T, 0, K) == 0
    assert lib.cfm_ctc_beam_workspace_bytes(B, T, 257, K) == 0
    assert lib.cfm_ctc_beam_workspace_bytes(B, T, W, 33) == 0
    # a valid call would launch: every case below breaks exactly one rule, the last one only the workspace size
    args = [a, None, B, T, V, 0, W, K, -5.0, -10.0, 1, a, need, a, a, a, a, None]

    def call(**kw):
        names = ["logits", "lengths", "B", "T", "V", "blank", "W", "K", "tmin", "prune", "N", "ws", "ws_bytes", "tokens",
                 "counts", "scores", "num_hyps", "stream"]
        v = list(args)
        for k, x in kw.items():
            v[names.index(k)] = x
        return lib.cfm_ctc_beam_decode_f32(*v)

    for name in ("logits", "ws", "tokens", "counts", "scores", "num_hyps"):
        assert call(**{name: None}) == -3, name
    assert call(W=0) < 0 and call(W=257) < 0
    assert call(K=0) < 0 and call(K=33) < 0
    assert call(N=W + 1) < 0 and call(N=0) < 0
    assert call(blank=-1) < 0 and call(blank=V) < 0
    assert call(V=1, blank=0) < 0
    assert call(B=0) < 0 and call(T=0) < 0
    assert call(tmin=math.nan) < 0 and call(prune=math.nan) < 0
    assert call(ws_bytes=need - 1) < 0
