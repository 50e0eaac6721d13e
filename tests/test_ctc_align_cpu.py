"""CTC forced alignment, the parts that need no GPU: the float64 restatement against brute force on exhaustive small
cases, the word grouping of `conformer_amd.align`, and the argument checks of the two C entries (they return before any
HIP call)."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from tests import ctc_align_restatement as R

BLANK = 0


def grid_logits(rng, T, V, lo=-2, hi=2, scale=1.0):
    """integer multiples of `scale`: float64 sums are exact, so equal-score paths tie exactly"""
    return (rng.integers(lo, hi + 1, size=(T, V)) * scale).astype(np.float32)


TARGETS = [[], [1], [2], [1, 2], [1, 1], [2, 1], [1, 2, 1], [1, 1, 2], [1, 2, 2], [1, 1, 1], [1, 2, 3]]


@pytest.mark.parametrize("T", [1, 2, 3, 4, 5, 6])
def test_restatement_equals_brute_force(T):
    """Every target up to L = 3 (repeats, L = 0, T = L + repeats exactly, infeasible ones) on tie-rich grid logits and on
    real-valued ones: the same states, frame for frame."""
    rng = np.random.default_rng(100 + T)
    ties = 0
    for y in TARGETS:
        for trial in range(6):
            x = grid_logits(rng, T, 4) if trial < 4 else rng.standard_normal((T, 4)).astype(np.float32)
            got, want = R.viterbi(x, y, BLANK), R.brute_force(x, y, BLANK)
            if not R.feasible(T, y):
                assert got is None and want is None, (T, y)
                continue
            assert want is not None and R.valid_path(y, want)
            assert got is not None and got.tolist() == want.tolist(), (T, y, trial, got, want)
            if trial < 4:                       # is the maximum shared by another path?  (the tie rule is exercised)
                best = R.path_score(x, y, BLANK, want)
                n = sum(1 for s in itertools.product(range(2 * len(y) + 1), repeat=T)
                        if R.valid_path(y, np.asarray(s)) and R.path_score(x, y, BLANK, np.asarray(s)) == best)
                ties += n > 1
    if T >= 3:
        assert ties > 0


def test_tie_rule_by_hand():
    """All-zero logits: every path ties.  Read from the last frame backwards the state stays as high as it can: the path
    ends in the final blank and holds it, and every move is as small as the remaining frames allow."""
    x = np.zeros((5, 3), dtype=np.float32)
    assert R.viterbi(x, [1], BLANK).tolist() == [1, 2, 2, 2, 2]
    assert R.viterbi(x, [1, 2], BLANK).tolist() == [1, 3, 4, 4, 4]
    assert R.viterbi(x, [1, 1], BLANK).tolist() == [1, 2, 3, 4, 4]
    assert R.viterbi(x[:3], [1, 1], BLANK).tolist() == [1, 2, 3]            # T = L + repeats exactly
    assert R.viterbi(x[:2], [1, 1], BLANK) is None
    assert R.viterbi(x, [], BLANK).tolist() == [0] * 5
    assert R.viterbi(x[:0], [], BLANK) is None                              # T = 0 is infeasible even for L = 0


def test_outputs_of_the_restatement():
    x = np.log(np.array([[.6, .3, .1], [.2, .7, .1], [.1, .8, .1], [.5, .1, .4], [.1, .1, .8]], dtype=np.float64))
    r = R.align(x.astype(np.float32), [1, 2], BLANK)
    assert r.ok and r.states.tolist() == [0, 1, 1, 2, 3]
    assert r.frame_tokens.tolist() == [0, 1, 1, 0, 2] and r.frame_index.tolist() == [-1, 0, 0, -1, 1]
    assert r.token_start.tolist() == [1, 4] and r.token_end.tolist() == [3, 5]
    assert abs(r.token_score[0] - (np.log(.7) + np.log(.8)) / 2) < 1e-6 and abs(r.token_score[1] - np.log(.8)) < 1e-6
    assert abs(r.score - np.log(.6 * .7 * .8 * .5 * .8)) < 1e-6
    bad = R.align(x.astype(np.float32), [1, 1, 1], BLANK, length=4)
    assert not bad.ok and bad.score == -np.inf and bad.frame_tokens.tolist() == [-1] * 4
    assert bad.token_start.tolist() == [-1] * 3 and np.all(bad.token_score == -np.inf)


def test_raw_logits_and_log_probabilities_give_the_same_path():
    rng = np.random.default_rng(7)
    for T, L, V in [(12, 4, 5), (60, 20, 9), (200, 30, 6)]:
        x = (rng.standard_normal((T, V)) * 3).astype(np.float32)
        y = rng.integers(1, V, size=L).tolist()
        assert R.viterbi(x, y, BLANK).tolist() == R.viterbi(R.log_softmax64(x), y, BLANK).tolist()


# ---- word grouping ---------------------------------------------------------------------------------------------------------

VOCAB = ["<pad>", "a", "b", "c", "|", "<unk>", "ch"]


def _group(ids, frames_each=2, score=None):
    from conformer_amd.align import group_words
    starts = [3 + frames_each * k for k in range(len(ids))]
    ends = [s + frames_each for s in starts]
    scores = score or [-0.5] * len(ids)
    return group_words(ids, starts, ends, scores, VOCAB, 4, 0.04, frozenset({5}))


def test_word_grouping():
    w = _group([1, 2, 4, 3])
    assert [x.text for x in w] == ["ab", "c"]
    assert (w[0].start_frame, w[0].end_frame, w[1].start_frame, w[1].end_frame) == (3, 7, 9, 11)
    assert w[0].start == pytest.approx(0.12) and w[0].end == pytest.approx(0.28)
    assert [x.text for x in _group([4, 1, 4, 4, 2, 3, 4])] == ["a", "bc"]          # delimiters at the ends, doubled
    assert _group([]) == [] and _group([4]) == [] and _group([4, 4]) == []          # empty transcript
    assert [x.text for x in _group([1, 5, 2])] == ["ab"]                            # a skipped id adds no characters
    assert _group([5]) == []


def test_word_score_is_frame_weighted():
    from conformer_amd.align import group_words
    w = group_words([1, 2], [0, 1], [1, 4], [-1.0, -2.0], VOCAB, 4, 0.04)
    assert len(w) == 1 and w[0].score == pytest.approx((-1.0 * 1 + -2.0 * 3) / 4)
    assert (w[0].start_frame, w[0].end_frame) == (0, 4)


def test_aligner_tokenises_and_refuses_bad_targets():
    from conformer_amd.align import CTCAligner
    al = CTCAligner(VOCAB, 0, skip_ids=(5,))
    assert al.tokenize("ab c") == [1, 2, 4, 3]
    assert al.tokenize("chab") == [6, 1, 2]                                         # longest token first
    assert al.tokenize("") == []
    with pytest.raises(ValueError):
        al.tokenize("ax")
    with pytest.raises(ValueError):
        al._ids([1, 0])                                                             # the blank id
    with pytest.raises(ValueError):
        al._ids([1, 7])
    with pytest.raises(ValueError):
        CTCAligner(VOCAB, 9)


def test_aligner_from_decoder():
    from conformer_amd.align import CTCAligner
    from conformer_amd.decode import BeamCTCDecoder
    dec = BeamCTCDecoder(VOCAB, 0, skip_ids=(5,), delim_token="|")
    al = CTCAligner.from_decoder(dec)
    assert al.vocab == VOCAB and al.blank_id == 0 and al.delim_id == 4 and al.skip_ids == {5}
    assert al.frame_seconds == 0.04


def test_no_cpu_path():
    import torch
    from conformer_amd._lib import ConformerHipError
    from conformer_amd.align import ctc_forced_align
    with pytest.raises(ConformerHipError):
        ctc_forced_align(torch.zeros(1, 4, 3), torch.ones(1, 2, dtype=torch.int64), 0)


# ---- the C entries, without a GPU -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from conformer_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


def test_workspace_bytes(lib):
    assert lib.cfm_ctc_align_workspace_bytes(0, 10, 4) == 0
    assert lib.cfm_ctc_align_workspace_bytes(2, 0, 4) == 0
    assert lib.cfm_ctc_align_workspace_bytes(2, 10, 0) == 0
    assert lib.cfm_ctc_align_workspace_bytes(2, 16385, 4) == 0
    assert lib.cfm_ctc_align_workspace_bytes(2, 10, 4097) == 0
    assert lib.cfm_ctc_align_workspace_bytes(-1, 10, 4) == 0
    assert lib.cfm_ctc_align_workspace_bytes(1, 16384, 4096) > 0
    # 2 bits per (frame, state) over at least 2 Lmax + 1 states, and a float64 per frame
    for B, T, L in [(1, 1, 1), (32, 249, 60), (3, 100, 1023), (3, 100, 1024), (1, 16384, 2048)]:
        n = lib.cfm_ctc_align_workspace_bytes(B, T, L)
        assert n >= B * T * ((2 * L + 1 + 3) // 4 + 8), (B, T, L, n)
    assert lib.cfm_ctc_align_workspace_bytes(1, 100, 1023) < lib.cfm_ctc_align_workspace_bytes(1, 100, 1024)


def test_argument_validation_without_gpu(lib):
    buf = (ctypes.c_double * 4096)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    n = lib.cfm_ctc_align_workspace_bytes(2, 8, 3)
    assert 0 < n < 4096 * 8 - 16
    good = [a, a, None, None, 2, 8, 5, 3, 0, a, n, a, a, a, a, a, a, a, None]

    def call(**kw):
        args = list(good)
        for k, v in kw.items():
            args[int(k[1:])] = v
        return lib.cfm_ctc_align_f32(*args)

    for i in (0, 1, 9, 11, 12, 13, 14, 15, 16, 17):
        assert call(**{f"a{i}": None}) == -3, i                                    # NULL
    assert call(a4=0) == -1 and call(a5=0) == -1 and call(a6=1) == -1 and call(a7=0) == -1      # B, T, V, Lmax
    assert call(a8=-1) == -1 and call(a8=5) == -1                                   # blank_id outside [0,V)
    assert call(a5=16385) == -2 and call(a7=4097) == -2                             # beyond the limits
    assert call(a9=a + 8) < 0                                                       # misaligned workspace
    assert call(a10=n - 1) < 0                                                      # workspace too small
