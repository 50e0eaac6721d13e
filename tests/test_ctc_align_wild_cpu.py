"""Forced alignment with wildcards, the parts that need no GPU: tokenising with a wildcard token, the refusals, `group_words`
and the assembly of Segments from a hand-made Alignment, and the planted construction of tests/ctc_align_wild_fixture.py run
through the float64 restatement (which pins the fixture and the definition, not the kernel)."""
import math

import numpy as np
import pytest
import torch

from conformer_amd import align as A
from conformer_amd.align import Alignment, CTCAligner, Segment, Word, group_words
from tests import ctc_align_restatement as R
from tests import ctc_align_wild_fixture as F

W = A.WILDCARD
VOCAB = ["<pad>", "a", "b", "c", "d", "ab", "|", "<unk>"]          # ids: a 1, b 2, c 3, d 4, ab 5, | 6


def aligner(**kw):
    return CTCAligner(VOCAB, 0, skip_ids=(7,), **kw)


def test_the_wildcard_value():
    assert W == F.W == -2 and A.WILDCARD == -2


def test_tokenising_with_a_wildcard_token():
    al = aligner(wildcard_token="*", wildcard_penalty=0.5)
    assert al.tokenize("ab cd") == [5, 6, 3, 4]                                         # as ever
    assert al.tokenize("* ab cd * c *") == [W, 5, 6, 3, 4, W, 3, W]                     # delimiters beside a wildcard are dropped
    assert al.tokenize("ab*c") == [5, W, 3] and al.tokenize("ab | * | c") == [5, W, 3]
    assert al.tokenize("*") == [W] and al.tokenize("") == [] and al.tokenize(" * ") == [W]
    assert al.tokenize(" ab * c ") == [6, 5, W, 3, 6]                                   # the outer delimiters stay, as ever
    assert aligner().tokenize("ab cd") == [5, 6, 3, 4]
    with pytest.raises(ValueError, match="no vocabulary token spells"):
        aligner().tokenize("ab * c")                                                    # without a token '*' is a character
    longer = aligner(wildcard_token="<gap>", wildcard_penalty=1)
    assert longer.tokenize("a<gap>b <gap> c") == [1, W, 2, W, 3]


def test_adjacent_wildcards_collapse():
    al = aligner(wildcard_token="*", wildcard_penalty=0.5)
    assert al.tokenize("a ** b") == [1, W, 2] and al.tokenize("a * * b") == [1, W, 2]
    assert al.tokenize("***") == [W] and al.tokenize("* | * a") == [W, 1]
    assert al._ids([1, W, W, 2]) == [1, W, W, 2]                                        # id sequences are taken as they are


def test_refusals():
    with pytest.raises(ValueError, match="the vocabulary spells wildcard_token 'ab'"):
        aligner(wildcard_token="ab")
    with pytest.raises(ValueError, match="the vocabulary spells wildcard_token 'a b'"):
        aligner(wildcard_token="a b")
    for bad in ("", "  ", 3):
        with pytest.raises(ValueError, match="wildcard_token must be a non-empty string"):
            aligner(wildcard_token=bad)
    for bad in (-1.0, math.nan, math.inf, "0.5", True):
        with pytest.raises(ValueError, match="wildcard_penalty must be a finite number >= 0"):
            aligner(wildcard_penalty=bad)
    assert aligner(wildcard_penalty=0).wildcard_penalty == 0.0
    x = torch.zeros(1, 9, len(VOCAB))
    no_penalty = aligner(wildcard_token="*")
    with pytest.raises(ValueError, match="holds a wildcard but no wildcard_penalty"):
        no_penalty.align(x, ["a * b"])
    with pytest.raises(ValueError, match="holds a wildcard but no wildcard_penalty"):
        no_penalty(x, [[1, W, 2]])
    with pytest.raises(ValueError, match="segments: needs the aligner's wildcard_penalty"):
        no_penalty.segments(x, [["a", "b"]])
    with_penalty = aligner(wildcard_penalty=0.5)
    with pytest.raises(ValueError, match="LIST of utterances"):
        with_penalty.segments(x, ["a b"])
    with pytest.raises(ValueError, match="utterance 1 .* has no token to locate"):
        with_penalty.segments(x, [["a", " "]])
    with pytest.raises(ValueError, match="blank id"):
        with_penalty._ids([1, 0, W])
    with pytest.raises(ValueError, match="outside"):
        with_penalty._ids([1, -3])
    from conformer_amd._lib import ConformerHipError
    with pytest.raises(ConformerHipError):                                              # no CPU path
        with_penalty(x, [[1, W, 2]])
    with pytest.raises(ValueError, match="wildcard_penalty"):
        A.long_workspace_bytes(1, 100, 10, wildcard_penalty=math.nan)
    assert A.long_workspace_bytes(1, 100, 10, wildcard_penalty=0.5) == A.long_workspace_bytes(1, 100, 10) + 400


def test_group_words_closes_a_word_at_a_wildcard():
    ids = [1, 2, W, 3, 6, 4, W]
    starts, ends, scores = [0, 2, 3, 9, 10, 11, 12], [2, 3, 9, 10, 11, 12, 20], [-1.0, -2.0, -0.1, -3.0, -9.0, -4.0, -0.2]
    words = group_words(ids, starts, ends, scores, VOCAB, 6, 0.04, wildcard=W)
    assert [(w.text, w.start_frame, w.end_frame) for w in words] == [("ab", 0, 3), ("c", 9, 10), ("d", 11, 12)]
    assert words[0].score == pytest.approx((-1.0 * 2 + -2.0) / 3) and words[1].score == -3.0
    # the keyword is new: old calls read the arguments they always read
    assert group_words([1, 2, 6, 3], [0, 2, 3, 4], [2, 3, 4, 5], [-1.0, -2.0, -9.0, -3.0], VOCAB, 6, 0.04) == \
        [Word("ab", 0, 3, 0.0, 0.12, pytest.approx(-4.0 / 3)), Word("c", 4, 5, 0.16, 0.2, -3.0)]


def hand_made(ids_rows, starts_rows, ends_rows, scores_rows, ok):
    L = max(len(r) for r in ids_rows)
    pad = lambda rows, v: [list(r) + [v] * (L - len(r)) for r in rows]              # noqa: E731
    return Alignment(torch.zeros(len(ids_rows), 1, dtype=torch.int64), torch.zeros(len(ids_rows), 1, dtype=torch.int64),
                     torch.tensor(pad(starts_rows, -1)), torch.tensor(pad(ends_rows, -1)),
                     torch.tensor(pad(scores_rows, -math.inf), dtype=torch.float32), torch.zeros(len(ids_rows), dtype=torch.float64),
                     torch.tensor(ok))


def test_segments_assembly():
    al = aligner(wildcard_penalty=0.5)
    target, ranges = al.segment_targets(["ab c", [4, 6], "| d |"])
    assert target == [W, 5, 6, 3, W, 4, W, 4, W] and ranges == [(1, 4), (5, 6), (7, 8)]
    target2, ranges2 = al.segment_targets(["a", "b"], ends=False)
    assert target2 == [1, W, 2] and ranges2 == [(0, 1), (2, 3)]
    assert al.segment_targets([], ends=True) == ([W], []) and al.segment_targets([], ends=False) == ([], [])
    #          W    ab    |     c     W     d     W     d     W
    starts = [0, 5, 7, 8, 10, 20, 21, 30, 33]
    ends = [5, 7, 8, 10, 20, 21, 30, 33, 40]
    scores = [-0.5, -1.0, -6.0, -2.0, -0.5, -3.0, -0.5, -4.0, -0.5]
    hm = hand_made([target, target2], [starts, [0, 1, 2]], [ends, [1, 2, 3]], [scores, [-1.0, -1.0, -1.0]], [True, False])
    utterances = [["ab c", [4, 6], "| d |"], ["a", "b"]]
    segs = al.segments_of(utterances, [target, target2], [ranges, ranges2], hm)
    assert segs[1] == []                                                                # does not fit: no segments
    s0, s1, s2 = segs[0]
    assert isinstance(s0, Segment) and (s0.index, s0.text, s0.start_frame, s0.end_frame) == (0, "ab c", 5, 10)
    assert s0.start == pytest.approx(0.2) and s0.end == pytest.approx(0.4)
    assert s0.score == pytest.approx((-1.0 * 2 + -6.0 * 1 + -2.0 * 2) / 5)             # frame-weighted over its tokens
    assert [(w.text, w.start_frame, w.end_frame) for w in s0.words] == [("ab", 5, 7), ("c", 8, 10)]
    assert (s1.index, s1.text, s1.start_frame, s1.end_frame, s1.score) == (1, "d", 20, 21, -3.0)
    assert (s2.index, s2.text, s2.start_frame, s2.end_frame, s2.score) == (2, "| d |", 30, 33, -4.0)
    assert al.words([target], hm)[0] == s0.words + s1.words + s2.words                  # a wildcard yields no Word


def test_transcriber_refusals(monkeypatch):
    """Transcriber.__init__ needs a model on the device, so the methods run on a bare object that carries what they read before
    any tensor is touched (the model check is stood in for): the argument checks come before the front end and the encoder."""
    from conformer_amd import longform
    from conformer_amd.decode import BeamCTCDecoder
    tr = longform.Transcriber.__new__(longform.Transcriber)
    tr.decoder, tr.frame_seconds, tr.model = BeamCTCDecoder(VOCAB, 0, skip_ids=(7,)), 0.04, None
    monkeypatch.setattr(longform, "lstm_state", lambda *a, **kw: (torch.device("cpu"), None))
    mel = torch.zeros(80, 40)
    with pytest.raises(ValueError, match="one LIST of utterances per recording"):
        tr.segments([mel], ["ab"], 0.5)
    with pytest.raises(ValueError, match="one LIST of utterances per recording"):
        tr.segments([mel, mel], [["ab"]], 0.5)
    with pytest.raises(ValueError, match="wildcard_penalty has no default"):
        tr.segments([mel], [["ab"]], None)
    with pytest.raises(ValueError, match="wildcard_penalty must be a finite number >= 0"):
        tr.segments([mel], [["ab"]], -1.0)
    with pytest.raises(ValueError, match="no vocabulary token spells 'x'"):
        tr.segments([mel], [["ab", "axb"]], 0.5)
    with pytest.raises(ValueError, match="utterance 0 .* has no token to locate"):
        tr.segments([mel], [[[]]], 0.5)
    assert tr.segments([], [], 0.5) == []
    with pytest.raises(ValueError, match="the vocabulary spells wildcard_token"):
        tr.align([mel], ["ab"], wildcard_token="a", wildcard_penalty=0.5)
    with pytest.raises(ValueError, match="no vocabulary token spells"):
        tr.align([mel], ["a * b"])                                                      # no token given: '*' is a character


SEEDS = range(50)


def test_the_planted_construction_needs_wildcards_and_a_penalty():
    """with wildcards at penalty 0.5 every planted token span is recovered exactly, for every seed; without wildcards for
    none; at penalty 0 every planted frame ties with the wildcard and the smaller move keeps it: almost never"""
    yw, yn = F.planted_target(True), F.planted_target(False)
    assert yw == [W, 1, 2, W, 3, 3, 4, W, 5, 6, 7, W]
    with_wild = without = free = 0
    for seed in SEEDS:
        p = F.planted(seed)
        assert p.x.shape == (F.PLANT_T, F.PLANT_V) and (p.x * 8 == np.round(p.x * 8)).all()
        spans = F.planted_token_spans(p)
        assert len(spans) == 8 and all(0 < a < b <= F.PLANT_T - 1 for a, b in spans)
        assert all(b <= c for (_, b), (c, _) in zip(spans, spans[1:]))
        ref = F.expected(p.x, yw, F.PLANT_BLANK, F.PLANT_PENALTY)
        assert ref.ok and R.valid_path(F.extended(p.x, yw, F.PLANT_PENALTY)[1], ref.states)
        assert set(ref.frame_tokens.tolist()) == {W, 0, 1, 2, 3, 4, 5, 6, 7}
        with_wild += F.recovered(ref, yw, p)
        without += F.recovered(R.align(p.x, yn, F.PLANT_BLANK), yn, p)
        free += F.recovered(F.expected(p.x, yw, F.PLANT_BLANK, 0.0), yw, p)
    assert (with_wild, without) == (len(SEEDS), 0) and free <= len(SEEDS) // 10


def test_the_definition_on_a_tiny_case_against_brute_force():
    """x' and y' by hand for T = 5: the restatement on the extended pair is the brute-force optimum over every labelling"""
    rng = np.random.default_rng(7)
    for _ in range(20):
        x = (rng.integers(-8, 9, size=(5, 4)) / 4.0).astype(np.float32)
        for y in ([W], [1, W], [W, 2, W], [W, W]):
            xp, yp = F.extended(x, y, 0.5)
            assert xp.shape == (5, 5) and (xp[:, 4] == x.max(-1) - np.float32(0.5)).all() and W not in yp
            want = R.brute_force(xp, yp, 0)
            got = R.viterbi(xp, yp, 0)
            assert (want is None and got is None) or (got == want).all()
            ref = F.expected(x, y, 0, 0.5)
            wild = ref.frame_tokens == W
            assert wild.any() and ref.score == pytest.approx(float(np.where(
                wild, R.log_softmax64(x).max(-1), R.log_softmax64(x)[np.arange(5), np.maximum(ref.frame_tokens, 0)]).sum()))
