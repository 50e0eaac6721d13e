"""Hotword boosting of the CTC beam search without a GPU: normalisation, priority order and limits (conformer_amd/hotwords.py);
the device's window step and bonus run on the host (cfm_hotword_count) against the literal re.findall definition; the float64
restatement (tests/ctc_beam_hotword_restatement.py) against brute force; the packer and the argument checks of the C
entries."""
import ctypes
import math
import os

import numpy as np
import pytest

from conformer_amd.hotwords import Hotwords, as_hotwords
from tests import ctc_beam_hotword_restatement as HR
from tests import ctc_beam_lm_restatement as LR
from tests import ctc_beam_restatement as R
from tests.test_ctc_beam_lm_cpu import ARPA3

INF = math.inf


@pytest.fixture(scope="module")
def lib():
    from conformer_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


# ---- the list
def test_normalisation_and_priority_order():
    h = Hotwords(["  fpt\ttelecom ", "fpt", "", "   ", "fpt  telecom", "ab", "cd", "telecom", "xyz"])
    assert h.phrases == ["fpt telecom", "fpt", "ab", "cd", "telecom", "xyz"]
    # longest first, ties in the given order
    assert h.priority == ["fpt telecom", "telecom", "fpt", "xyz", "ab", "cd"]
    assert h.unigrams == ["fpt", "telecom", "xyz", "ab", "cd"]
    assert h.phrase_ids == [[0, 1], [1], [0], [2], [3], [4]]
    assert HR.priority(["  fpt\ttelecom ", "fpt", "", "   ", "fpt  telecom", "ab", "cd", "telecom", "xyz"]) == h.priority
    assert Hotwords(["Ab", "ab"]).phrases == ["Ab", "ab"]               # no case folding


def test_limits_and_types():
    assert len(Hotwords([" ".join("w%d" % i for i in range(8))])) == 1
    with pytest.raises(ValueError, match="8 words"):
        Hotwords([" ".join("w%d" % i for i in range(9))])
    assert len(Hotwords(["p%d" % i for i in range(1024)] + ["p0"])) == 1024
    with pytest.raises(ValueError, match="1024 phrases"):
        Hotwords(["p%d" % i for i in range(1025)])
    with pytest.raises(ValueError, match="str"):
        Hotwords(["ok", 3])
    with pytest.raises(ValueError, match="str"):
        Hotwords([b"bytes"])
    with pytest.raises(ValueError, match="single string"):
        Hotwords("fpt")
    assert as_hotwords(None) is None and as_hotwords([]) is None and as_hotwords(["  "]) is None
    h = Hotwords(["a"])
    assert as_hotwords(h) is h


def test_whitespace_tokens_are_refused():
    h = Hotwords(["ab"])
    with pytest.raises(ValueError, match="whitespace"):
        h.pack(["_", "a b", "|"])
    with pytest.raises(ValueError, match="whitespace"):
        h.pack(["_", "a", "|", " "], skip_ids=(3,))
    h.pack(["_", "a", "|", " "])                                        # " " is a delimiter


# ---- counts
VOC = ["_", "a", "b", "c", "d", "e", "f", "g", "h", "x", "é", "ß", "|"]
DELIM = VOC.index("|")


def enc(text):
    return [DELIM if ch == " " else VOC.index(ch) for ch in text]


@pytest.mark.parametrize("text,want", [("ab", 1), ("ab cd", 1), ("ab cd ef gh", 1), ("x cd ef gh ab", 2), ("cd cd", 2),
                                       ("abcd", 0), ("", 0), ("cd ef", 1), ("cd ef gh cd ef gh", 2)])
def test_hand_counts_for_overlapping_phrases(lib, text, want):
    phrases = ["ab", "ab cd", "cd", "cd ef gh"]
    m = HR.Matcher(phrases)
    assert m.count(text.split()) == want
    (_, _, final), = Hotwords(phrases).count([enc(text)], VOC, weight=1.0)
    assert final == want


def test_longer_phrase_wins_over_its_parts(lib):
    phrases = ["fpt", "telecom", "fpt telecom"]
    assert HR.Matcher(phrases).count(["fpt", "telecom"]) == 1
    voc = ["_", "f", "p", "t", "e", "l", "c", "o", "m", "|"]
    seq = [voc.index(c) if c != " " else 9 for c in "fpt telecom fpt"]
    (_, _, final), = Hotwords(phrases).count([seq], voc, weight=1.0)
    assert final == 2


def random_case(rng, n_phr=6):
    alphabet = ["a", "b", "ab", "é", "ßa", "c"]
    words = ["".join(rng.choice(alphabet, size=rng.integers(1, 3))) for _ in range(10)]
    phrases = [" ".join(rng.choice(words, size=rng.integers(1, 4))) for _ in range(n_phr)]
    return words, phrases


def test_host_window_rule_equals_findall_on_every_prefix(lib):
    rng = np.random.default_rng(0)
    voc = ["_", "a", "b", "c", "é", "ß", "ab", "|", "<unk>"]
    d, unk = 7, 8
    n_seq = 0
    for trial in range(40):
        words, phrases = random_case(rng)
        if trial % 5 == 0:
            phrases.append(" ".join(rng.choice(words, size=8)))              # an 8-word phrase
        h = Hotwords(phrases)
        m = HR.Matcher(phrases)
        weight = float(rng.uniform(-5, 12))
        seqs = []
        for _ in range(60):
            seq = []
            for w in rng.choice(words, size=rng.integers(0, 14)):
                spell = [voc.index(ch) for ch in w]
                if rng.random() < 0.2:
                    spell.insert(int(rng.integers(0, len(spell) + 1)), unk)
                seq += spell + [d] * int(rng.integers(1, 3))
            if rng.random() < 0.5 and seq:
                seq = seq[:int(rng.integers(0, len(seq)))]
            seqs.append(seq)
        got = h.count(seqs, voc, skip_ids=(unk,), weight=weight)
        f = HR.Fusion(phrases, voc, skip_ids=(unk,), weight=weight)
        for seq, (counts, bonus, final) in zip(seqs, got):
            n_seq += 1
            for i in range(len(seq)):
                ws, p = f.words(seq[:i + 1])
                assert counts[i] == m.count(ws), (phrases, ws)
                assert bonus[i] == m.bonus(p, weight), (phrases, p)
            ws, p = f.words(seq)
            assert final == m.count(ws + ([p] if p else []))
    assert n_seq >= 2000


def test_bonus_by_hand(lib):
    m = HR.Matcher(["abc", "ab x", "abcdef"])
    assert m.bonus("a", 9.0) == 9.0 * 1 / 2 and m.bonus("abc", 9.0) == 9.0 * 3 / 3 and m.bonus("abcd", 9.0) == 9.0 * 4 / 6
    assert m.bonus("b", 9.0) == 0.0 and m.bonus("", 9.0) == 0.0
    voc = ["_", "a", "b", "c", "d", "|"]
    (_, bonus, _), = Hotwords(["abc", "ab x", "abcdef"]).count([[1, 2, 3, 4, 5, 2]], voc, weight=9.0)
    assert bonus == [4.5, 9.0, 9.0, 6.0, 0.0, 0.0]


# ---- the restatement
VOCAB = ["_", "A", "B", "|"]


@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("with_lm", [False, True], ids=["nolm", "lm"])
def test_restatement_equals_brute_force_in_the_exact_regime(tmp_path, T, with_lm):
    rng = np.random.default_rng(30 + T + 7 * with_lm)
    x = (rng.standard_normal((T, 4)) * 2).astype(np.float32)
    lm = None
    if with_lm:
        p = tmp_path / "m3.arpa"
        p.write_text(ARPA3, encoding="utf-8")
        lm = LR.Fusion(LR.Arpa.read(str(p)), VOCAB, alpha=0.7, beta=0.5)
    f = HR.Fusion(["A", "AB", "A B", "BB"], VOCAB, weight=2.5, lm=lm)
    bf = HR.brute_force(x, 0, f)
    out, _ = HR.beam_search(x, 0, f, 256, max_candidates=3, token_min_logp=-INF, beam_prune_logp=-INF, n_best=256)
    got = {seq: sc for seq, sc, am in out if am > -INF}
    assert set(got) == set(bf)
    for seq, sc in bf.items():
        assert abs(got[seq] - sc) <= 1e-9, (seq, got[seq], sc)


def test_hotwords_change_the_best_hypothesis():
    # acoustically "B" wins over "A"; the hotword A wins the boosted search
    x = np.log(np.array([[0.05, 0.42, 0.5, 0.03]], dtype=np.float64)).astype(np.float32)
    plain, _ = R.beam_search(x, 0, 8, n_best=8, token_min_logp=-INF, beam_prune_logp=-INF)
    assert plain[0][0] == (2,)
    boosted, _ = HR.beam_search(x, 0, HR.Fusion(["A"], VOCAB, weight=1.0), 8, n_best=8, token_min_logp=-INF,
                                beam_prune_logp=-INF)
    assert boosted[0][0] == (1,)
    assert boosted[0][1] == pytest.approx(math.log(0.42) + 1.0) and boosted[0][2] == pytest.approx(math.log(0.42))


def test_zero_weight_equals_the_unboosted_restatement():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((12, 4)) * 2).astype(np.float32)
    f = HR.Fusion(["A", "A B"], VOCAB, weight=0.0)
    a, _ = HR.beam_search(x, 0, f, 8, n_best=8, length=10)
    b, _ = R.beam_search(x, 0, 8, n_best=8, length=10)
    assert [(s, sc) for s, sc, _ in a] == b and [(s, am) for s, _, am in a] == b


# ---- the packer and the C entries
def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_pack_writes_the_tables(lib):
    h = Hotwords(["ab cd", "ab", "é"])
    blob = h.pack(VOC)
    hdr = np.frombuffer(blob[:24].tobytes(), dtype=np.int32)
    assert hdr[0] == 0x57484643 and hdr[1] == len(VOC) and hdr[2] == 3 and hdr[3] == 3
    assert hdr[4] == 1 + 2 + 2 + 1                       # character trie: root, a, ab, c, cd, é
    assert hdr[5] == 1 + 3                               # phrase trie: root, ab, ab cd, é
    assert h.pack(VOC) is blob                           # packed once per vocabulary
    assert h.pack(VOC, skip_ids=(9,)) is not blob


def test_pack_entries_validate_their_arguments_without_gpu(lib):
    uoff = np.array([0, 2, 3], dtype=np.int64)
    ucp = np.array([97, 98, 99], dtype=np.int32)
    poff = np.array([0, 2, 3], dtype=np.int64)
    pw = np.array([0, 1, 1], dtype=np.int32)
    toff = np.array([0, 0, 1, 1], dtype=np.int64)
    tcp = np.array([97], dtype=np.int32)
    kind = np.array([2, 0, 1], dtype=np.int32)
    need = lib.cfm_hotword_pack_bytes(2, 3, 2, 3, 3, 1)
    assert need > 0
    assert lib.cfm_hotword_pack_bytes(-1, 3, 2, 3, 3, 1) == 0
    assert lib.cfm_hotword_pack_bytes(2, 3, 1025, 3, 3, 1) == 0
    assert lib.cfm_hotword_pack_bytes(2, 3, 2, 17, 3, 1) == 0            # more than 8 words per phrase on average
    assert lib.cfm_hotword_pack_bytes(2, 3, 2, 3, 0, 1) == 0
    out = np.zeros(need, dtype=np.uint8)
    args = [2, _p(uoff), _p(ucp), 2, _p(poff), _p(pw), 3, _p(toff), _p(tcp), _p(kind), _p(out), need]
    names = ["n_uni", "uoff", "ucp", "n_phr", "poff", "pw", "V", "toff", "tcp", "kind", "out", "out_bytes"]

    def call(**kw):
        v = list(args)
        for k, x in kw.items():
            v[names.index(k)] = x
        return lib.cfm_hotword_pack(*v)

    assert call() == 0
    for name in ("uoff", "ucp", "poff", "pw", "toff", "tcp", "kind", "out"):
        assert call(**{name: None}) == -3, name
    assert call(n_phr=1025) < 0 and call(n_uni=-1) < 0
    assert call(out_bytes=need - 1) < 0
    bad = pw.copy(); bad[2] = 2
    assert call(pw=_p(bad)) < 0                                          # unigram id out of range
    dup = np.array([0, 1, 2], dtype=np.int64); cp = np.array([97, 97, 98], dtype=np.int32)
    assert call(uoff=_p(dup), ucp=_p(cp)) < 0                            # two unigrams, one spelling
    empty = np.array([0, 0, 3], dtype=np.int64)
    assert call(uoff=_p(empty)) < 0                                      # an empty unigram
    long_ = np.array([0, 9, 10], dtype=np.int64); pw9 = np.zeros(10, dtype=np.int32)
    assert call(poff=_p(long_), pw=_p(pw9)) < 0                          # a phrase of 9 words
    bk = kind.copy(); bk[1] = 3
    assert call(kind=_p(bk)) < 0
    # the host count entry, on a freshly packed blob
    assert call() == 0
    tok = np.array([1, 2, 1], dtype=np.int32)
    off = np.array([0, 3], dtype=np.int64)
    cnt = np.zeros(3, dtype=np.int32); bon = np.zeros(3); fin = np.zeros(1, dtype=np.int32)
    assert lib.cfm_hotword_count(_p(out), _p(tok), _p(off), 1, 1.0, _p(cnt), _p(bon), _p(fin)) == 0
    assert lib.cfm_hotword_count(None, _p(tok), _p(off), 1, 1.0, _p(cnt), _p(bon), _p(fin)) == -3
    assert lib.cfm_hotword_count(_p(out), _p(tok), _p(off), 0, 1.0, _p(cnt), _p(bon), _p(fin)) < 0
    assert lib.cfm_hotword_count(_p(out), _p(tok), _p(off), 1, math.nan, _p(cnt), _p(bon), _p(fin)) < 0
    assert lib.cfm_hotword_count(_p(out), _p(tok), _p(off), 1, math.inf, _p(cnt), _p(bon), _p(fin)) < 0
    badtok = np.array([1, 3, 1], dtype=np.int32)
    assert lib.cfm_hotword_count(_p(out), _p(badtok), _p(off), 1, 1.0, _p(cnt), _p(bon), _p(fin)) < 0
    junk = np.zeros(need, dtype=np.uint8)
    assert lib.cfm_hotword_count(_p(junk), _p(tok), _p(off), 1, 1.0, _p(cnt), _p(bon), _p(fin)) < 0


def test_hw_decode_entries_validate_their_arguments_without_gpu(lib):
    buf = (ctypes.c_float * 4096)()
    a = (ctypes.addressof(buf) + 255) // 256 * 256
    B, T, V, W, K = 2, 7, 5, 8, 4
    need = lib.cfm_ctc_beam_hw_workspace_bytes(B, T, W, K)
    assert need == lib.cfm_ctc_beam_workspace_bytes(B, T, W, K) > 0
    assert lib.cfm_ctc_beam_hw_workspace_bytes(B, T, 0, K) == 0
    assert lib.cfm_ctc_beam_hw_workspace_bytes(B, T, 257, K) == 0
    assert lib.cfm_ctc_beam_hw_workspace_bytes(B, T, W, 33) == 0
    args = [a, None, B, T, V, 0, W, K, -5.0, -10.0, 1, None, 2.1, 9.2, -10.0, 1, a, 9.0, a, need, a, a, a, a, a, None]
    names = ["logits", "lengths", "B", "T", "V", "blank", "W", "K", "tmin", "prune", "N", "lm", "alpha", "beta", "unk",
             "boundary", "hw", "weight", "ws", "ws_bytes", "tokens", "counts", "scores", "am_scores", "num_hyps", "stream"]

    def call(**kw):
        v = list(args)
        for k, x in kw.items():
            v[names.index(k)] = x
        return lib.cfm_ctc_beam_hw_decode_f32(*v)

    for name in ("logits", "hw", "ws", "tokens", "counts", "scores", "am_scores", "num_hyps"):
        assert call(**{name: None}) == -3, name
        assert call(lm=a, **{name: None}) == -3, name
    assert call(W=0) < 0 and call(W=257) < 0
    assert call(K=0) < 0 and call(K=33) < 0
    assert call(N=W + 1) < 0 and call(N=0) < 0
    assert call(blank=-1) < 0 and call(blank=V) < 0
    assert call(V=1, blank=0) < 0
    assert call(B=0) < 0 and call(T=0) < 0
    assert call(tmin=math.nan) < 0 and call(prune=math.nan) < 0
    assert call(alpha=math.nan) < 0 and call(beta=math.inf) < 0 and call(unk=-math.inf) < 0
    assert call(weight=math.nan) < 0 and call(weight=math.inf) < 0 and call(weight=-math.inf) < 0
    assert call(ws_bytes=need - 1) < 0


def test_python_entry_refuses_a_non_finite_weight():
    import torch
    from conformer_amd.decode import BeamCTCDecoder, beam_ctc_hotword_decode
    for w in (math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError, match="finite"):
            beam_ctc_hotword_decode(torch.zeros(1, 2, 4), 0, ["A"], vocab=VOCAB, hotword_weight=w)
        with pytest.raises(ValueError, match="finite"):
            BeamCTCDecoder(VOCAB, 0, hotwords=["A"], hotword_weight=w)
    assert BeamCTCDecoder(VOCAB, 0, hotwords=[]).hotwords is None
