"""Language-model fusion of the CTC beam search without a GPU: the ARPA loader (conformer_amd/lm.py) on a hand-made 3-gram
model with every backoff branch, gzip and malformed files; the float64 restatement (tests/ctc_beam_lm_restatement.py) against
brute force and against the LM-free restatement; the packer and the argument checks of the C entries."""
import ctypes
import gzip
import math
import os

import numpy as np
import pytest

from conformer_amd.lm import NgramLanguageModel, write_synthetic_arpa
from tests import ctc_beam_lm_restatement as LR
from tests import ctc_beam_restatement as R

INF = math.inf

ARPA3 = """
\\data\\
ngram 1=6
ngram 2=4
ngram 3=2

\\1-grams:
-1.0\t<s>\t-0.5
-0.7\t</s>
-0.8\tA\t-0.3
-0.9\tB\t-0.2
-1.2\tAB\t-0.25
-1.5\t<unk>

\\2-grams:
-0.4\t<s> A\t-0.1
-0.6\tA B\t-0.15
-0.5\tB </s>
-0.3\tA AB

\\3-grams:
-0.2\t<s> A B
-0.1\tA B </s>

\\end\\
"""

# (word, context, log10 P by hand): every branch of the backoff
HAND = [
    ("B", ("<s>", "A"), -0.2),                       # top-order hit
    ("AB", ("<s>", "A"), -0.1 + -0.3),               # backoff by one order: bo(<s> A) + p(A AB)
    ("</s>", ("<s>", "A"), -0.1 + -0.3 + -0.7),      # by two orders: bo(<s> A) + bo(A) + p(</s>)
    ("A", ("B", "AB"), -0.25 + -0.8),                # absent context "B AB" adds 0, then bo(AB) + p(A)
    ("XYZ", ("A",), -0.3 + -1.5),                    # an unknown word is <unk>: bo(A) + p(<unk>)
    ("</s>", ("A", "B"), -0.1),                      # </s> as a top-order hit
    ("</s>", ("B",), -0.5),
    ("A", (), -0.8),
]


@pytest.fixture
def arpa3(tmp_path):
    p = tmp_path / "m3.arpa"
    p.write_text(ARPA3, encoding="utf-8")
    return str(p)


def test_loader_reads_words_ids_and_float32_values(arpa3):
    lm = NgramLanguageModel.from_arpa(arpa3)
    assert lm.order == 3 and lm.counts == [6, 4, 2]
    assert lm.words == ["<s>", "</s>", "A", "B", "AB", "<unk>"]
    assert (lm.bos, lm.eos, lm.unk) == (0, 1, 5)
    ids, lp, bo = lm.ngrams[1]
    assert ids.dtype == np.int32 and lp.dtype == bo.dtype == np.float32
    assert ids.tolist() == [[0, 2], [2, 3], [3, 1], [2, 4]]
    assert lp.tolist() == np.float32([-0.4, -0.6, -0.5, -0.3]).tolist()
    assert bo.tolist() == np.float32([-0.1, -0.15, 0.0, 0.0]).tolist()        # a missing backoff is 0
    assert lm.ngrams[0][2][1] == 0.0 and lm.ngrams[2][2].tolist() == [0.0, 0.0]


@pytest.mark.parametrize("w,h,want", HAND)
def test_restatement_backoff_matches_hand_values(arpa3, w, h, want):
    lm = LR.Arpa.read(arpa3)
    assert lm.cond(w, h) == pytest.approx(want, abs=1e-6)


def test_sentence_scores_by_hand(arpa3):
    lm = LR.Arpa.read(arpa3)
    assert lm.sentence(["A", "B"]) == pytest.approx(-0.4 + -0.2 + -0.1, abs=1e-6)
    assert lm.sentence(["A", "B"], boundary=False) == pytest.approx(-0.8 + -0.6, abs=1e-6)
    assert lm.sentence(["Q"], boundary=False) == pytest.approx(-1.5, abs=1e-6)


def test_missing_unk_scores_minus_100(tmp_path):
    text = ARPA3.replace("ngram 1=6", "ngram 1=5").replace("-1.5\t<unk>\n", "")
    p = tmp_path / "nounk.arpa"
    p.write_text(text, encoding="utf-8")
    lm = NgramLanguageModel.from_arpa(str(p))
    assert lm.words[-1] == "<unk>" and lm.unk == 5 and lm.counts[0] == 6
    assert float(lm.ngrams[0][1][lm.unk]) == -100.0
    assert LR.Arpa.read(str(p)).cond("XYZ", ()) == -100.0


def test_gzip_equals_plain(arpa3, tmp_path):
    gz = tmp_path / "m3.arpa.gz"
    with gzip.open(gz, "wt", encoding="utf-8") as f:
        f.write(ARPA3)
    a, b = NgramLanguageModel.from_arpa(arpa3), NgramLanguageModel.from_arpa(str(gz))
    assert a.words == b.words
    for x, y in zip(a.ngrams, b.ngrams):
        for u, v in zip(x, y):
            assert np.array_equal(u, v)


MALFORMED = [
    ("no end", lambda t: t.replace("\\end\\", "")),
    ("count", lambda t: t.replace("ngram 2=4", "ngram 2=5")),
    ("count low", lambda t: t.replace("ngram 2=4", "ngram 2=3")),
    ("number", lambda t: t.replace("-0.6\tA B", "x.6\tA B")),
    ("fields", lambda t: t.replace("-0.6\tA B\t-0.15", "-0.6\tA B C D")),
    ("no unigram", lambda t: t.replace("-0.3\tA AB", "-0.3\tA ZZ")),
    ("order 7", lambda t: t.replace("ngram 3=2", "ngram 3=2\nngram 4=0\nngram 5=0\nngram 6=0\nngram 7=0")),
    ("no data", lambda t: t.replace("\\data\\", "")),
    ("no bos", lambda t: t.replace("ngram 1=6", "ngram 1=5").replace("-1.0\t<s>\t-0.5\n", "")
                          .replace("-0.4\t<s> A\t-0.1", "-0.4\tB A\t-0.1").replace("-0.2\t<s> A B", "-0.2\tB A B")),
]


@pytest.mark.parametrize("name,edit", MALFORMED, ids=[m[0] for m in MALFORMED])
def test_malformed_files_raise(tmp_path, name, edit):
    p = tmp_path / "bad.arpa"
    p.write_text(edit(ARPA3), encoding="utf-8")
    with pytest.raises(ValueError):
        NgramLanguageModel.from_arpa(str(p))


def test_malformed_line_is_named(tmp_path):
    p = tmp_path / "bad.arpa"
    p.write_text(ARPA3.replace("-0.6\tA B", "x.6\tA B"), encoding="utf-8")
    with pytest.raises(ValueError, match=r"bad\.arpa:17:"):
        NgramLanguageModel.from_arpa(str(p))


def test_kenlm_binary_is_refused(tmp_path):
    p = tmp_path / "m.bin"
    p.write_bytes(b"mmap lm http://kheafield.com/code format version 5\n\0\0\0")
    with pytest.raises(ValueError, match="binary"):
        NgramLanguageModel.from_arpa(str(p))
    q = tmp_path / "m.klm"
    q.write_text(ARPA3)
    with pytest.raises(ValueError, match="binary"):
        NgramLanguageModel.from_arpa(str(q))


# ---- the restatement
VOCAB = ["_", "A", "B", "|"]                    # blank 0, two letters, the delimiter


def fusion(arpa3, **kw):
    return LR.Fusion(LR.Arpa.read(arpa3), VOCAB, **kw)


def test_fusion_terms_by_hand(arpa3):
    f = fusion(arpa3, alpha=0.5, beta=1.5, unk_score_offset=-10.0)
    ln10 = math.log(10)
    st = f.of_sequence([1, 3, 2, 2])                    # "A|BB": A completed, partial "BB" spells no word prefix
    assert st[1] == "BB" and st[2] == ("<s>", "A")
    assert st[0] == pytest.approx(0.5 * ln10 * -0.4 + 1.5, abs=1e-6)      # float32 table values
    assert f.penalty("BB") == -10.0 and f.penalty("AB") == 0.0 and f.penalty("A") == 0.0
    assert f.penalty("BBBBBBBBB") == pytest.approx(-10.0 * 9 / 6)
    # the end: "BB" is OOV (scored as <unk> plus the offset), then </s> after (A, <unk>)
    want = st[0] + (0.5 * ln10 * ((-0.1 + -0.3 + -1.5) + -10.0) + 1.5) + 0.5 * ln10 * -0.7
    assert f.final(st) == pytest.approx(want, abs=1e-6)
    assert f.of_sequence([3, 3]) == f.root()            # delimiters with an empty partial word add nothing
    g = fusion(arpa3, skip_ids=(2,))
    assert g.of_sequence([1, 2, 1]) == (0.0, "AA", ("<s>",))     # a skipped token has no characters


def exact(logits, f, W=256, length=None):
    V = logits.shape[1]
    return LR.beam_search(logits, 0, f, W, max_candidates=V - 1, token_min_logp=-INF, beam_prune_logp=-INF, n_best=W,
                          length=length)


@pytest.mark.parametrize("T", [1, 2, 3, 4])
@pytest.mark.parametrize("kw", [{}, {"score_boundary": False}, {"alpha": 0.7, "beta": -1.0, "unk_score_offset": -3.0}],
                         ids=["default", "noboundary", "weights"])
def test_restatement_equals_brute_force_in_the_exact_regime(arpa3, T, kw):
    rng = np.random.default_rng(10 * T + len(kw))
    x = (rng.standard_normal((T, 4)) * 2).astype(np.float32)
    f = fusion(arpa3, **kw)
    bf = LR.brute_force(x, 0, f)
    out, _ = exact(x, f)
    got = {seq: sc for seq, sc, am in out if am > -INF}
    assert set(got) == set(bf)
    for seq, sc in bf.items():
        assert abs(got[seq] - sc) <= 1e-9, (seq, got[seq], sc)
    assert [s for _, s, _ in out] == sorted((s for _, s, _ in out), reverse=True)


def test_lm_changes_the_ranking(arpa3):
    # acoustically "B" wins over "A"; the model prefers the word A (and penalises nothing else)
    x = np.log(np.array([[0.05, 0.42, 0.5, 0.03]], dtype=np.float64)).astype(np.float32)
    plain, _ = R.beam_search(x, 0, 8, n_best=8, token_min_logp=-INF, beam_prune_logp=-INF)
    assert plain[0][0] == (2,)
    fused, _ = LR.beam_search(x, 0, fusion(arpa3, alpha=2.0, beta=0.0), 8, n_best=8, token_min_logp=-INF,
                              beam_prune_logp=-INF)
    assert fused[0][0] == (1,)


@pytest.mark.parametrize("seed", range(4))
def test_zero_weights_equal_the_lm_free_restatement(tmp_path, seed):
    rng = np.random.default_rng(seed)
    toks = [chr(ord("a") + i) for i in range(12)] + ["th", "ch"]
    vocab = ["<pad>"] + toks + ["|", "<unk>"]
    write_synthetic_arpa(tmp_path / "s.arpa", toks, 40, [0, 120, 160], seed=seed)
    f = LR.Fusion(LR.Arpa.read(str(tmp_path / "s.arpa")), vocab, skip_ids=(16,), alpha=0.0, beta=0.0, unk_score_offset=0.0)
    x = (rng.standard_normal((20, len(vocab))) * 2).astype(np.float32)
    for W, N in ((1, 1), (8, 4), (32, 32)):
        a, ma = LR.beam_search(x, 0, f, W, n_best=N, length=17)
        b, mb = R.beam_search(x, 0, W, n_best=N, length=17)
        assert [(s, sc) for s, sc, _ in a] == b
        assert [(s, am) for s, _, am in a] == b


def test_synthetic_arpa_is_deterministic_and_valid(tmp_path):
    toks = ["A", "B", "C", "DE"]
    w1 = write_synthetic_arpa(tmp_path / "a.arpa", toks, 30, [0, 80, 90, 60], seed=3)
    w2 = write_synthetic_arpa(tmp_path / "b.arpa.gz", toks, 30, [0, 80, 90, 60], seed=3)
    assert w1 == w2
    a = NgramLanguageModel.from_arpa(tmp_path / "a.arpa")
    b = NgramLanguageModel.from_arpa(tmp_path / "b.arpa.gz")
    assert a.counts == b.counts == [33, 80, 90, 60]
    ref = LR.Arpa.read(str(tmp_path / "a.arpa"))
    assert len(ref.table) == sum(a.counts)


# ---- the packer and the C entries
@pytest.fixture(scope="module")
def lib():
    from conformer_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


def test_pack_writes_the_tables(arpa3, lib):
    lm = NgramLanguageModel.from_arpa(arpa3)
    blob = lm.pack(VOCAB)
    hdr = np.frombuffer(blob[:36].tobytes(), dtype=np.int32)
    assert hdr[0] == 0x4D4C4643 and hdr[1] == 3 and hdr[2] == len(VOCAB) and hdr[3] == 6
    assert tuple(hdr[4:7]) == (0, 1, 5)
    assert hdr[7] == 4                                   # trie nodes: root, A, B, AB
    assert lm.pack(VOCAB) is blob                        # packed once per vocabulary


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def test_pack_entries_validate_their_arguments_without_gpu(lib):
    counts = np.array([3, 1], dtype=np.int64)
    ids = np.array([0, 1, 2, 0, 2], dtype=np.int32)
    lp = np.full(4, -1.0, dtype=np.float32)
    bo = np.zeros(4, dtype=np.float32)
    woff = np.array([0, 3, 7, 10], dtype=np.int64)
    wcp = np.array([ord(c) for c in "<s></s>WOR"], dtype=np.int32)
    toff = np.array([0, 0, 1, 1], dtype=np.int64)
    tcp = np.array([ord("W")], dtype=np.int32)
    kind = np.array([2, 0, 1], dtype=np.int32)
    need = lib.cfm_ngram_lm_pack_bytes(2, _p(counts), 3, 10, 3, 1)
    assert need > 0
    assert lib.cfm_ngram_lm_pack_bytes(0, _p(counts), 3, 10, 3, 1) == 0
    assert lib.cfm_ngram_lm_pack_bytes(7, _p(counts), 3, 10, 3, 1) == 0
    assert lib.cfm_ngram_lm_pack_bytes(2, None, 3, 10, 3, 1) == 0
    assert lib.cfm_ngram_lm_pack_bytes(2, _p(counts), 4, 10, 3, 1) == 0          # counts[0] != n_words
    out = np.zeros(need, dtype=np.uint8)
    args = [2, _p(counts), _p(ids), _p(lp), _p(bo), 3, _p(woff), _p(wcp), 0, 1, 2, 3, _p(toff), _p(tcp), _p(kind), _p(out), need]
    names = ["order", "counts", "ids", "lp", "bo", "n_words", "woff", "wcp", "bos", "eos", "unk", "V", "toff", "tcp", "kind",
             "out", "out_bytes"]

    def call(**kw):
        v = list(args)
        for k, x in kw.items():
            v[names.index(k)] = x
        return lib.cfm_ngram_lm_pack(*v)

    assert call() == 0
    for name in ("counts", "ids", "lp", "bo", "woff", "toff", "kind", "out"):
        assert call(**{name: None}) == -3, name
    assert call(order=0) == -2 and call(order=7) == -2
    assert call(out_bytes=need - 1) < 0
    assert call(bos=3) < 0 and call(unk=-1) < 0
    bad = ids.copy(); bad[4] = 3
    assert call(ids=_p(bad)) < 0                                                   # word id out of range
    dup = ids.copy(); dup[1] = 0
    assert call(ids=_p(dup)) < 0                                                   # a unigram twice
    bk = kind.copy(); bk[1] = 3
    assert call(kind=_p(bk)) < 0


def test_lm_decode_entries_validate_their_arguments_without_gpu(lib):
    buf = (ctypes.c_float * 4096)()
    a = (ctypes.addressof(buf) + 255) // 256 * 256
    B, T, V, W, K = 2, 7, 5, 8, 4
    need = lib.cfm_ctc_beam_lm_workspace_bytes(B, T, W, K)
    assert need == lib.cfm_ctc_beam_workspace_bytes(B, T, W, K) > 0
    assert lib.cfm_ctc_beam_lm_workspace_bytes(B, T, 0, K) == 0
    assert lib.cfm_ctc_beam_lm_workspace_bytes(B, T, 257, K) == 0
    assert lib.cfm_ctc_beam_lm_workspace_bytes(B, T, W, 33) == 0
    args = [a, None, B, T, V, 0, W, K, -5.0, -10.0, 1, a, 2.1, 9.2, -10.0, 1, a, need, a, a, a, a, a, None]
    names = ["logits", "lengths", "B", "T", "V", "blank", "W", "K", "tmin", "prune", "N", "lm", "alpha", "beta", "unk",
             "boundary", "ws", "ws_bytes", "tokens", "counts", "scores", "am_scores", "num_hyps", "stream"]

    def call(**kw):
        v = list(args)
        for k, x in kw.items():
            v[names.index(k)] = x
        return lib.cfm_ctc_beam_lm_decode_f32(*v)

    for name in ("logits", "lm", "ws", "tokens", "counts", "scores", "am_scores", "num_hyps"):
        assert call(**{name: None}) == -3, name
    assert call(W=0) < 0 and call(W=257) < 0
    assert call(K=0) < 0 and call(K=33) < 0
    assert call(N=W + 1) < 0 and call(N=0) < 0
    assert call(blank=-1) < 0 and call(blank=V) < 0
    assert call(V=1, blank=0) < 0
    assert call(B=0) < 0 and call(T=0) < 0
    assert call(tmin=math.nan) < 0 and call(prune=math.nan) < 0
    assert call(alpha=math.nan) < 0 and call(beta=math.inf) < 0 and call(unk=-math.inf) < 0
    assert call(ws_bytes=need - 1) < 0
    assert lib.cfm_ngram_lm_score_f64(None, a, a, 1, 1, a, None) == -3
    assert lib.cfm_ngram_lm_score_f64(a, a, a, 0, 1, a, None) < 0
