"""Per-request hotwords without a GPU (INTEGRATION.md "Per-request hotwords"): the third-generation family
conformer_hip3_hotword_rows.h in the binding, its argument refusals (all before any HIP call), the table of the empty list, the
host layout of HotwordRows, and the reserved-size bound."""
import ctypes
import math
import os

import numpy as np
import pytest

from conformer_amd import _lib
from conformer_amd.hotwords import MAX_PHRASES, HotwordRows, Hotwords, reserved_bytes

HEADER = "conformer_hip3_hotword_rows.h"
DECODE, STEP, FINISH = ("cfm3_ctc_beam_hw_rows_decode_f32", "cfm3_ctc_beam_hw_rows_stream_step_f32",
                        "cfm3_ctc_beam_hw_rows_stream_finish_f32")
VOCAB = ["<pad>"] + [chr(ord("A") + i) for i in range(10)] + ["TH", "É", "ßA", "|", "<unk>"]
UNK = len(VOCAB) - 1


@pytest.fixture(scope="module")
def lib():
    from conformer_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


def test_the_header_is_discovered_and_declares_the_three_entries():
    assert HEADER in [os.path.basename(p) for p in _lib.OPEN_HEADERS]
    path = next(p for p in _lib.OPEN_HEADERS if os.path.basename(p) == HEADER)
    assert list(_lib.OPEN[path].signatures) == [DECODE, STEP, FINISH] and _lib.OPEN_CONSTANTS[HEADER] == {}
    assert [len(_lib.OPEN_PARAMS[n]) for n in (DECODE, STEP, FINISH)] == [26, 32, 24]
    # the first-generation entries with (hw_tables, hotword_weight) replaced by the two arrays, and the nullable times group
    first = _lib.PARAMS["cfm_ctc_beam_hw_decode_f32"]
    swap = lambda names: ["hw_row_tables" if n in ("hw_tables", "hw_tables_or_null") else                       # noqa: E731
                          "hw_row_weights" if n == "hotword_weight" else n for n in names]
    assert _lib.OPEN_PARAMS[DECODE] == swap(first)
    times = ["times_or_null", "times_bytes", "token_frames_or_null", "token_logp_or_null"]
    step = _lib.PARAMS["cfm_ctc_beam_stream_step_f32"]
    assert _lib.OPEN_PARAMS[STEP] == swap(step[:-1]) + times + step[-1:]
    fin = _lib.PARAMS["cfm_ctc_beam_stream_finish_f32"]
    assert _lib.OPEN_PARAMS[FINISH] == [n.replace("am_scores_or_null", "am_scores") for n in swap(fin[:-1])] + times + fin[-1:]
    assert _lib.OPEN_ENTRIES[DECODE][1][16] is ctypes.c_void_p and _lib.OPEN_ENTRIES[DECODE][1][17] is ctypes.c_void_p


def test_every_refusal_returns_before_any_hip_call(lib):
    """No GPU here: an entry that reached a launch would fail with a HIP status, not with these."""
    buf = (ctypes.c_double * 4096)()
    a = ctypes.addressof(buf)
    NULL, SHAPE, UNSUPPORTED = (_lib.CONSTANTS[k] for k in ("CFM_ERR_NULL", "CFM_ERR_BAD_SHAPE", "CFM_ERR_UNSUPPORTED"))
    B, T, V, W, K, N = 2, 8, 5, 4, 3, 2

    def call(entry, base, **kw):
        args = list(base)
        for k, v in kw.items():
            args[int(k[1:])] = v
        return entry(*args)

    # ---- the one-shot search
    ws = lib.cfm_ctc_beam_hw_workspace_bytes(B, T, W, K)
    good = [a, None, B, T, V, 0, W, K, -5.0, -10.0, N, None, 2.1, 9.2, -10.0, 1, a, a, a, ws, a, a, a, a, a, None]
    for i in (0, 16, 17, 18, 20, 21, 22, 23, 24):
        assert call(getattr(lib, DECODE), good, **{f"a{i}": None}) == NULL, i
    for i, bad in ((2, 0), (3, 0), (4, 1), (10, 0), (10, W + 1), (5, -1), (5, V), (8, math.nan), (9, math.nan), (12, math.inf),
                   (13, math.nan), (14, -math.inf), (19, ws - 1)):
        assert call(getattr(lib, DECODE), good, **{f"a{i}": bad}) == SHAPE, (i, bad)
    for i, bad in ((6, 0), (6, 257), (7, 0), (7, 33), (4, (1 << 23) + 1)):
        assert call(getattr(lib, DECODE), good, **{f"a{i}": bad}) == UNSUPPORTED, (i, bad)
    assert call(getattr(lib, DECODE), good, a0=None, a2=0) == NULL and call(getattr(lib, DECODE), good, a2=0, a6=0) == SHAPE    # the order
    # ---- the resumable step: ... state, bytes, T_max, t_used, 5 outputs, the times group, stream
    Tm = 16
    sb = lib.cfm_ctc_beam_stream_state_bytes(B, Tm, W, K, 0, 1)
    tb = lib.cfm_ctc_beam_times_bytes(B, Tm, W, 0)
    assert sb and tb
    step = [a, None, B, T, V, 0, W, K, -5.0, -10.0, N, None, 2.1, 9.2, -10.0, 1, a, a, a, sb, Tm, 0, a, a, a, None, a,
            None, 0, None, None, None]
    timed = list(step)
    timed[27:31] = [a, tb, a, a]
    for base in (step, timed):
        for i in (0, 16, 17, 18, 22, 23, 24, 26):
            assert call(getattr(lib, STEP), base, **{f"a{i}": None}) == NULL, i
        for i, bad in ((3, 0), (2, 0), (4, 1), (10, 0), (5, V), (21, -1), (21, Tm + 1), (21, Tm - T + 1), (19, sb - 1),
                       (12, math.nan), (8, math.nan)):
            assert call(getattr(lib, STEP), base, **{f"a{i}": bad}) == SHAPE, (i, bad)
        for i, bad in ((6, 257), (7, 33)):
            assert call(getattr(lib, STEP), base, **{f"a{i}": bad}) == UNSUPPORTED, (i, bad)
    for i in (27, 29, 30):                                  # a times group that is neither whole nor absent
        assert call(getattr(lib, STEP), timed, **{f"a{i}": None}) == NULL, i
    assert call(getattr(lib, STEP), step, a28=64) == NULL and call(getattr(lib, STEP), step, a29=a) == NULL
    assert call(getattr(lib, STEP), timed, a28=tb - 1) == SHAPE
    # ---- the finish: B, W, K, N, the fusion group, the arrays, state, bytes, T_max, 5 outputs, the times group, stream
    fin = [B, W, K, N, None, 2.1, 9.2, -10.0, 1, a, a, a, sb, Tm, a, a, a, a, a, None, 0, None, None, None]
    fint = list(fin)
    fint[19:23] = [a, tb, a, a]
    for base in (fin, fint):
        for i in (9, 10, 11, 14, 15, 16, 17, 18):
            assert call(getattr(lib, FINISH), base, **{f"a{i}": None}) == NULL, i
        for i, bad in ((0, 0), (3, 0), (3, W + 1), (13, 0), (12, sb - 1), (5, math.inf)):
            assert call(getattr(lib, FINISH), base, **{f"a{i}": bad}) == SHAPE, (i, bad)
        for i, bad in ((1, 0), (1, 257), (2, 33)):
            assert call(getattr(lib, FINISH), base, **{f"a{i}": bad}) == UNSUPPORTED, (i, bad)
    for i in (19, 21, 22):
        assert call(getattr(lib, FINISH), fint, **{f"a{i}": None}) == NULL, i
    assert call(getattr(lib, FINISH), fint, a20=tb - 1) == SHAPE and call(getattr(lib, FINISH), fin, a20=8) == NULL


def _header(blob):
    """HwHeader of csrc/hotword.h: magic, V, n_phrases, n_unigrams, n_cnodes, n_pnodes, (pad), total_bytes, 7 offsets, 2 masks"""
    ints = np.frombuffer(blob[:24].tobytes(), dtype=np.int32)
    longs = np.frombuffer(blob[24:24 + 64].tobytes(), dtype=np.int64)
    masks = np.frombuffer(blob[88:96].tobytes(), dtype=np.uint32)
    return ints, longs, masks


def test_the_empty_list_packs_to_a_valid_table_that_counts_nothing(lib):
    empty = Hotwords(())
    assert len(empty) == 0 and empty.unigrams == [] and empty.code_points == 0
    blob = empty.pack(VOCAB, "|", (UNK,))
    ints, longs, masks = _header(blob)
    assert ints[0] == 0x57484643 and ints[1] == len(VOCAB) and list(ints[2:6]) == [0, 0, 1, 1]      # the two roots only
    assert longs[0] == blob.nbytes and blob.nbytes % 256 == 0
    assert list(longs[1:]) == sorted(longs[1:]) and longs[1] >= 96 and longs[-1] < blob.nbytes and all(o % 256 == 0 for o in longs)
    assert list(masks) == [1, 1]                                            # two slots per trie, both empty
    ctrie = np.frombuffer(blob[longs[1]:longs[1] + 32].tobytes(), dtype=np.int32)
    ptrie = np.frombuffer(blob[longs[3]:longs[3] + 32].tobytes(), dtype=np.int32)
    assert ctrie[0] == ctrie[4] == -1 and ptrie[0] == ptrie[4] == -1
    # the vocabulary sections are those of any other list
    other = Hotwords(["A B", "THÉ"]).pack(VOCAB, "|", (UNK,))
    _, ol, _ = _header(other)
    for i in (5, 6, 7):
        end = longs[i + 1] if i < 7 else blob.nbytes
        assert bytes(blob[longs[i]:end]) == bytes(other[ol[i]:ol[i] + end - longs[i]]), i
    ID = {t: i for i, t in enumerate(VOCAB)}
    seqs = [[ID[t] for t in "A | B | C".split()], [ID["TH"], ID["É"], ID["|"], ID["ßA"], ID["B"]], [], [ID["|"], ID["|"]]]
    for w in (9.0, -3.0, 0.0):
        for counts, bonus, final in empty.count(seqs, VOCAB, "|", (UNK,), weight=w):
            assert not any(counts) and not any(bonus) and final == 0


def test_hotword_rows_layout():
    dec = Hotwords(["A", "B C"])
    rows = HotwordRows([["A B", "C"], None, (), ["A B", "  C "], [], Hotwords(["C", "A B"]), dec], [1.0, None, 0.0, -2.5, 4, 5.0, None],
                       VOCAB, "|", (UNK,), default=dec, default_weight=7.0)
    assert len(rows) == 7 and rows.distinct == 4                                  # ["A B","C"] x2, dec x2, empty x2, ["C","A B"]
    assert rows.offsets[0] == rows.offsets[3] and rows.offsets[2] == rows.offsets[4] and rows.offsets[1] == rows.offsets[6]
    assert len(set(rows.offsets)) == 4 and all(o % 256 == 0 for o in rows.offsets) and rows.blob.nbytes % 256 == 0
    assert rows.weights.dtype == np.float64 and rows.weights.tolist() == [1.0, 7.0, 0.0, -2.5, 4.0, 5.0, 7.0]
    for b, want in ((0, Hotwords(["A B", "C"])), (1, dec), (2, Hotwords(())), (5, Hotwords(["C", "A B"]))):
        t = want.pack(VOCAB, "|", (UNK,))
        assert bytes(rows.blob[rows.offsets[b]:rows.offsets[b] + t.nbytes]) == bytes(t), b
    # (the order of the phrases is part of a list: equal priority breaks ties in the given order)
    assert rows.offsets[5] != rows.offsets[0]
    # None without a decoder list is no hotwords; one weight serves every utterance
    plain = HotwordRows([None, ()], 2.0, VOCAB, "|", (UNK,))
    assert plain.distinct == 1 and plain.weights.tolist() == [2.0, 2.0]
    # a per-request list does not touch the decoder's own caches, nor any other
    assert list(dec._packed) == [(tuple(VOCAB), "|", frozenset((UNK,)))] and not dec._device


def test_hotword_rows_refusals():
    kw = dict(vocab=VOCAB, delim_token="|", skip_ids=(UNK,))
    with pytest.raises(ValueError, match="expected 3 entries"):
        HotwordRows([None, ()], None, batch=3, **kw)
    with pytest.raises(ValueError, match="one float or 2"):
        HotwordRows([None, ()], [1.0], **kw)
    for bad in (math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError, match="finite"):
            HotwordRows([None, ()], [1.0, bad], **kw)
        with pytest.raises(ValueError, match="finite"):
            HotwordRows([None], None, default_weight=bad, **kw)
    with pytest.raises(ValueError, match="max_phrases=2"):
        HotwordRows([["A", "B", "C"]], None, bounds=(2, 100), **kw)
    with pytest.raises(ValueError, match="max_code_points=4"):
        HotwordRows([(), ["AB CD E"]], None, bounds=(2, 4), **kw)
    HotwordRows([(), ["AB CD", "AB"]], None, bounds=(2, 6), **kw)            # at the bounds
    # the limits of Hotwords hold per list
    with pytest.raises(ValueError, match="at most 8 words"):
        HotwordRows([["A B C D E F G H I"]], None, **kw)
    with pytest.raises(ValueError, match="at most 1024 phrases"):
        HotwordRows([[f"{chr(0x4E00 + i)}" for i in range(MAX_PHRASES + 1)]], None, **kw)
    with pytest.raises(ValueError, match="must be a str"):
        HotwordRows([["A", 3]], None, **kw)
    with pytest.raises(ValueError, match="single string"):
        HotwordRows(["A B", "C"], None, **kw)                                # a flat list of phrases is not one entry per utterance
    with pytest.raises(ValueError, match="whitespace"):
        HotwordRows([["A"]], None, vocab=VOCAB + ["x y"], delim_token="|")
    with pytest.raises(ValueError, match="max_phrases"):
        reserved_bytes(MAX_PHRASES + 1, 10, VOCAB)


def _cp(i):
    return chr(0x4E00 + i)                                                     # distinct non-ASCII code points


@pytest.mark.parametrize("name,phrases", [
    ("one-character unigrams, 8 per phrase", [" ".join(_cp(8 * p + j) for j in range(8)) for p in range(64)]),
    ("one-character unigrams, one per phrase", [_cp(i) for i in range(300)]),
    ("one phrase of 8 long words", [" ".join(_cp(j) * 40 + "É" * j for j in range(8))]),
    ("non-ASCII words that share prefixes", ["ÉÉ ÉÉÉ ßAß", "ÉÉÉÉ ß", "ßAßA É", "日本 日本語 語"]),
    ("repeated words", ["A A A A A A A A", "A B A B", "B"]),
    ("the empty list", []),
], ids=lambda v: v.replace(" ", "_").replace(",", "") if isinstance(v, str) else "")
def test_reserved_bytes_is_an_upper_bound(lib, name, phrases):
    h = Hotwords(phrases)
    n = len(h.pack(VOCAB, "|", (UNK,)))
    P, C = len(h), h.code_points
    at = reserved_bytes(P, C, VOCAB, "|", (UNK,))
    assert n <= at, (name, n, at)
    assert at <= reserved_bytes(P + 1, C + 1, VOCAB, "|", (UNK,)) <= reserved_bytes(MAX_PHRASES, 4 * C + 64, VOCAB, "|", (UNK,))
    if len(h) > 1:                                                              # just under the bounds: the list less a phrase
        less = Hotwords(h.phrases[:-1])
        assert len(less.pack(VOCAB, "|", (UNK,))) <= reserved_bytes(len(less), less.code_points, VOCAB, "|", (UNK,)) <= at
    if "8 per phrase" in name or not phrases:                                   # all words distinct, 8 per phrase: the bound is met
        assert n == at
