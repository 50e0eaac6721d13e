"""Error rates on the MI355X (conformer_amd/error_rate.py, cfm_error_rate_units and cfm_error_rate_distance).

Every output is an integer: errors, hyp_units and ref_units equal the plain-Python restatement (tests/error_rate_restatement.py)
integer for integer, for words, characters and tokens, at the lengths where the kernels change path: the 256-token tile of the
extraction, the 64-lane wave and the 512-column strip of the distance kernel, empty and very unequal sides, and the cap."""
import random

import numpy as np
import pytest
import torch

from conformer_amd import _lib
from conformer_amd.decode import BeamCTCDecoder, beam_ctc_decode, greedy_ctc_decode
from conformer_amd.error_rate import MAX_UNITS, ErrorRateMeter, ErrorRateTables, error_counts
from conformer_amd.evaluation import ConformerMetric
from tests import error_rate_restatement as R

pytestmark = pytest.mark.gpu

#         0    1    2    3     4      5    6    7             8    9        10  11   12   13   14
VOCAB = ["_", "a", "b", "ch", "sch", "|", " ", "\U0001F600", "é", "<unk>", "", "z", "s", "c", "h"]
SKIP = (0, 9)
KINDS, CPS = R.tables(VOCAB, "|", SKIP)
KIND_NAMES = ("word", "char", "token")
LETTERS = [1, 2, 8, 11, 12, 13, 14, 7]                                        # one code point each


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def tables():
    return ErrorRateTables(VOCAB, "|", SKIP)


def _letters(rng, n):
    return [rng.choice(LETTERS) for _ in range(n)]


def _words(rng, n):
    """n one-token words between single delimiters: n words, 2n - 1 characters, 2n - 1 tokens"""
    row = []
    for i in range(n):
        if i:
            row.append(5)
        row.append(rng.choice(LETTERS))
    return row


def _mutate(rng, row, k):
    row = list(row)
    for _ in range(k):
        op, at = rng.randrange(3), rng.randrange(len(row) + 1)
        if op == 0 and row:
            row[min(at, len(row) - 1)] = rng.choice(LETTERS)
        elif op == 1 and row:
            del row[min(at, len(row) - 1)]
        else:
            row.insert(at, rng.choice(LETTERS + [5]))
    return row


def _pairs():
    """(reference ids, hypothesis ids): the shapes at which the kernels can go wrong"""
    rng = random.Random(11)
    pairs = [([], []), ([], [1]), ([1], []), ([1], [1]), ([1], [2]), ([], _letters(rng, 70)), (_letters(rng, 70), [])]
    for n in (63, 64, 65, 255, 256, 257, 511, 512, 513):                     # the counts themselves, as characters and as words
        a = _letters(rng, n)
        pairs.append((a, _mutate(rng, a, 5)))
        if n <= 257:
            w = _words(rng, n)
            pairs.append((w, _mutate(rng, w, 7)))
    a = _letters(rng, 64)
    pairs += [(a, list(a)), (a, a[:63]), (a[:63], a), (a + a[:1], a)]         # identical; one lane more or less
    pairs += [([1] * 40, [2] * 50), ([1, 5, 1, 5, 1], [2, 5, 2])]             # no unit in common
    one, many, strip = _letters(rng, 1), _letters(rng, 257), _letters(rng, 513)
    pairs += [(one, many), (many, one), (one, strip), (strip, one), (many, strip), (strip, many)]   # very unequal sides
    pairs += [(_words(rng, 1), _words(rng, 257)), (_words(rng, 257), _words(rng, 1))]
    a = _letters(rng, 512)
    pairs += [(a, a + [1]), (a + [1], a), (a + [1], a + [2])]                 # just over the strip, on either side and on both
    # delimiters and skips
    pairs += [([5, 1, 2, 5, 5, 3, 5], [1, 2, 5, 3]),                          # leading, doubled and trailing delimiters
              ([6, 6, 1, 6, 5, 2], [1, 5, 2, 6]),                             # " " is a delimiter too, mixed runs
              ([5, 5, 6, 5], [1]), ([1], [5, 6]), ([5], [6, 5, 5]),           # delimiters only
              ([1, 0, 2, 9, 1], [1, 2, 1]), ([0, 9, 0], [9]),                 # skip ids inside a word; skips only
              ([1, 10, 2], [1, 2]), ([1, 10, 5, 10, 2], [1, 5, 2]),           # a token without code points separates nothing
              ([5, 0, 5, 1], [1]), ([1, 5, 0, 9, 5, 2], [1, 5, 2])]           # skips between delimiters
    # words
    pairs += [([1, 1, 2, 5, 2], [1, 1, 1, 5, 2]),                             # the same length, the last code point differs
              ([1, 2, 11, 5, 2], [1, 2, 5, 2]), ([1, 2], [1, 2, 11]),         # one a prefix of the other
              ([4, 5, 1], [12, 3, 5, 1]), ([4], [12, 13, 14]),                # the same word spelled with other tokens
              ([7, 8, 5, 7], [7, 5, 8, 7]), ([3, 3], [13, 14, 3])]            # non-BMP and multi-code-point tokens
    for _ in range(12):                                                       # random text over the whole vocabulary
        r = rng.choices(range(len(VOCAB)), weights=[1, 4, 4, 2, 1, 3, 1, 1, 1, 1, 1, 2, 1, 1, 1], k=rng.randint(0, 90))
        pairs.append((r, _mutate(rng, r, rng.randint(0, 6)) if rng.random() < 0.7 else
                      rng.choices(range(len(VOCAB)), k=rng.randint(0, 90))))
    return pairs


@pytest.fixture(scope="module")
def cases():
    """the pairs and, per kind, the restatement's (errors, hyp units, ref units): computed once, never changed"""
    pairs = _pairs()
    want = {k: [R.counts(h, len(h), r, len(r), KINDS, CPS, k) for r, h in pairs] for k in KIND_NAMES}
    return pairs, want


def _pad(rows, width, fill, seed=0):
    """(len(rows), width) int64 rows; behind each row: fill = an int, "valid" (random ids of the vocabulary) or "wild" (ids
    outside [0, V))"""
    rng = np.random.default_rng(seed)
    if fill == "valid":
        out = rng.integers(0, len(VOCAB), size=(len(rows), width))
    elif fill == "wild":
        out = rng.choice(np.array([-1, -2, len(VOCAB), len(VOCAB) + 7, 2 ** 31, 2 ** 40, -2 ** 40, 2 ** 32 + 1]), size=(len(rows), width))
    else:
        out = np.full((len(rows), width), fill)
    out = out.astype(np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return torch.from_numpy(out), torch.tensor([len(r) for r in rows], dtype=torch.int64)


def _want(want, kind):
    return tuple([w[i] for w in want[kind]] for i in range(3))


@pytest.mark.parametrize("fill", [-1, "valid", "wild"])
@pytest.mark.parametrize("kind", KIND_NAMES)
def test_counts_equal_the_restatement(dev, tables, cases, kind, fill):
    pairs, want = cases
    refs, hyps = [p[0] for p in pairs], [p[1] for p in pairs]
    ht, hc = _pad(hyps, max(map(len, hyps)) + 3, fill, 1)
    rt, rc = _pad(refs, max(map(len, refs)), fill, 2)
    e, nh, nr = error_counts(ht.to(dev), hc.to(dev), rt.to(dev), rc.to(dev), tables, unit=kind)
    assert e.dtype == nh.dtype == nr.dtype == torch.int32 and e.shape == nh.shape == nr.shape == (len(pairs),)
    we, wh, wr = _want(want, kind)
    assert nr.tolist() == wr and nh.tolist() == wh
    assert e.tolist() == we


def test_counts_past_the_row_and_below_zero_are_clamped(dev, tables):
    rows = [[1, 2, 5, 1], [1, 5, 2, 2]]
    t, _ = _pad(rows, 4, -1)
    big = torch.tensor([99, -3], dtype=torch.int64)
    for kind in KIND_NAMES:
        e, nh, nr = error_counts(t.to(dev), big.to(dev), t.to(dev), torch.tensor([4, 4]).to(dev), tables, unit=kind)
        want = [R.counts(rows[0], 99, rows[0], 4, KINDS, CPS, kind), R.counts(rows[1], -3, rows[1], 4, KINDS, CPS, kind)]
        assert list(zip(e.tolist(), nh.tolist(), nr.tolist())) == want and want[0][0] == 0 and want[1][1] == 0


def test_an_id_outside_the_vocabulary_in_front_of_the_count_spells_nothing(dev, tables):
    clean, dirty = [1, 2, 5, 3], [1, -1, 2, len(VOCAB), 5, 2 ** 40, 3, -2 ** 33]
    ct, cc = _pad([clean], 4, -1)
    dt, dc = _pad([dirty], 8, -1)
    for kind in KIND_NAMES:
        e, nh, nr = error_counts(dt.to(dev), dc.to(dev), ct.to(dev), cc.to(dev), tables, unit=kind)
        assert (e.tolist(), nh.tolist()) == ([0], nr.tolist()), kind


# ---- n-best input and the meter ---------------------------------------------------------------------------------------------------
def _nbest(rng, B=5, N=3, L=40):
    refs = [[rng.choice([1, 2, 3, 5, 8, 11]) for _ in range(rng.randint(3, L))] for _ in range(B)]
    hyps = [[_mutate(rng, r, rng.randint(0, 8))[:L] for _ in range(N)] for r in refs]
    hyps[1][1], hyps[1][2] = [], []                                           # unused rows: count 0
    hyps[3][2] = []
    hyps[4][0] = []                                                           # an empty best hypothesis is a hypothesis
    return refs, hyps


def _nbest_tensors(refs, hyps, L, dev, fill="valid"):
    B, N = len(hyps), len(hyps[0])
    ht, hc = _pad([h for hs in hyps for h in hs], L, fill, 3)
    rt, rc = _pad(refs, L + 2, fill, 4)
    return ht.reshape(B, N, L).to(dev), hc.reshape(B, N).to(dev), rt.to(dev), rc.to(dev)


def _expected_totals(refs, hyps):
    """what the meter should hold: best errors, reference units and oracle errors per kind, and the utterances"""
    best, units, oracle = [], [], []
    for kind in KIND_NAMES:
        per = [[R.counts(h, len(h), r, len(r), KINDS, CPS, kind) for h in hs] for r, hs in zip(refs, hyps)]
        best.append(sum(p[0][0] for p in per))
        units.append(sum(p[0][2] for p in per))
        oracle.append(sum(min(c[0] for n, (c, h) in enumerate(zip(p, hs)) if n == 0 or len(h) > 0)
                          for p, hs in zip(per, hyps)))
    return best + units + oracle + [len(refs)]


def test_n_best_rows_and_the_oracle(dev, tables):
    refs, hyps = _nbest(random.Random(3))
    ht, hc, rt, rc = _nbest_tensors(refs, hyps, 40, dev)
    for kind in KIND_NAMES:
        e, nh, nr = error_counts(ht, hc, rt, rc, tables, unit=kind)
        assert e.shape == nh.shape == (5, 3) and nr.shape == (5,)
        want = [[R.counts(h, len(h), r, len(r), KINDS, CPS, kind) for h in hs] for r, hs in zip(refs, hyps)]
        assert e.tolist() == [[c[0] for c in row] for row in want]
        assert nh.tolist() == [[c[1] for c in row] for row in want]
        assert nr.tolist() == [row[0][2] for row in want]
        assert e[1, 1].item() == nr[1].item() and nh[1, 1].item() == 0        # an unused row scores as an empty hypothesis
    m = ErrorRateMeter(tables)
    m.update(ht, hc, rt, rc)
    want = _expected_totals(refs, hyps)
    assert m.totals.dtype == torch.int64 and m.totals.is_cuda and m.totals.tolist() == want
    assert want[6] < want[0]                                                  # the oracle is better than the best row here
    out = m.compute()
    assert out["wer"] == want[0] / want[3] and out["cer"] == want[1] / want[4] and out["ter"] == want[2] / want[5]
    assert out["oracle_wer"] == want[6] / want[3] and out["oracle_cer"] == want[7] / want[4]
    assert out["oracle_ter"] == want[8] / want[5] and out["utterances"] == 5


def test_two_updates_accumulate_to_one_update_on_the_concatenated_batch(dev, tables):
    refs, hyps = _nbest(random.Random(4), B=6)
    ht, hc, rt, rc = _nbest_tensors(refs, hyps, 40, dev)
    one, two = ErrorRateMeter(tables), ErrorRateMeter(tables)
    one.update(ht, hc, rt, rc)
    two.update(ht[:2], hc[:2], rt[:2], rc[:2])
    two.update(ht[2:], hc[2:], rt[2:], rc[2:])                                # (non-contiguous views are fine)
    assert one.totals.tolist() == two.totals.tolist() == _expected_totals(refs, hyps)
    assert one.compute() == two.compute()
    # (B, L) input: the best row alone, whose oracle is itself
    g = ErrorRateMeter(tables)
    g.update(ht[:, 0], hc[:, 0], rt, rc)
    t = g.totals.tolist()
    assert t[:6] == one.totals.tolist()[:6] and t[6:9] == t[:3] and t[9] == 6
    two.reset()
    assert two.totals.tolist() == [0] * 10
    g.all_reduce()                                                            # no process group: nothing happens
    assert g.totals.tolist() == t


def test_conformer_metric_on_tokens_equals_conformer_metric_on_strings(dev, tables):
    refs, hyps = _nbest(random.Random(6))
    ht, hc, rt, rc = _nbest_tensors(refs, hyps, 40, dev)
    dec = BeamCTCDecoder(VOCAB, blank_id=0, skip_ids=SKIP)
    metric = ConformerMetric()
    texts_h, texts_r = [dec.text(hs[0]) for hs in hyps], [dec.text(r) for r in refs]
    for args in ((ht, hc), (ht[:, 0].contiguous(), hc[:, 0].contiguous())):
        w, c = metric.wer_tokens(*args, rt, rc, tables), metric.cer_tokens(*args, rt, rc, tables)
        assert w.is_cuda and w.dim() == 0 and c.is_cuda and c.dim() == 0
        assert float(w.float()) == float(metric.wer_score(texts_h, texts_r))
        assert float(c.float()) == float(metric.cer_score(texts_h, texts_r))
    empty = torch.zeros(5, dtype=torch.int64, device=dev)
    assert torch.isnan(metric.wer_tokens(ht, hc, rt, empty, tables)).item()


# ---- end to end: the decoders' own outputs ----------------------------------------------------------------------------------------
V40 = (["_", "|", " ", "<unk>"] + [chr(ord("a") + i) for i in range(26)]
       + ["ch", "sch", "é", "\U0001F600", "ß", "th", "ing", "'", "qu", ""])


def _e2e(dev, seed):
    assert len(V40) == 40
    g = torch.Generator().manual_seed(seed)
    logits = (3.0 * torch.randn(4, 50, 40, generator=g)).to(dev)
    logits[:, :, 1] += 4.0                                                    # enough delimiters for several words per row
    rng = random.Random(seed)
    refs = [rng.choices(range(1, 40), weights=[6] + [1] * 38, k=rng.randint(5, 30)) for _ in range(4)]
    rt, rc = _pad(refs, 30, "valid", seed)
    t = ErrorRateTables(V40, "|", (0, 3))
    dec = BeamCTCDecoder(V40, blank_id=0, skip_ids=(0, 3))
    return logits, refs, rt.to(dev), rc.to(dev), t, dec


def _assert_meter_equals_strings(out, texts_h, texts_r):
    metric = ConformerMetric()
    assert float(torch.tensor(out["wer"])) == float(metric.wer_score(texts_h, texts_r))
    assert float(torch.tensor(out["cer"])) == float(metric.cer_score(texts_h, texts_r))
    assert out["ref_words"] == sum(len(r.split()) for r in texts_r) and out["ref_chars"] == sum(map(len, texts_r))


def test_greedy_decode_into_the_meter_equals_conformer_metric_on_the_strings(dev):
    logits, refs, rt, rc, t, dec = _e2e(dev, 21)
    _, tokens, counts = greedy_ctc_decode(logits, 0, 3)
    m = ErrorRateMeter(t)
    m.update(tokens, counts, rt, rc)
    out = m.compute()
    texts_h = [dec.text(row[:n]) for row, n in zip(tokens.cpu().tolist(), counts.cpu().tolist())]
    texts_r = [dec.text(r) for r in refs]
    assert sum(len(x.split()) for x in texts_h) > 8 and out["word_errors"] > 0
    _assert_meter_equals_strings(out, texts_h, texts_r)


def test_beam_search_n_best_into_the_meter_equals_conformer_metric_on_the_strings(dev):
    logits, refs, rt, rc, t, dec = _e2e(dev, 22)
    tokens, counts, _, num = beam_ctc_decode(logits, 0, n_best=3, beam_width=16)
    m = ErrorRateMeter(t)
    m.update(tokens, counts, rt, rc)
    out = m.compute()
    tk, ct = tokens.cpu().tolist(), counts.cpu().tolist()
    texts_r = [dec.text(r) for r in refs]
    _assert_meter_equals_strings(out, [dec.text(tk[b][0][:ct[b][0]]) for b in range(4)], texts_r)
    assert num.min().item() >= 2
    metric = ConformerMetric()
    oracle = 0
    for b in range(4):
        rows = [n for n in range(3) if n == 0 or ct[b][n] > 0]
        oracle += min(round(float(metric.wer_score(dec.text(tk[b][n][:ct[b][n]]), texts_r[b])) * len(texts_r[b].split()))
                      for n in rows)
    assert out["oracle_word_errors"] == oracle <= out["word_errors"]


# ---- the buffers ------------------------------------------------------------------------------------------------------------------
def test_nothing_is_written_outside_the_outputs_or_behind_the_lengths(dev, tables):
    """raw entries on buffers with a sentinel border, and sentinel-filled rows: behind each length nothing is written"""
    S = -77
    rng = random.Random(9)
    refs = [_mutate(rng, _words(rng, 20), 3), [], _letters(rng, 300)]
    hyps = [[_mutate(rng, r, 4), [], _mutate(rng, r, 2)[:5]] for r in refs]
    B, N, L, PADR = 3, 3, 310, 2                                               # PADR sentinel rows on either side
    kind, off, cp = tables.on(dev)
    mc = tables.max_token_cps

    def extract(rows):
        n = len(rows)
        t, c = _pad(rows, L, "wild", 5)
        t, c = t.to(dev), c.to(dev)
        bufs = [torch.full((n + 2 * PADR, w), S, dtype=torch.int32, device=dev) for w in (L * mc, L * 4, L, 4)]
        ptr = [b[PADR:].data_ptr() for b in bufs]
        _lib.call("cfm_error_rate_units", t.data_ptr(), L, c.data_ptr(), n, L, kind.data_ptr(), off.data_ptr(), cp.data_ptr(),
                  len(VOCAB), mc, ptr[0], L * mc, ptr[1], L, ptr[2], L, ptr[3], torch.cuda.current_stream().cuda_stream)
        return bufs

    hb, rb = extract([h for hs in hyps for h in hs]), extract(refs)
    for bufs, rows in ((hb, [h for hs in hyps for h in hs]), (rb, refs)):
        host = [b.cpu() for b in bufs]
        for b in host:
            assert (b[:PADR] == S).all() and (b[-PADR:] == S).all()
        for i, row in enumerate(rows):
            lens = host[3][PADR + i].tolist()
            u = {k: R.units(row, len(row), KINDS, CPS, k) for k in KIND_NAMES}
            assert lens == [len(u["char"]), len(u["word"]), len(u["token"]), 0]
            assert host[0][PADR + i, :lens[0]].tolist() == u["char"] and (host[0][PADR + i, lens[0]:] == S).all()
            assert host[2][PADR + i, :lens[2]].tolist() == u["token"] and (host[2][PADR + i, lens[2]:] == S).all()
            spans = host[1][PADR + i].reshape(L, 4)
            assert (spans[lens[1]:] == S).all()
            assert [tuple(u["char"][s:s + n]) for s, n, _, _ in spans[:lens[1]].tolist()] == u["word"]
            assert (spans[:lens[1], 3] == 0).all()
    outs = [torch.full((3 * B * N + 8,), S, dtype=torch.int32, device=dev), torch.full((3 * B * N + 8,), S, dtype=torch.int32, device=dev),
            torch.full((3 * B + 8,), S, dtype=torch.int32, device=dev)]
    _lib.call("cfm_error_rate_distance", rb[0][PADR:].data_ptr(), L * mc, rb[1][PADR:].data_ptr(), L, rb[2][PADR:].data_ptr(), L,
              rb[3][PADR:].data_ptr(), hb[0][PADR:].data_ptr(), L * mc, hb[1][PADR:].data_ptr(), L, hb[2][PADR:].data_ptr(), L,
              hb[3][PADR:].data_ptr(), B, N, 3, outs[0][4:].data_ptr(), outs[1][4:].data_ptr(), outs[2][4:].data_ptr(),
              torch.cuda.current_stream().cuda_stream)
    e, nh, nr = (o.cpu() for o in outs)
    for o in (e, nh, nr):
        assert (o[:4] == S).all() and (o[-4:] == S).all()
    for p, k in enumerate(KIND_NAMES):
        want = [[R.counts(h, len(h), r, len(r), KINDS, CPS, k) for h in hs] for r, hs in zip(refs, hyps)]
        assert e[4:-4].reshape(3, B, N)[p].tolist() == [[c[0] for c in row] for row in want]
        assert nh[4:-4].reshape(3, B, N)[p].tolist() == [[c[1] for c in row] for row in want]
        assert nr[4:-4].reshape(3, B)[p].tolist() == [row[0][2] for row in want]
    # one kind per launch writes one plane only
    outs = [torch.full((B * N + 8,), S, dtype=torch.int32, device=dev), torch.full((B * N + 8,), S, dtype=torch.int32, device=dev),
            torch.full((B + 8,), S, dtype=torch.int32, device=dev)]
    _lib.call("cfm_error_rate_distance", rb[0][PADR:].data_ptr(), L * mc, None, 0, None, 0, rb[3][PADR:].data_ptr(),
              hb[0][PADR:].data_ptr(), L * mc, None, 0, None, 0, hb[3][PADR:].data_ptr(), B, N, 1, outs[0][4:].data_ptr(),
              outs[1][4:].data_ptr(), outs[2][4:].data_ptr(), torch.cuda.current_stream().cuda_stream)
    for o in outs:
        assert (o[:4] == S).all() and (o[-4:] == S).all() and (o[4:-4] != S).all()


def test_the_entries_refuse_bad_arguments_before_any_launch(dev, tables):
    kind, off, cp = tables.on(dev)
    z = torch.zeros(64, dtype=torch.int64, device=dev)
    o = torch.zeros(1024, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream().cuda_stream
    V, mc = len(VOCAB), tables.max_token_cps

    def units(ids=z.data_ptr(), ld_ids=4, R_=2, L=4, V_=V, mc_=mc, ld_cps=4 * mc, ld_words=4, ld_toks=4, lens=o.data_ptr()):
        _lib.call("cfm_error_rate_units", ids, ld_ids, z.data_ptr(), R_, L, kind.data_ptr(), off.data_ptr(), cp.data_ptr(), V_, mc_,
                  o.data_ptr(), ld_cps, o.data_ptr(), ld_words, o.data_ptr(), ld_toks, lens, s)

    units()
    for kw, msg in ((dict(ids=None), "null"), (dict(lens=None), "null"), (dict(R_=0), "shape"), (dict(L=0), "shape"),
                    (dict(V_=0), "shape"), (dict(mc_=-1), "shape"), (dict(ld_ids=3), "shape"), (dict(ld_cps=4 * mc - 1), "shape"),
                    (dict(ld_words=3), "shape"), (dict(ld_toks=3), "shape")):
        with pytest.raises(_lib.ConformerHipError, match="(?i)" + msg):
            units(**kw)
    with pytest.raises(_lib.ConformerHipError, match="(?i)unsupported"):
        units(L=MAX_UNITS // mc + 1, ld_ids=MAX_UNITS, ld_cps=4 * MAX_UNITS, ld_words=MAX_UNITS, ld_toks=MAX_UNITS)

    def distance(ref=o.data_ptr(), ld=8, B=2, N=2, unit=3, errors=o.data_ptr()):
        _lib.call("cfm_error_rate_distance", ref, ld, o.data_ptr(), ld, o.data_ptr(), ld, o.data_ptr(), o.data_ptr(), ld,
                  o.data_ptr(), ld, o.data_ptr(), ld, o.data_ptr(), B, N, unit, errors, o.data_ptr(), o.data_ptr(), s)

    for kw, msg in ((dict(ref=None), "null"), (dict(errors=None), "null"), (dict(B=0), "shape"), (dict(N=0), "shape"),
                    (dict(unit=4), "shape"), (dict(unit=-1), "shape"), (dict(ld=0), "shape"),
                    (dict(ld=MAX_UNITS + 1), "unsupported"), (dict(N=65536), "unsupported")):
        with pytest.raises(_lib.ConformerHipError, match="(?i)" + msg):
            distance(**kw)
    torch.cuda.synchronize()


# ---- the cap ----------------------------------------------------------------------------------------------------------------------
def _levenshtein_np(ref, hyp):
    """The restatement's recurrence a row at a time in numpy (the pure-Python loop takes minutes at the cap): with c[j] =
    min(prev[j] + 1, prev[j - 1] + cost), the row is cur[j] = min over k <= j of c[k] + (j - k), a running minimum of c[k] - k."""
    ref, hyp = np.asarray(ref, dtype=np.int64), np.asarray(hyp, dtype=np.int64)
    j = np.arange(len(hyp) + 1)
    prev = j.copy()
    for i, r in enumerate(ref, 1):
        c = np.empty_like(prev)
        c[0] = i
        c[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (hyp != r))
        prev = np.minimum.accumulate(c - j) + j
    return int(prev[-1])


def test_rows_at_the_cap_pass_and_a_row_over_it_is_refused(dev):
    vocab = ["_", "|"] + [chr(ord("a") + i) for i in range(6)]                # one code point per token: L may reach the cap
    t = ErrorRateTables(vocab, "|", (0,))
    kinds, cps = R.tables(vocab, "|", (0,))
    rng = random.Random(13)
    small = [rng.randrange(8) for _ in range(60)]
    assert _levenshtein_np(small, small[5:40]) == R.levenshtein(small, small[5:40])
    assert _levenshtein_np(small[::2], small) == R.levenshtein(small[::2], small)
    long_ = [rng.choice([1, 2, 2, 3, 4, 5, 6, 7]) for _ in range(MAX_UNITS)]  # no skip id: MAX_UNITS tokens and characters
    short = [x for x in long_[:3000] if rng.random() < 0.6]
    refs, hyps = [long_, short], [short, long_]                               # the full edge column; 32 strips
    ht, hc = _pad(hyps, MAX_UNITS, 0)
    rt, rc = _pad(refs, MAX_UNITS, 0)
    ht, hc, rt, rc = ht.to(dev), hc.to(dev), rt.to(dev), rc.to(dev)
    for kind in KIND_NAMES:
        u = [[R.units(x, len(x), kinds, cps, kind) for x in side] for side in (refs, hyps)]
        if kind == "word":                                                    # words as ids of their spellings
            ids = {}
            u = [[[ids.setdefault(w, len(ids)) for w in row] for row in side] for side in u]
        e, nh, nr = error_counts(ht, hc, rt, rc, t, unit=kind)
        assert nr.tolist() == [len(x) for x in u[0]] and nh.tolist() == [len(x) for x in u[1]]
        assert e.tolist() == [_levenshtein_np(u[0][b], u[1][b]) for b in range(2)], kind
    assert nr.tolist()[0] == MAX_UNITS
    m = ErrorRateMeter(t)
    m.update(ht[:, :500], hc.clamp(max=500), rt[:, :400], rc.clamp(max=400))
    before = m.totals.tolist()
    over = torch.ones(2, MAX_UNITS + 1, dtype=torch.int64, device=dev)
    n = torch.tensor([3, MAX_UNITS + 1], device=dev)
    with pytest.raises(_lib.ConformerHipError, match="(?i)unsupported|" + str(MAX_UNITS)):
        m.update(over, n, rt, rc)
    with pytest.raises(_lib.ConformerHipError, match="(?i)unsupported|" + str(MAX_UNITS)):
        m.update(ht, hc, over, n)
    with pytest.raises(_lib.ConformerHipError, match="(?i)unsupported|" + str(MAX_UNITS)):
        error_counts(ht[:, :MAX_UNITS // 3 + 1], hc, rt, rc, ErrorRateTables(["_", "|", "abc"]))   # three code points a token
    assert m.totals.tolist() == before and before[9] == 2
