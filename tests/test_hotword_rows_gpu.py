"""Per-request hotwords on the MI355X (INTEGRATION.md "Per-request hotwords"): a hotword list and a weight per utterance, from
the search kernel up to SlotTranscriber.open and Transcriber.transcribe.

The definition is the existing single-list search: row b of every output equals, bit for bit, what that search returns for
utterance b alone under its list and weight.  The batch of tests/hotword_rows_cases.py holds the SAME logits in every row, so a
kernel that mixed the rows' tables, or ignored them, returns equal rows where the reference rows differ (asserted)."""
import math

import pytest
import torch

from conformer_amd.decode import (BeamCTCDecoder, _beam_search, beam_ctc_decode, beam_ctc_hotword_decode, beam_ctc_lm_decode)
from conformer_amd.hotwords import Hotwords, reserved_bytes
from tests import hotword_rows_cases as C
from tests.test_ctc_beam_hotword_gpu import G_UNK, GVOCAB, MARGIN, close32, dev, small_lm  # noqa: F401  (fixtures)
from tests.test_endpoint_gpu import VOCAB, _tiny_model
from tests.test_write_guard_gpu import guarded_allocations

pytestmark = pytest.mark.gpu
INF = math.inf
B = len(C.ENTRIES)
LM = pytest.mark.parametrize("with_lm", [False, True], ids=["nolm", "lm"])
BEAMS = pytest.mark.parametrize("W,N", C.BEAMS, ids=lambda v: str(v))


def decoder(lm=None, W=16, hotwords=C.DEC, weight=C.DEC_WEIGHT):
    return BeamCTCDecoder(GVOCAB, 0, skip_ids=(G_UNK,), beam_width=W, hotwords=hotwords, hotword_weight=weight, lm=lm,
                          **C.LMKW, **C.KNOBS)


def rows_search(x, dec, N, entries=C.ENTRIES, weights=C.WEIGHTS, lengths=None, times=False):
    """the decoder's search with per-request hotwords, every output (what __call__ and words() run)"""
    out = _beam_search(x, 0, lengths, N, dec.beam_width, dec.token_min_logp, dec.beam_prune_logp, dec.max_candidates, GVOCAB,
                       dec._call_fusion(x.shape[0], entries, weights), times)
    return out


def single(x, phrases, weight, lm, W, N, lengths=None, times=False):
    """the existing single-list call (the unboosted searches for a list without phrases)"""
    kw = dict(beam_width=W, n_best=N, return_times=times, **C.KNOBS)
    if len(Hotwords(phrases)):
        return beam_ctc_hotword_decode(x, 0, phrases, lengths, vocab=GVOCAB, skip_ids=(G_UNK,), hotword_weight=weight, lm=lm,
                                       **C.LMKW, **kw)
    if lm is not None:
        return beam_ctc_lm_decode(x, 0, lm, lengths, vocab=GVOCAB, skip_ids=(G_UNK,), **C.LMKW, **kw)
    out = beam_ctc_decode(x, 0, lengths, **kw)
    return (*out[:3], out[2], *out[3:])                       # (am_scores = scores without fusion)


def flat(out):
    return [t for u in out for t in (u if isinstance(u, tuple) else (u,))]


def same(got, want, b, what=""):
    """Row b of `got` (a batch) equals row 0 of `want` (one utterance) bit for bit, the times pair included.  Where the tree of
    `got` has room for more frames, its (B, N, T') outputs hold the same T columns and then padding."""
    g, w = flat(got), flat(want)
    assert len(g) == len(w), (what, b, len(g), len(w))
    for i, (u, v) in enumerate(zip(g, w)):
        assert u.dtype == v.dtype, (what, b, i)
        if u.dim() == 3 and u.shape[2] > v.shape[2]:
            T = v.shape[2]
            assert bool((u[b, :, T:] == (-1 if u.dtype == torch.int64 else -INF)).all()), (what, b, i)
            u = u[:, :, :T]
        assert torch.equal(u[b], v[0]), (what, b, i)


def best(out, b=0):
    n = int(out[1][b, 0])
    return tuple(out[0][b, 0, :n].tolist()), float(out[2][b, 0])


@pytest.fixture(scope="module")
def xb(dev):
    return torch.from_numpy(C.batch()).to(dev)


@pytest.fixture(scope="module")
def references(dev, xb, small_lm):
    """The single-list reference rows, once: {(with_lm, W, N, times): ([row outputs], unboosted outputs)}.  Left unchanged."""
    out = {}
    for with_lm in (False, True):
        lm = small_lm[1] if with_lm else None
        for W, N in C.BEAMS:
            for times in (False, True):
                rows = [single(xb[b:b + 1], C.LISTS[b], C.WEIGHTS[b], lm, W, N, times=times) for b in range(B)]
                out[with_lm, W, N, times] = (rows, single(xb[:1], [], 0.0, lm, W, N, times=times))
    return out


@LM
@BEAMS
@pytest.mark.parametrize("times", [False, True], ids=["", "times"])
def test_no_cross_talk(dev, xb, small_lm, references, with_lm, W, N, times):
    lm = small_lm[1] if with_lm else None
    rows, plain = references[with_lm, W, N, times]
    # the references alone tell the lists apart: otherwise a kernel that ignored them would pass
    bests = [best(r) for r in rows]
    assert C.distinct([bests[0], bests[1], bests[3], best(plain)]), bests
    assert bests[2] == best(plain)
    got = rows_search(xb, decoder(lm, W), N, times=times)
    assert got[0].shape[:2] == (B, N)
    for b in range(B):
        same(got, rows[b], b, "rows")
    same(got, plain, 2, "the empty list is the search without hotwords")
    # the functional form: None is no hotwords there (no decoder whose list it could mean), weights as a list
    fn = beam_ctc_hotword_decode(xb, 0, [C.L1, C.L2, (), None], vocab=GVOCAB, skip_ids=(G_UNK,), hotword_weight=C.WEIGHTS, lm=lm,
                                 beam_width=W, n_best=N, return_times=times, **C.LMKW, **C.KNOBS)
    for b in (0, 1, 2):
        same(fn, rows[b], b, "functional")
    same(fn, plain, 3, "functional None")


@LM
@BEAMS
def test_against_the_definition(dev, xb, small_lm, with_lm, W, N):
    lm_path = small_lm[0] if with_lm else None
    ref_rows, ref_plain = C.restated(lm_path, W, N)
    assert C.margins_ok(ref_rows, ref_plain, MARGIN) and C.lists_matter(ref_rows, ref_plain)
    tokens, counts, scores, am, num = (t.cpu() for t in rows_search(xb, decoder(small_lm[1] if with_lm else None, W), N))
    for b, (hyps, _) in enumerate(ref_rows):
        assert int(num[b]) == len(hyps), (b, int(num[b]), len(hyps))
        for r, (seq, sc, a) in enumerate(hyps):
            n = int(counts[b, r])
            assert tuple(tokens[b, r, :n].tolist()) == seq, (b, r)
            assert close32(float(scores[b, r]), sc), (b, r, float(scores[b, r]), sc)
            assert close32(float(am[b, r]), a), (b, r, float(am[b, r]), a)
            assert bool((tokens[b, r, n:] == -1).all())
        for r in range(len(hyps), N):
            assert int(counts[b, r]) == 0 and float(scores[b, r]) == -INF and float(am[b, r]) == -INF


def stream_with_lists(dec, dev, T, **kw):
    st = dec.stream(B, T, dev, hotword_rows=(8, 40), **kw)
    for b in range(B):
        st.set_hotwords(b, C.ENTRIES[b], C.WEIGHTS[b])
    return st


def chunk(xb, at, width):
    """(B, width, V): row b's frames at[b] .. at[b] + width - 1 (zeros past its end)"""
    out = torch.zeros(xb.shape[0], width, xb.shape[2], device=xb.device)
    for b, a in enumerate(at):
        n = max(0, min(width, xb.shape[1] - a))
        out[b, :n] = xb[b, a:a + n]
    return out


@LM
@pytest.mark.parametrize("times", [False, True], ids=["", "times"])
def test_streaming_equals_the_one_shot_rows(dev, xb, small_lm, references, with_lm, times):
    from conformer_amd.decode import beam_ctc_stream_finish
    W, N = C.BEAMS[0]
    rows, _ = references[with_lm, W, N, times]
    T = xb.shape[1]
    dec = decoder(small_lm[1] if with_lm else None, W)
    for cuts in ([T], [1, 7, 8, 20, T], [5, 6, T]):
        st = stream_with_lists(dec, dev, T, times=times)
        t0 = 0
        for t1 in cuts:
            st.step(xb[:, t0:t1].contiguous())
            t0 = t1
        got = beam_ctc_stream_finish(st.state, N)
        for b in range(B):
            same(got, rows[b], b, f"cuts {cuts}")
    # ragged: rows 1 and 3 consume no frame in the first step and stay k frames behind
    k = 4
    st = stream_with_lists(dec, dev, T + k, times=times)
    at = [0] * B
    for width, take in ((k, [k, 0, k, 0]), (k, [k] * B), (T - k, None)):
        take = [T - a for a in at] if take is None else take
        st.step(chunk(xb, at, width), torch.tensor(take, device=dev))
        at = [a + n for a, n in zip(at, take)]
        with pytest.raises(RuntimeError, match="empty prefix"):
            st.set_hotwords(1, C.L1)                         # (stepped, even where it consumed nothing: the host cannot know)
    assert at == [T] * B
    got = beam_ctc_stream_finish(st.state, N)
    for b in range(B):
        same(got, rows[b], b, "ragged")
    st.reset()
    st.set_hotwords(1, C.L1)                                  # at the empty prefix again


@pytest.mark.parametrize("short,weight", [(["B C"], 9.0), ((), 3.0)], ids=["short", "empty"])
def test_slot_reuse_never_reads_stale_tables(dev, xb, references, short, weight):
    """Utterance b runs 9 frames under a long list, is reset and given a short one between two steps; it then equals the short
    list alone, and the other utterances, which went on meanwhile, equal their undisturbed runs."""
    from conformer_amd.decode import beam_ctc_stream_finish
    W, N = C.BEAMS[0]
    T, b, k = xb.shape[1], 1, 9
    dec = decoder(None, W)
    long_list = ["A B C D", "C D E", "ÉA", "THE", "B C", "THÉ ßA", "É É", "CA B"]
    pack = lambda h: Hotwords(h).pack(GVOCAB, "|", (G_UNK,))             # noqa: E731
    assert len(pack(long_list)) > len(pack(list(short)))
    want = single(xb[:1], short, weight, None, W, N)
    assert best(want) != best(single(xb[:1], long_list, 6.0, None, W, N))
    undisturbed = references[False, W, N, False][0]
    st = stream_with_lists(dec, dev, T + k)
    st.set_hotwords(b, long_list, 6.0)
    st.step(xb[:, :k].contiguous())
    st.reset_slots([b])
    st.set_hotwords(b, short, weight)
    at = [0 if r == b else k for r in range(B)]
    st.step(chunk(xb, at, T - k), torch.full((B,), T - k, device=dev))
    last = [k if r == b else 0 for r in range(B)]
    st.step(chunk(xb, [T - k] * B, k), torch.tensor(last, device=dev))
    got = beam_ctc_stream_finish(st.state, N)
    same(got, want, b, "the short list after the long one")
    for r in range(B):
        if r != b:
            same(got, undisturbed[r], r, "the undisturbed utterances")


def test_a_table_of_exactly_the_reserved_size_stays_in_its_region(dev, xb):
    from conformer_amd.decode import beam_ctc_stream_finish
    W, N = C.BEAMS[0]
    T = xb.shape[1]
    full = ["A B C D E F G H"]                               # 8 distinct one-letter words: the bound's own worst case
    h = Hotwords(full)
    bounds = (len(h), h.code_points)
    n = reserved_bytes(*bounds, GVOCAB, "|", (G_UNK,))
    assert len(h.pack(GVOCAB, "|", (G_UNK,))) == n and n % 256 == 0
    dec = decoder(None, W, hotwords=None)
    with guarded_allocations() as guard:
        st = dec.stream(2, T, dev, hotword_rows=bounds)
        r = st.state.regions
        assert r.stride == n and r.buf.numel() == 2 * n
        before = r.buf[:n].clone()
        st.set_hotwords(1, full, 4.0)                         # the LAST region: one byte more would leave the buffer
        st.step(xb[:2].contiguous())
        got = beam_ctc_stream_finish(st.state, N)
        bad = guard.check()
    assert guard.allocs and not bad, bad
    assert torch.equal(r.buf[:n], before)                    # the neighbour region holds the empty table still
    assert torch.equal(r.buf[n:].cpu(), torch.from_numpy(h.pack(GVOCAB, "|", (G_UNK,))))
    same(got, single(xb[:1], full, 4.0, None, W, N), 1, "full region")
    same(got, single(xb[:1], [], 0.0, None, W, N), 0, "its neighbour")
    with pytest.raises(ValueError, match="max_code_points=8"):
        st.reset(), st.set_hotwords(0, ["AB C D E F G H I"])
    with pytest.raises(ValueError, match="max_phrases=1"):
        st.set_hotwords(0, ["A", "B"])


# ---- SlotTranscriber ---------------------------------------------------------------------------------------------------------

# (the tiny random model spells little but "md": every list holds a short word that a weight of this size pulls in)
SLOT_LISTS = {0: (["ab", "c d"], 6.0), 1: (["e", "nn"], 9.0), 2: ((), 2.0)}
REOPEN = (["d", "ab c"], 8.0)
FRAMES = [[64, 40, 0], [33, 64, 64], [64, 5, 30], [7, 64, 64], [64, 0, 64], [40, 64, 1]]


def slot_decoder(hotwords=None, weight=3.0):
    return BeamCTCDecoder(VOCAB, 0, skip_ids=(16,), beam_width=16, hotwords=hotwords, hotword_weight=weight)


def drive_slots(tr, dev, lists, reopen=None, segment_at=None, seed=9):
    """FRAMES on three slots (slot 2 opens before step 1; slot 1 is closed after step 2 and opened again with `reopen`):
    per slot the list of its utterances (text, logits)."""
    g = torch.Generator().manual_seed(seed)
    S = tr.S
    rows = {s: [] for s in range(S)}
    done = {s: [] for s in range(S)}
    opened = {s: False for s in range(S)}

    def close(s, how):
        done[s].append((how(s), torch.cat(rows[s]) if rows[s] else None))
        rows[s] = []

    for s in (0, 1):
        if s in lists:
            tr.open(s, *lists[s]), opened.update({s: True})
    for i, fr in enumerate(FRAMES):
        if i == 1 and 2 in lists:
            tr.open(2, *lists[2]), opened.update({2: True})
        fr = [f if opened[s] else 0 for s, f in enumerate(fr[:S])]
        logits, k = tr.step(torch.randn(S, 80, 64, generator=g).mul(3.0).to(dev), fr)
        for s in range(S):
            if k[s]:
                rows[s].append(logits[s, :k[s]].clone())
        if i == 2 and reopen is not None and opened.get(1):
            close(1, tr.close)
            tr.open(1, *reopen)
        if segment_at == i and opened.get(0):
            close(0, tr.segment)                              # the slot keeps its list
    for s in range(S):
        if opened[s]:
            close(s, tr.close)
    return done


def test_slot_transcriber_lists_per_slot(dev):
    from conformer_amd.slots import SlotTranscriber
    m = _tiny_model(71, dev)
    dec = slot_decoder(["c", "ab"], 3.0)
    tr = SlotTranscriber(m, dec, 3, 800, slot_hotwords=(4, 12))
    done = drive_slots(tr, dev, SLOT_LISTS, reopen=REOPEN, segment_at=3)
    plain = slot_decoder()
    every = list(SLOT_LISTS.values()) + [REOPEN]
    for s, utts in done.items():
        assert len(utts) == {0: 2, 1: 2, 2: 1}[s]
        for j, (text, logits) in enumerate(utts):
            h, w = REOPEN if (s, j) == (1, 1) else SLOT_LISTS[s]
            want = slot_decoder(list(h), w)(logits[None])[0]
            print(f"slot {s} utterance {j}: {want!r}; without hotwords {plain(logits[None])[0]!r}")
            if len(h):
                # the reference alone tells this list from no list and from the other slots' lists
                assert want != plain(logits[None])[0], (s, j)
                assert all(want != slot_decoder(list(h2), w2)(logits[None])[0] for h2, w2 in every if (h2, w2) != (h, w)), (s, j)
            assert text == want, (s, j, text, want)
    # None: the decoder's own list and weight
    tr.open(0)
    g = torch.Generator().manual_seed(4)
    logits, k = tr.step(torch.randn(3, 80, 64, generator=g).mul(3.0).to(dev), [64, 0, 0])
    assert tr.close(0) == dec(logits[:1, :k[0]])[0]
    with pytest.raises(ValueError, match="max_phrases=4"):
        tr.open(0, ["a", "b", "c", "d", "e"])
    assert not tr.is_open[0]
    with pytest.raises(ValueError, match="slot_hotwords"):
        SlotTranscriber(m, dec, 3, 800).open(0, ["a"])


@pytest.mark.parametrize("mode", ["max_pending", "times"])
def test_slot_transcriber_modes_against_a_single_slot_with_the_list_at_construction(dev, mode):
    from conformer_amd.slots import SlotTranscriber
    m = _tiny_model(71, dev)
    kw = dict(left_context=16, max_chunk_mel_frames=64, max_pending=12) if mode == "max_pending" else dict(times=True)
    T = None if mode == "max_pending" else 800

    def run(tr, slots, lists):
        """FRAMES on the mel columns of `slots`; per slot (committed tokens, final text) or its final Words"""
        g = torch.Generator().manual_seed(9)
        for i in range(len(slots)):
            tr.open(i, *lists[i]) if lists else tr.open(i)
        popped = [[] for _ in slots]
        for fr in FRAMES:
            x = torch.randn(3, 80, 64, generator=g).mul(3.0).to(dev)
            tr.step(x[slots].contiguous(), [fr[s] for s in slots])
            if mode == "max_pending":
                for i, ids in tr.pop_committed().items():
                    popped[i] += ids
        if mode == "max_pending":
            return [(popped[i], tr.close(i)) for i in range(len(slots))]
        return [tr.close_words(i) for i in range(len(slots))]

    def agree(a, b):
        if mode == "max_pending":
            return a == b
        # Word.score is a mean of fp32 log-probabilities and three slots may tile the GEMMs differently from one (the slot
        # objects agree to GEMM rounding): the words and their frames are exact, the scores agree to 1e-4
        return [(w.text, w.start_frame, w.end_frame) for w in a] == [(w.text, w.start_frame, w.end_frame) for w in b] and \
            all(abs(u.score - v.score) <= 1e-4 for u, v in zip(a, b))

    lists = [SLOT_LISTS[s] for s in range(3)]
    got = run(SlotTranscriber(m, slot_decoder(["c", "ab"], 3.0), 3, T, slot_hotwords=(4, 12), **kw), [0, 1, 2], lists)
    plain = run(SlotTranscriber(m, slot_decoder(), 3, T, **kw), [0, 1, 2], None)
    for s, (h, w) in enumerate(lists):
        want = run(SlotTranscriber(m, slot_decoder(list(h), w), 1, T, **kw), [s], None)[0]
        assert agree(got[s], want), (mode, s, got[s], want)
    assert not agree(got[0], plain[0]) or not agree(got[1], plain[1])


# ---- long form -----------------------------------------------------------------------------------------------------------------

def test_long_form_lists_follow_their_recordings(dev):
    from conformer_amd.longform import Transcriber
    m = _tiny_model(71, dev)
    g = torch.Generator().manual_seed(3)
    audios = [torch.randn(80, n, generator=g).mul(3.0).to(dev) for n in (150, 403, 64)]     # grouped longest first: 1, 0, 2
    lists = [(["ab", "c d"], 6.0), (["e", "nn"], 9.0), (["d", "ab c"], 8.0)]
    mk = lambda dec, **kw: Transcriber(m, dec, window_seconds=0.64, overlap_seconds=0.24, batch_windows=2, **kw)   # noqa: E731
    tr = mk(slot_decoder(["c"], 3.0), times=True)
    got = tr.transcribe(audios, hotwords=[h for h, _ in lists], hotword_weight=[w for _, w in lists])
    plain = mk(slot_decoder()).transcribe(audios)
    for i, (h, w) in enumerate(lists):
        want = mk(slot_decoder(h, w), times=True).transcribe(audios)[i]
        assert got[i].text == want.text and got[i].words == want.words, i
        others = [mk(slot_decoder(*lists[j])).transcribe(audios)[i].text for j in range(3) if j != i]
        assert want.text != plain[i].text or any(want.text != o for o in others), i
    assert [t.text for t in got] != [t.text for t in plain]
    with pytest.raises(ValueError, match="one entry per recording"):
        tr.transcribe(audios, hotwords=[["a"]])
