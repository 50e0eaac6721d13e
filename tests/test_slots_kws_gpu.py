"""Keyword spotting wired into the transcribers, on the MI355X: SlotTranscriber(keywords=...) on the tiny model and the schedule
of the endpointing tests, and Transcriber.spot on the tiny long-form pipeline.  The yardstick is kws.spot_keywords on the very
logits the transcribers produced (tests/test_kws_gpu.py holds that against the restatement): every comparison is exact."""
import sys

import pytest
import torch

import conformer_amd
from conformer_amd import _lib
from conformer_amd.align import CTCAligner
from conformer_amd.decode import BeamCTCDecoder
from conformer_amd.kws import Keywords, spot_keywords
from conformer_amd.longform import Transcriber
from tests.test_endpoint_gpu import SCHED, SEGMENTS, VOCAB, _tiny_model

pytestmark = pytest.mark.gpu

PHRASES = ["a", "b", "ab", "c d", "nn"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _decoder():
    return BeamCTCDecoder(VOCAB, 0, skip_ids=(16,), beam_width=16)


def _keywords(dec, threshold=8.0):
    return Keywords(PHRASES, CTCAligner.from_decoder(dec), threshold=threshold)


def _drive(tr, dev, pop_after=()):
    """SCHED with SEGMENTS: per slot its texts, the logits of all its frames since open(s), and the detections popped"""
    g = torch.Generator().manual_seed(9)
    S = 3
    rows = {s: [] for s in range(S)}
    texts = {s: [] for s in range(S)}
    popped = {s: [] for s in range(S)}
    tr.open(0), tr.open(1)
    for i, fr in enumerate(SCHED):
        if i == 2:
            tr.open(2)
        logits, k = tr.step(torch.randn(S, 80, 64, generator=g).mul(3.0).to(dev), fr)
        for s in range(S):
            if k[s]:
                rows[s].append(logits[s, :k[s]].clone())
        if i in pop_after:
            for s, found in tr.keywords().items():
                popped[s] += found
        for s in SEGMENTS.get(i, []):
            texts[s].append(tr.segment(s))
    for s in range(S):
        texts[s].append(tr.close(s))
    return texts, {s: torch.cat(r) for s, r in rows.items()}, popped


def test_slot_transcriber_keywords_equal_spot_keywords_on_the_slots_own_logits(dev):
    from conformer_amd.slots import SlotTranscriber
    m, dec = _tiny_model(71, dev), _decoder()
    kw = _keywords(dec)
    assert kw.tokens == [[1], [2], [1, 2], [3, 15, 4], [14, 14]] and kw.blank_id == 0
    tr = SlotTranscriber(m, dec, 3, 800, keywords=kw, max_detections=256)
    texts, rows, popped = _drive(tr, dev, pop_after=(1, 2, 4, 6))
    assert not any(tr.is_open) and tr.spotter.lost == [0, 0, 0]
    total = 0
    for s in range(3):
        want = spot_keywords(rows[s], kw, frame_seconds=0.04)[0]
        got = sorted(popped[s] + tr.close_keywords(s), key=lambda d: (d.end_frame, d.keyword))
        assert got == want, s                                   # segment(s) did not arm the spotter again: times from open(s)
        assert all(0 <= d.start_frame < d.end_frame <= len(rows[s]) and d.end == d.end_frame * 0.04 for d in got)
        total += len(got)
    assert total >= 3 and any(popped.values())
    assert tr.close_keywords(0) == []                           # flushed: armed again
    with pytest.raises(ValueError, match="outside"):
        tr.close_keywords(3)
    with pytest.raises(ValueError, match="kws.Keywords or None"):
        SlotTranscriber(m, dec, 3, 800, keywords=PHRASES)
    with pytest.raises(ValueError, match="blank"):
        SlotTranscriber(m, dec, 3, 800, keywords=Keywords([[1]], blank_id=5, vocab_size=len(VOCAB), threshold=1.0))


def test_without_keywords_nothing_is_imported_or_launched_and_nothing_changes(dev, monkeypatch):
    from conformer_amd.slots import SlotTranscriber
    m, dec = _tiny_model(71, dev), _decoder()
    kw = _keywords(dec)
    _drive(SlotTranscriber(m, dec, 3, 800), dev)                               # the model's one-time packs, before any count
    called = []
    call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: called.append(name) or call(name, *a))
    with_kw = _drive(SlotTranscriber(m, dec, 3, 800, keywords=kw), dev)
    names_with = list(called)
    del called[:]
    monkeypatch.setitem(sys.modules, "conformer_amd.kws", None)                # an import of it would raise ImportError
    monkeypatch.delattr(conformer_amd, "kws")
    tr = SlotTranscriber(m, dec, 3, 800)
    assert tr.spotter is None
    without = _drive(tr, dev)
    names_without = list(called)
    with pytest.raises(RuntimeError, match="keywords="):
        tr.keywords()
    with pytest.raises(RuntimeError, match="keywords="):
        tr.close_keywords(0)
    with pytest.raises(ImportError):
        SlotTranscriber(m, dec, 3, 800, keywords=kw)
    monkeypatch.undo()
    assert with_kw[0] == without[0] and all(torch.equal(with_kw[1][s], without[1][s]) for s in range(3))
    assert not [n for n in names_without if "kws" in n]
    assert [n for n in names_with if "kws" not in n] == names_without         # two more launches per step, nothing else
    assert [n for n in names_with if "kws" in n] == ["cfm3_kws_rowmax_f32", "cfm3_kws_scan_f32"] * len(SCHED)


def test_transcriber_spot_is_spot_keywords_on_the_recordings_logits(dev):
    m, dec = _tiny_model(71, dev), _decoder()
    kw = _keywords(dec)
    tr = Transcriber(m, dec, window_seconds=0.64, overlap_seconds=0.24, batch_windows=2)
    g = torch.Generator().manual_seed(3)
    audios = [torch.randn(80, n, generator=g).mul(3.0).to(dev) for n in (150, 403, 64)]
    got = tr.spot(audios, kw)
    want = [None] * 3
    groups = 0
    for group, n, _, logits, lengths in tr._group_logits(audios, None):
        found = spot_keywords(logits, kw, lengths, tr.frame_seconds)
        groups += 1
        for k, i in enumerate(group):
            want[i] = found[k]
            assert all(d.end_frame <= n[k] for d in found[k])
    assert got == want and groups == 2 and sum(len(w) for w in want) >= 3
    assert tr.spot([], kw) == []
    with pytest.raises(ValueError, match="kws.Keywords"):
        tr.spot(audios, PHRASES)
