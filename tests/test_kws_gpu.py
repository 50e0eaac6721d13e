"""Keyword spotting on the MI355X (conformer_amd/kws.py, cfm3_kws_rowmax_f32 and cfm3_kws_scan_f32).

The numpy float32 restatement (tests/kws_restatement.py) is the yardstick and the comparison is EXACT: the arithmetic is one
max chain, one subtraction and one add per state and frame, nothing is contracted and fp32 subnormals are kept, so every
integer must be identical and every float compares with ==, state words bit by bit.  No test row holds zeros of both signs.
Rows behind a slot's k are poisoned with NaN in every test."""
import math

import numpy as np
import pytest
import torch

from conformer_amd import _lib
from conformer_amd.kws import RING_FRAMES, Detection, Keywords, StreamingKeywordSpotter, spot_keywords
from tests import kws_restatement as R

pytestmark = pytest.mark.gpu

BLANK = 0
NEG_BITS = int(np.float32(-np.inf).view(np.int32))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_CASES: dict = {}


def case(V, T=67):
    """(keyword token lists, per slot its planted logits (T_b, V)) for a vocabulary of V; computed once per (V, T).
    Six keywords over three groups: 32 tokens (lanes 0 .. 62 of group 0), one token (lane 63 of group 0, next to the long
    one's last state), two equal tokens, A and B of two tokens each in adjacent lanes, and 31 tokens (a group of its own).
    Slot 0 of T = 67 holds A then B back to back (A's last state is at score 0 on the frame B starts: a shift that leaked across
    the border would hand B A's start), the repeated pair, and the long keyword followed at once by the one-token keyword."""
    if (V, T) in _CASES:
        return _CASES[(V, T)]
    if V == 2:
        kws = [[1] * 32, [1], [1, 1], [1, 1, 1], [1] * 4, [1] * 31]
        plants = [(2, R.spell([1] * 32, BLANK))]                           # 1 0 1 0 ... : 63 frames, every keyword occurs
    else:
        long = list(range(1, 33))
        kws = [long, [40], [41, 41], [42, 43], [44, 45], long[1:]]
        plants = [(0, [42, 43, 44, 45]), (5, R.spell([41, 41], BLANK)), (10, long + [40])]
    ks = (T, 0, {67: 33, 2: 1, 1: 1}[T])
    slots = [R.peaky(100 * V + b, 67, V, BLANK, plants)[:k] for b, k in enumerate(ks)]
    _CASES[(V, T)] = (kws, slots)
    return kws, slots


_RUNS: dict = {}


def restated(V, T, b, thresholds):
    """the restatement's Stream of slot b of case(V, T), run once"""
    if (V, T, b) not in _RUNS:
        kws, slots = case(V, T)
        _RUNS[(V, T, b)] = R.run(slots[b], kws, BLANK, thresholds)
    return _RUNS[(V, T, b)]


def feed(sp, slots, parts, dev):
    """slots: per slot its (T_b, V) float32 frames; parts: per slot the frame counts of the steps.  Rows behind k[b] hold NaN."""
    pos = [0] * len(slots)
    for i in range(len(parts[0])):
        ks = [p[i] for p in parts]
        x = torch.full((len(slots), max(max(ks), 1), slots[0].shape[1]), math.nan)
        for b, f in enumerate(slots):
            x[b, :ks[b]] = torch.from_numpy(f[pos[b]:pos[b] + ks[b]])
            pos[b] += ks[b]
        sp.step(x.to(dev), torch.tensor(ks, dtype=torch.int64, device=dev))
    assert pos == [len(f) for f in slots]


def group_rows(stream, kw, g):
    """the rows the kernel appends for group g: the restatement's emissions of the group's keywords, in their order"""
    mine = {q for q, gg, _ in kw.packing if gg == g}
    return [[q, s, e, int(np.float32(sc).view(np.int32))] for q, s, e, sc in stream.emissions if q in mine]


def check_against(sp, kw, streams, skip=()):
    state, det, counts = sp.state.cpu().numpy(), sp.detections.cpu().numpy(), sp.counts.cpu().numpy()
    for b, st in enumerate(streams):
        if b in skip:
            continue
        for g in range(kw.G):
            want = R.state_words(st, kw.packing, g)
            if not np.array_equal(state[b, g], want):                      # (the words that differ, before the assertion)
                rows, lanes = np.nonzero(state[b, g] != want)
                print(f"slot {b} group {g}: {len(rows)} state words differ, (row, lane, got, want): "
                      f"{[(int(r), int(l), int(state[b, g, r, l]), int(want[r, l])) for r, l in zip(rows[:12], lanes[:12])]}")
            assert np.array_equal(state[b, g], want), (b, g)
            rows = group_rows(st, kw, g)
            assert counts[b, g] == len(rows) and det[b, g, :len(rows)].tolist() == rows, (b, g)


# ---- the row maximum alone -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [2, 63, 64, 65, 370])
def test_rowmax_alone(dev, V):
    rng = np.random.default_rng(V)
    S, k_max, ks = 3, 9, [9, 0, 5]
    x = (rng.standard_normal((S, k_max, V)) * 3).astype(np.float32)
    x[0, 1, V - 1] = 50.0                                                  # the last column counts
    x[0, 2, rng.integers(0, V)] = math.nan
    x[0, 3], x[0, 4, 0], x[0, 5] = math.nan, math.inf, -math.inf
    x[2, 5:] = math.nan                                                    # behind k: never read
    out = torch.full((S + 2, k_max + 3), -7.25, device=dev)
    xd, kd = torch.from_numpy(x).to(dev), torch.tensor(ks, dtype=torch.int64, device=dev)
    _lib.call("cfm3_kws_rowmax_f32", xd.data_ptr(), k_max * V, V, kd.data_ptr(), k_max, V, out[1:, 1:].data_ptr(), k_max + 3, S,
              None)
    got = out.cpu().numpy()
    for b in range(S):
        want = np.array([R.row_max(r) for r in x[b, :ks[b]]], dtype=np.float32)
        mine = got[1 + b, 1:1 + ks[b]]
        assert np.array_equal(np.isnan(mine), np.isnan(want)) and np.array_equal(mine[~np.isnan(want)], want[~np.isnan(want)])
        mine[:] = -7.25
    assert (got == -7.25).all()                                            # nothing else was written
    assert np.isnan([R.row_max(r) for r in x[0, 3:6]]).all() and R.row_max(x[0, 1]) == 50.0


# ---- the DP --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 67])
@pytest.mark.parametrize("V", [2, 65, 370])
def test_dp_equals_the_restatement(dev, V, T):
    kws, slots = case(V, T)
    kw = Keywords(kws, blank_id=BLANK, vocab_size=V, threshold=1.0)
    assert kw.G == 3 and [p[1:] for p in kw.packing] == [(0, 0), (0, 63), (1, 0), (1, 3), (1, 3 + 2 * len(kws[3]) - 1), (2, 0)]
    sp = StreamingKeywordSpotter(3, kw, max_detections=128, device=dev)
    junk = torch.full_like(sp.state[1], 0x5A5A5A5A)
    sp.state[1], sp.detections[1], sp.counts[1] = junk, 0x5A5A5A5A, 0x5A5A5A5A
    feed(sp, slots, [[len(s)] for s in slots], dev)
    streams = [restated(V, T, b, kw.thresholds) for b in range(3)]
    check_against(sp, kw, streams, skip=(1,))
    assert (sp.state[1].cpu() == 0x5A5A5A5A).all() and (sp.detections[1].cpu() == 0x5A5A5A5A).all()      # k = 0: not touched
    assert (sp.counts[1].cpu() == 0x5A5A5A5A).all()
    if T == 67:                                                            # the restatement alone: the inputs exercise every keyword
        found = streams[0].finish()
        assert {d[0] for d in found} == set(range(6))
        assert all(len(group_rows(streams[0], kw, g)) < 128 for g in range(3))
        if V != 2:
            assert (3, 0, 1, 0.0) in found and (4, 2, 3, 0.0) in found and (0, 10, 41, 0.0) in found and (1, 42, 42, 0.0) in found
    got = [(d.keyword, d.start_frame, d.end_frame - 1, d.score) for d in sorted(sp.pop([0])[0] + sp.held(0),
                                                                               key=lambda d: (d.end_frame, d.keyword))]
    assert got == [(q, s, e, float(sc)) for q, s, e, sc in streams[0].finish()]
    sp.reset_slots([1])
    assert sp.pop([1])[1] == [] and sp.flush(1) == []


# ---- chunking ------------------------------------------------------------------------------------------------------------------
def test_any_chunking_gives_the_same_bits(dev):
    V, T = 65, 150
    kws, _ = case(V)
    plants = [(0, [42, 43, 44, 45]), (5, R.spell([41, 41], BLANK)), (10, kws[0] + [40]), (60, [42, 43]), (63, kws[0]), (100, [40]),
              (110, [44, 45, 44, 45]), (120, [41, 41, 0, 41])]
    x = [R.peaky(150 + b, T, V, BLANK, plants)[:n] for b, n in enumerate((T, 0, 71))]
    kw = Keywords(kws, blank_id=BLANK, vocab_size=V, threshold=1.0)
    assert RING_FRAMES == 8                                               # steps of 1 and 7 frames are below the ring, 64 and 65 above
    outs = []
    for cuts in ([1, 7, 64, 65, 13], [150]):
        parts = []
        for f in x:
            left, mine = len(f), []
            for c in cuts:
                mine.append(min(c, left))
                left -= mine[-1]
            parts.append(mine)
        sp = StreamingKeywordSpotter(3, kw, max_detections=64, device=dev)
        feed(sp, x, parts, dev)
        outs.append((sp.state.cpu(), sp.detections.cpu(), sp.counts.cpu()))
        last = sp
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    streams = [R.run(f, kws, BLANK, kw.thresholds) for f in x]
    check_against(last, kw, streams)
    assert int(outs[0][2][0].sum()) >= 8 and (outs[0][0][1, :, 0] == NEG_BITS).all() and outs[0][0][0, 0, 6, 0] == T


# ---- special values ------------------------------------------------------------------------------------------------------------
def test_special_values(dev):
    V, T = 65, 67
    kws, slots = case(V)
    x = slots[0].copy()
    x[0, 42] = math.nan            # a NaN on a label: A's first frame
    x[6, 7] = math.nan             # a NaN elsewhere in the row
    x[20] = math.nan               # a row of NaN: a BREAK in the middle of the long keyword's occurrence
    x[50, 3] = math.inf            # a +inf entry
    x[55] = -math.inf              # a row of -inf
    kw = Keywords(kws, blank_id=BLANK, vocab_size=V, threshold=1.0)
    sp = StreamingKeywordSpotter(1, kw, device=dev)
    feed(sp, [x], [[T]], dev)
    st = R.run(x, kws, BLANK, kw.thresholds)
    check_against(sp, kw, [st])
    rowmax = sp.rowmax.cpu().numpy()[0]
    assert np.isnan(rowmax[[20, 50, 55]]).all() and np.array_equal(rowmax[:20], np.array(st.rowmax[:20]))
    found = st.finish()
    assert found and not [d for d in found if d[1] <= 20 <= d[2]]          # no detection spans the BREAK
    assert not [d for d in found if d[0] in (0, 5)] and (4, 2, 3, 0.0) in found and (2, 5, 7, 0.0) in found
    assert not [d for d in found if d[0] == 3 and d[1] == 0]


# ---- bounds --------------------------------------------------------------------------------------------------------------------
def test_sentinels_around_every_buffer(dev):
    """the object runs on the middle rows of larger tensors: a guard slot in front of and behind state, detections, counts and
    the row maxima keeps its bytes"""
    V, T = 65, 67
    kws, slots = case(V)
    kw = Keywords(kws, blank_id=BLANK, vocab_size=V, threshold=1.0)
    S = 3
    sp = StreamingKeywordSpotter(S, kw, max_detections=8, device=dev)
    big = {}
    for name in ("state", "detections", "counts"):
        t = getattr(sp, name)
        big[name] = torch.full((S + 2, *t.shape[1:]), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        big[name][1:S + 1] = t
        setattr(sp, name, big[name][1:S + 1])
    big["rowmax"] = torch.full((S + 2, T), -7.25, device=dev)
    sp._buffers[T] = big["rowmax"][1:S + 1]
    feed(sp, slots, [[len(s)] for s in slots], dev)
    torch.cuda.synchronize()
    for name in ("state", "detections", "counts"):
        assert (big[name][[0, S + 1]].cpu() == 0x5A5A5A5A).all(), name
    rm = big["rowmax"].cpu()
    assert (rm[[0, 2, S + 1]] == -7.25).all() and (rm[3, 33:] == -7.25).all() and torch.isfinite(rm[1]).all()
    check_against(sp, kw, [restated(V, T, b, kw.thresholds) for b in range(3)])
    det, counts = sp.detections.cpu(), sp.counts.cpu()
    for g in range(3):
        assert (det[0, g, int(counts[0, g]):] == 0).all()                  # nothing behind the emitted rows


def test_overflow_counts_on_and_writes_nothing_past_the_buffer(dev):
    """five emissions of one group into max_detections = 2"""
    V = 12
    kws = [[3], [4, 5]]
    plants = [(2, [3]), (5, [4, 5]), (9, [3]), (12, [4, 5]), (15, [3])]
    x = R.peaky(5, 20, V, BLANK, plants)
    kw = Keywords(kws, blank_id=BLANK, vocab_size=V, threshold=1.0)
    st = R.run(x, kws, BLANK, kw.thresholds)
    assert len(st.emissions) == 5 and not st.held()
    sp = StreamingKeywordSpotter(1, kw, max_detections=2, device=dev)
    guard = torch.full((2 * 4 + 16,), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    guard[:8] = 0
    sp.detections = guard[:8].view(1, 1, 2, 4)
    feed(sp, [x], [[20]], dev)
    assert sp.counts.cpu().tolist() == [[5]]
    assert (guard.cpu()[8:] == 0x5A5A5A5A).all()
    assert guard.cpu()[:8].view(2, 4).tolist() == group_rows(st, kw, 0)[:2]
    got = sp.pop()[0]
    assert [(d.keyword, d.start_frame, d.end_frame) for d in got] == [(0, 2, 3), (1, 5, 7)] and sp.lost == [3]
    assert sp.counts.cpu().tolist() == [[0]] and sp.pop()[0] == [] and sp.lost == [3]
    with pytest.raises(RuntimeError, match="did not fit"):
        spot_keywords(torch.from_numpy(x).to(dev), kw, max_detections=2)


# ---- the rest of the interface -------------------------------------------------------------------------------------------------
def test_a_step_is_capturable_and_replays(dev):
    V = 65
    kws, slots = case(V)
    kw = Keywords(kws, blank_id=BLANK, vocab_size=V, threshold=1.0)
    first, second = torch.from_numpy(slots[0][:32]).to(dev)[None], torch.from_numpy(slots[0][32:64]).to(dev)[None]
    k = torch.tensor([32], dtype=torch.int64, device=dev)
    eager = StreamingKeywordSpotter(1, kw, device=dev)
    eager.step(first, k)
    eager.step(second, k)
    fresh = StreamingKeywordSpotter(1, kw, max_chunk_frames=32, device=dev)
    static = first.clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        fresh.step(static, k)                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(stream)
    fresh.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fresh.step(static, k)
    fresh.reset()
    graph.replay()
    static.copy_(second)
    graph.replay()
    torch.cuda.synchronize()
    for name in ("state", "detections", "counts"):
        assert torch.equal(getattr(fresh, name), getattr(eager, name)), name
    assert int(eager.state[0, 0, 6, 0]) == 64 and int(eager.counts.sum()) >= 3


def test_offline_pop_and_flush_agree_with_each_other_and_the_restatement(dev):
    V, T = 65, 67
    kws, slots = case(V)
    al_vocab = ["<b>"] + [chr(0x100 + i) for i in range(1, V)]
    from conformer_amd.align import CTCAligner
    kw = Keywords(["".join(al_vocab[i] for i in k) for k in kws], CTCAligner(al_vocab, BLANK, delim_token="|"), threshold=1.0)
    assert kw.tokens == kws
    want = []
    for b in range(3):
        fin = restated(V, T, b, kw.thresholds).finish()
        want.append([Detection(q, kw.phrases[q], s * 0.02, (e + 1) * 0.02, float(sc), s, e + 1) for q, s, e, sc in fin])
    x = torch.full((3, T, V), math.nan)
    for b, f in enumerate(slots):
        x[b, :len(f)] = torch.from_numpy(f)
    lengths = torch.tensor([len(f) for f in slots], dtype=torch.int64, device=dev)
    assert spot_keywords(x.to(dev), kw, lengths, 0.02) == want
    assert spot_keywords(torch.from_numpy(slots[0]).to(dev), kw, frame_seconds=0.02) == [want[0]]
    sp = StreamingKeywordSpotter(3, kw, 0.02, device=dev)
    popped = [[] for _ in range(3)]
    at = 0
    for n in (5, 20, 42):                                                  # pops between the steps, the flush at the end
        sp.step(x[:, at:at + n].to(dev), (lengths - at).clamp(0, n))
        at += n
        for b, found in enumerate(sp.pop()):
            popped[b] += found
    assert any(popped) and sp.lost == [0, 0, 0]
    for b in range(3):
        assert sorted(popped[b] + sp.flush(b), key=lambda d: (d.end_frame, d.keyword)) == want[b]
    assert (sp.state.cpu() == sp._armed.cpu()).all() and sp.counts.cpu().abs().sum() == 0      # flush arms the slots again


def test_host_tensors_and_wrong_shapes_are_refused(dev):
    kw = Keywords([[1, 2]], blank_id=BLANK, vocab_size=8, threshold=1.0)
    sp = StreamingKeywordSpotter(2, kw, device=dev)
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        sp.step(torch.zeros(2, 4, 8))
    with pytest.raises(_lib.ConformerHipError, match="float32"):
        sp.step(torch.zeros(2, 4, 8, dtype=torch.float16, device=dev))
    with pytest.raises(_lib.ConformerHipError, match="int64"):
        sp.step(torch.zeros(2, 4, 8, device=dev), torch.tensor([4, 4], dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="vocabulary of 8"):
        sp.step(torch.zeros(2, 4, 9, device=dev))
    with pytest.raises(ValueError, match="2 frame counts"):
        sp.step(torch.zeros(2, 4, 8, device=dev), [4])
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        StreamingKeywordSpotter(2, kw, device="cpu")
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        spot_keywords(torch.zeros(1, 4, 8), kw)
    with pytest.raises(ValueError, match="must be a Keywords"):
        StreamingKeywordSpotter(2, [[1, 2]], device=dev)
    assert (sp.state.cpu() == sp._armed.cpu()).all()
