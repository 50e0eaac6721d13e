"""Confidence on the MI355X (conformer_amd/confidence.py, include/conformer_hip_confidence.h).

Frame values against the float64 restatement (tests/confidence_restatement.py) on the fp32-cast inputs within 1e-4 absolute, the
project's end-to-end fp32 parity bar (the same formulas in numpy float32 stay within 2.6e-5 at alpha = 1 -+ 1/16 and 5e-6
elsewhere, so the bar sits about four above plain fp32 and far below a wrong normaliser or a dropped lane); ids exactly; any
chunking and the ring bit for bit; the span kernel on synthetic histories; the greedy spans; both transcribers end to end."""
import math

import numpy as np
import pytest
import torch

from conformer_amd import _lib
from conformer_amd import confidence as C
from conformer_amd.align import Word, ctc_forced_align
from conformer_amd.confidence import (AGGREGATIONS, METHODS, ConfidenceConfig, StreamingConfidence, alignment_confidence,
                                      frame_confidence, greedy_ctc_confidence, span_confidence, word_confidence)
from conformer_amd.decode import BeamCTCDecoder, greedy_ctc_decode
from tests import confidence_restatement as R
from tests.test_endpoint_gpu import SCHED, SEGMENTS, VOCAB, _tiny_model
from tests.test_write_guard_gpu import GuardedTorch

pytestmark = pytest.mark.gpu

BOUND = 1e-4
ALPHAS = (1 / 16, 0.33, 15 / 16, 17 / 16, 2.0, 8.0)
MEASURES = [("max_prob", 0.33), ("entropy", 0.33)] + [(m, a) for m in ("tsallis", "renyi") for a in ALPHAS]
RANKING = [("max_prob", 0.33), ("entropy", 0.33), ("tsallis", 0.33), ("tsallis", 2.0), ("renyi", 0.33), ("renyi", 2.0)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _logits(B, T, V, seed):
    """(B, T, V) fp32: Gaussian logits at scale 0.1, 1 or 10 by row, clipped to |x| <= 30, one logit raised by 8 in every
    fourth row."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B * T, V)) * np.array([0.1, 1.0, 10.0])[np.arange(B * T) % 3][:, None]
    rows = np.arange(0, B * T, 4)
    x[rows, rng.integers(0, V, len(rows))] += 8.0
    return torch.from_numpy(np.clip(x, -30.0, 30.0).astype(np.float32).reshape(B, T, V))


def _bits(t):
    """fp32 -> its int32 bits (a NaN equals itself)"""
    return t.detach().cpu().contiguous().view(torch.int32)


def _same(a, b):
    return torch.equal(_bits(a), _bits(b))


def _cfg(method, alpha=0.33, aggregation="min", exclude_blank=True):
    return ConfidenceConfig(method, alpha, aggregation, exclude_blank)


# ---- frame values and ids ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [2, 5, 63, 64, 65, 512, 513, 1025])      # 512 | 513: a row in registers | walked from L1
def test_frame_values_and_ids_equal_the_restatement(dev, V):
    worst = {}
    for T in (1, 63, 64, 65, 130):
        x = _logits(3, T, V, seed=1000 * V + T)
        lengths = [T, T // 2, 0]
        if T == 130:                                        # two equal maxima: the lower index
            x[0, 5, V - 1] = x[0, 5, 0] = 30.0
        xd, ld = x.to(dev), torch.tensor(lengths, dtype=torch.int64, device=dev)
        greedy_ids = greedy_ctc_decode(xd, 0, 1, ld)[0].cpu()
        want_ids = [R.frames(x[b, :n].numpy(), "max_prob")[1] for b, n in enumerate(lengths)]
        for method, alpha in MEASURES:
            conf, ids = frame_confidence(xd, ld, _cfg(method, alpha))
            conf, ids = conf.cpu(), ids.cpu()
            for b, n in enumerate(lengths):
                want = R.frames(x[b, :n].numpy(), method, alpha)[0]
                got = conf[b, :n].double().numpy()
                assert np.isfinite(got).all() and (got >= 0).all() and (got <= 1).all()
                err = float(np.abs(got - want).max()) if n else 0.0
                worst[method, alpha] = max(worst.get((method, alpha), 0.0), err)
                assert ids[b, :n].tolist() == want_ids[b].tolist() == greedy_ids[b, :n].tolist()
                assert torch.isnan(conf[b, n:]).all() and (ids[b, n:] == -1).all()          # padding
        if T == 130:
            assert ids[0, 5] == 0
    for key, err in sorted(worst.items()):
        print(f"V={V} {key[0]} alpha={key[1]:.4f}: max |err| = {err:.3e}")
    assert max(worst.values()) <= BOUND, worst


def test_special_logits(dev):
    inf, nan = math.inf, math.nan
    x = torch.tensor([[[0.0, -inf, 0.0, 0.0],              # uniform over three of four
                       [2.0, -inf, -inf, -inf],             # one-hot
                       [0.0, nan, 1.0, 0.0],                # a NaN logit: NaN
                       [1.0, 3.0, 3.0, 0.0]]])              # two equal maxima: the lower index
    for method, alpha in RANKING:
        conf, ids = frame_confidence(x.to(dev), None, _cfg(method, alpha))
        conf = conf.cpu()[0]
        want = [R.frame_confidence(r.numpy(), method, alpha) for r in x[0]]
        assert not math.isnan(conf[0]) and abs(float(conf[0]) - want[0]) <= BOUND and conf[1] == 1.0
        assert math.isnan(conf[2]) and math.isnan(want[2])
        assert abs(float(conf[3]) - want[3]) <= BOUND
        assert ids.cpu()[0, [0, 1, 3]].tolist() == [0, 0, 1]
    # 16-bit logits are cast to fp32 first
    h = _logits(2, 9, 67, seed=3).to(dev).bfloat16()
    assert _same(frame_confidence(h)[0], frame_confidence(h.float())[0])


# ---- padding, rows behind k, guard bytes --------------------------------------------------------------------------------------------
def test_rows_behind_k_are_never_read_and_nothing_is_written_outside(dev, monkeypatch):
    """Every buffer confidence.py allocates is carved out of sentinel bytes (the idiom of tests/test_write_guard_gpu.py); the
    rows behind k[b] hold NaN and +-inf and change no bit of any output."""
    proxy = GuardedTorch()
    monkeypatch.setattr(C, "torch", proxy)
    V, T = 67, 70
    x = _logits(3, T, V, seed=17)
    lengths = [70, 33, 0]
    outs = []
    for fill in (0.0, math.nan, math.inf, -math.inf):
        y = x.clone()
        for b, n in enumerate(lengths):
            y[b, n:] = fill
        ld = torch.tensor(lengths, dtype=torch.int64, device=dev)
        conf, ids = frame_confidence(y.to(dev), ld, _cfg("entropy"))
        g = greedy_ctc_confidence(y.to(dev) if fill == 0.0 else x.to(dev), 0, 1, ld)
        sc = StreamingConfidence(3, 0, _cfg("renyi", 2.0, "mean"), history=64, device=dev)
        sc.step(y.to(dev), lengths)
        y2 = x[:, :40].clone()
        y2[1], y2[2, 7:] = fill, fill
        sc.step(y2.to(dev), [40, 0, 7])
        w = sc.spans(torch.tensor([[80, 100], [0, 20], [0, 3]], device=dev), torch.tensor([[110, 104], [33, 33], [7, 9]], device=dev),
                     torch.tensor([2, 2, 1], device=dev))
        outs.append((conf, ids.float(), sc.conf, sc.ids.float(), sc.total.float(), w, g.token_confidence))
    bad = proxy.check()
    assert len(proxy.allocs) >= 4 * 10 and not bad, f"{len(bad)} of {len(proxy.allocs)} buffers written outside: {bad[:5]}"
    for o in outs[1:]:
        assert all(_same(a, b) for a, b in zip(o, outs[0]))
    conf, _, ring, ring_ids, total, w, _ = outs[0]
    assert total.tolist() == [110, 33, 7]
    assert torch.isnan(conf.cpu()[1, 33:]).all() and torch.isnan(conf.cpu()[2]).all()
    assert torch.isnan(ring.cpu()[2, 7:]).all() and (ring_ids.cpu()[2, 7:] == -1).all()     # never written: as allocated
    assert not torch.isnan(w.cpu()[0]).any() and torch.isnan(w.cpu()[2, 1])


# ---- chunking and the ring ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [67, 513])
def test_any_chunking_and_the_ring_give_the_offline_bits(dev, V):
    S, T = 3, 150
    x = _logits(S, T, V, seed=29 + V).to(dev)
    cfg = _cfg("tsallis", 0.33, "mean")
    off_conf, off_ids = frame_confidence(x, None, cfg)
    hist = {}
    for name, parts, history in (("one", (150,), 200), ("cut", (1, 63, 64, 22), 200), ("ring", (1, 63, 64, 22), 64),
                                 ("lap", (150,), 64)):       # (lap: a step longer than the ring is fed in laps)
        sc = StreamingConfidence(S, 0, cfg, history=history, device=dev)
        t0 = 0
        for n in parts:
            sc.step(x[:, t0:t0 + n])                                           # (a view: its strides are the entry's pitches)
            t0 += n
        assert sc.total.tolist() == [T] * S
        hist[name] = sc
    for name in ("one", "cut"):
        assert _same(hist[name].conf[:, :T], off_conf) and torch.equal(hist[name].ids[:, :T], off_ids)
        assert torch.isnan(hist[name].conf[:, T:]).all()
    cols = torch.arange(T - 64, T, device=dev) % 64                                    # frame t sits at column t mod 64
    for name in ("ring", "lap"):
        assert _same(hist[name].conf[:, cols], off_conf[:, T - 64:]) and torch.equal(hist[name].ids[:, cols], off_ids[:, T - 64:])
    # spans: inside the history the offline bits, a start that has rolled out (< 150 - 64 = 86) NaN
    starts = torch.tensor([[86, 100, 85, 149]] * S, device=dev)
    ends = torch.tensor([[150, 131, 120, 150]] * S, device=dev)
    want = span_confidence(off_conf, off_ids, starts, ends, None, cfg, exclude_ids=(0,))
    got = hist["ring"].spans(starts, ends, torch.full((S,), 4, device=dev))
    assert _same(got[:, [0, 1, 3]], want[:, [0, 1, 3]]) and torch.isnan(got[:, 2]).all() and not torch.isnan(want).any()
    # reset_slots restarts one slot and leaves the others' bits alone
    sc = hist["cut"]
    before = (sc.conf.clone(), sc.ids.clone())
    sc.reset_slots([1])
    assert sc.total.tolist() == [T, 0, T] and torch.isnan(sc.conf[1]).all() and (sc.ids[1] == -1).all()
    sc.step(x[:, 10:15], [0, 5, 0])
    assert sc.total.tolist() == [T, 5, T] and _same(sc.conf[1, :5], off_conf[1, 10:15]) and torch.isnan(sc.conf[1, 5:]).all()
    assert _same(sc.conf[[0, 2]], before[0][[0, 2]]) and torch.equal(sc.ids[[0, 2]], before[1][[0, 2]])


def test_a_step_is_capturable(dev):
    S, V, c = 3, 67, 50
    frames = _logits(S, 3 * c, V, seed=41).to(dev)
    ks = [[50, 0, 7], [1, 50, 0], [50, 50, 50]]
    eager, sc = (StreamingConfidence(S, 0, history=128, device=dev) for _ in range(2))
    x, k = torch.zeros(S, c, V, device=dev), torch.zeros(S, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sc.step(x, k)                                                         # (warm-up outside the capture: k = 0, a no-op)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sc.step(x, k)
    for i, kk in enumerate(ks):
        x.copy_(frames[:, i * c:(i + 1) * c])
        k.copy_(torch.tensor(kk, device=dev))
        graph.replay()
        eager.step(frames[:, i * c:(i + 1) * c], kk)
    assert sc.total.tolist() == eager.total.tolist() == [101, 100, 57]
    assert _same(sc.conf, eager.conf) and torch.equal(sc.ids, eager.ids) and not torch.isnan(sc.conf[:, :57]).any()


# ---- the span kernel alone ------------------------------------------------------------------------------------------------------------
def test_the_span_kernel_on_synthetic_histories(dev):
    S, Rr = 2, 200
    rng = np.random.default_rng(7)
    conf = (0.5 + 0.5 * rng.random((S, Rr))).astype(np.float32)             # in [0.5, 1): a product of 129 stays normal
    ids = rng.integers(0, 5, (S, Rr)).astype(np.int64)
    total = [237, 150]                                                      # slot 0 has lapped: it holds frames 37 .. 236
    ids[1, 10:75] = 0                                                       # a stretch that is all "blank"
    conf[1, 100] = math.nan
    # slot 0: lengths 1, 63, 64, 65, 129 at starts off a multiple of 64; two across the seam (column 199 -> 0), the first
    # clamped to total; a start that has rolled out; an empty one; one clamped to [230, 237)
    spans0 = [(41, 42), (70, 133), (71, 135), (37, 102), (101, 230), (190, 255), (199, 201), (36, 50), (90, 90), (230, 300)]
    # slot 1: all "blank"; part "blank"; the NaN frame inside, just before the span and just behind it; clamped to total; one
    # frame; the NaN inside again; two that lie beyond n_spans
    spans1 = [(10, 75), (5, 80), (95, 101), (101, 130), (90, 100), (140, 170), (3, 4), (0, 150), (7, 71), (1, 2)]
    starts = torch.tensor([[a for a, _ in spans0], [a for a, _ in spans1]])
    ends = torch.tensor([[b for _, b in spans0], [b for _, b in spans1]])
    n_spans = [10, 8]                                                       # slot 1: the last two are beyond n_spans
    proxy = GuardedTorch()
    out_of = {}
    for agg in R.AGGREGATIONS:
        for excl in ((), (0, 1), (0, 1, 2, 3, 4)):                          # none, some, every id there is
            out = proxy.empty(S, len(spans0), dtype=torch.float32, device=dev)
            ex = torch.tensor(excl, dtype=torch.int32, device=dev) if excl else None
            args = [torch.from_numpy(conf).to(dev), torch.from_numpy(ids).to(dev), torch.tensor(total, device=dev),
                    starts.to(dev), ends.to(dev), torch.tensor(n_spans, device=dev)]
            _lib.call("cfm_confidence_spans_f32", args[0].data_ptr(), args[1].data_ptr(), args[2].data_ptr(), Rr,
                      args[3].data_ptr(), args[4].data_ptr(), args[5].data_ptr(), len(spans0), AGGREGATIONS[agg],
                      None if ex is None else ex.data_ptr(), len(excl), out.data_ptr(), S, None)
            got = out.cpu()
            out_of[agg, excl] = got
            for b in range(S):
                want = R.spans(conf[b].astype(np.float64), ids[b], total[b], Rr, starts[b].tolist(), ends[b].tolist(), n_spans[b],
                               agg, excl)
                for j, w in enumerate(want):
                    g = float(got[b, j])
                    if math.isnan(w):
                        assert math.isnan(g), (agg, excl, b, j)
                        continue
                    span = range(int(starts[b, j]), min(int(ends[b, j]), total[b]))
                    n = sum(ids[b, t % Rr] not in excl for t in span) or len(span)          # the frames that count
                    if agg in ("min", "max"):
                        assert g == w, (agg, excl, b, j)                    # a minimum is one of the fp32 values: bit for bit
                    else:
                        # an fp32 sum (product) of n terms, folded in any order, is within (n - 1) roundings of 2^-24 each
                        # of the exact one, and the mean's division adds one more: n 2^-23 (n 2^-22) leaves a factor two (four)
                        rel = n * (2.0 ** -23 if agg == "mean" else 2.0 ** -22)
                        assert abs(g - w) <= rel * abs(w), (agg, excl, b, j, g, w)
    assert not proxy.check()
    nan0 = [math.isnan(v) for v in out_of["mean", ()][0].tolist()]
    assert nan0 == [False] * 7 + [True, True, False]                        # rolled out, empty; [230, 300) is clamped to 237
    nan1 = [math.isnan(v) for v in out_of["mean", ()][1].tolist()]
    assert nan1 == [False, False, True, False, False, False, False, True, True, True]
    assert _same(out_of["min", (0, 1)][1, 0], out_of["min", ()][1, 0])       # all excluded: all frames count
    assert not _same(out_of["mean", (0, 1)][1, 1], out_of["mean", ()][1, 1])


# ---- greedy -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_lengths", [False, True])
@pytest.mark.parametrize("T", [1, 64, 65, 130])
def test_greedy_confidence_agrees_with_the_greedy_decoder(dev, T, use_lengths):
    B, V, pad, unk = 4, 6, 0, 5
    rng = np.random.default_rng(50 + T)
    x = _logits(B, T, V, seed=60 + T)
    x = x[:, torch.from_numpy(np.sort(rng.integers(0, T, T)))]               # frames repeat: runs of one id
    x[3, :, pad] = 100.0                                                     # an all-pad row
    lengths = torch.tensor([T, T // 2, max(T - 1, 0), T], dtype=torch.int64, device=dev) if use_lengths else None
    cfg = _cfg("entropy", aggregation="min")
    g = greedy_ctc_confidence(x.to(dev), pad, unk, lengths, cfg)
    frame_ids, tokens, counts = greedy_ctc_decode(x.to(dev), pad, unk, lengths)
    assert torch.equal(g.frame_ids, frame_ids) and torch.equal(g.tokens, tokens) and torch.equal(g.counts, counts)
    conf, ids = frame_confidence(x.to(dev), lengths, cfg)
    assert _same(g.frame_confidence, conf)
    fi, cf = frame_ids.cpu().numpy(), conf.cpu().double().numpy()
    some = 0
    for b in range(B):
        n = T if lengths is None else int(lengths[b])
        ws, we = R.greedy_spans(fi[b], pad, unk, n)
        assert g.token_start[b].tolist() == ws and g.token_end[b].tolist() == we
        cnt = int(counts[b])
        assert sum(s >= 0 for s in ws) == cnt
        assert [int(fi[b, s]) for s in ws[:cnt]] == tokens[b, :cnt].tolist() == R.greedy_tokens(fi[b], pad, unk, n)
        want = R.spans(cf[b], fi[b], n, T, ws, we, cnt, "min", (pad, unk))
        got = g.token_confidence[b].cpu().tolist()
        assert [math.isnan(v) for v in got] == [math.isnan(v) for v in want]
        assert got[:cnt] == want[:cnt]                                       # a minimum: bit for bit
        some += cnt
    assert some > 0 and int(counts[3]) == 0


def test_alignment_and_word_confidence_offline(dev):
    B, T, V, blank = 2, 40, 9, 0
    x = _logits(B, T, V, seed=77).to(dev)
    lengths = torch.tensor([40, 31], dtype=torch.int64, device=dev)
    targets = torch.tensor([[3, 4, 4, 2], [5, 1, 0, 0]], dtype=torch.int64, device=dev)
    al = ctc_forced_align(x, targets, blank, lengths, torch.tensor([4, 2], device=dev))
    cfg = _cfg("renyi", 2.0, "mean")
    conf, ids = frame_confidence(x, lengths, cfg)
    got = alignment_confidence(al, conf, ids, blank, cfg).cpu()
    cf, fi = conf.cpu().double().numpy(), ids.cpu().numpy()
    ts, te = al.token_start.cpu().tolist(), al.token_end.cpu().tolist()
    assert bool(al.ok.all())
    for b, n in enumerate((4, 2)):
        want = R.spans(cf[b], fi[b], T, T, ts[b], te[b], 4, "mean", (blank,))
        for j in range(n):                                                   # (an fp32 mean of at most te - ts frames)
            assert abs(float(got[b, j]) - want[j]) <= (te[b][j] - ts[b][j]) * 2.0 ** -23 * want[j]
    words = [[Word("a", 2, 9, 0.0, 0.0, 0.0), Word("b", 9, 40, 0.0, 0.0, 0.0)], [Word("c", 30, 35, 0.0, 0.0, 0.0)]]
    wc = word_confidence(words, conf, ids, blank, lengths, _cfg("renyi", 2.0, "max"))
    assert [len(w) for w in wc] == [2, 1]
    for b, ws in enumerate(words):
        for w, got_w in zip(ws, wc[b]):
            assert got_w == R.span(cf[b], fi[b], int(lengths[b]), T, w.start_frame, w.end_frame, "max", (blank,))
    assert word_confidence([[], []], conf, ids, blank) == [[], []]


# ---- ranking --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,alpha", RANKING)
def test_peaked_frames_rank_above_flat_ones(dev, method, alpha):
    x = torch.from_numpy(np.stack(R.ranking_frames())).to(dev)               # (2, 40, 67): peaked, flat
    cfg = _cfg(method, alpha, "mean", exclude_blank=False)
    conf, ids = frame_confidence(x, None, cfg)
    whole = torch.tensor([[0], [0]], device=dev), torch.tensor([[40], [40]], device=dev)
    mean = span_confidence(conf, ids, *whole, None, cfg).cpu()[:, 0].tolist()
    print(f"{method} alpha={alpha}: peaked {mean[0]:.4f} flat {mean[1]:.4f}")
    assert mean[0] - mean[1] >= 0.25, mean


# ---- the C entries' refusals ----------------------------------------------------------------------------------------------------------
def _status(name, good, **kw):
    try:
        _lib.call(name, *{**good, **kw}.values())
    except _lib.ConformerHipError as e:
        return int(str(e).rsplit("status ", 1)[1].rstrip(")"))
    return 0


def test_the_entries_refuse_before_any_launch(dev):
    S, k_max, V, Rr, L = 2, 3, 5, 8, 4
    x = torch.zeros(S, k_max, V, device=dev)
    k = torch.full((S,), k_max, dtype=torch.int64, device=dev)
    conf = torch.full((S, Rr), 0.25, device=dev)
    ids = torch.full((S, Rr), 7, dtype=torch.int64, device=dev)
    total = torch.tensor([1, 2], dtype=torch.int64, device=dev)
    starts, ends = torch.zeros(S, L, dtype=torch.int64, device=dev), torch.ones(S, L, dtype=torch.int64, device=dev)
    out = torch.full((S, L), 0.5, device=dev)
    ex = torch.zeros(8, dtype=torch.int32, device=dev)
    keep = [t.clone() for t in (conf, ids, total, out, starts)]
    C_ = _lib.CONSTANTS
    NULL, BAD, UNSUP = C_["CFM_ERR_NULL"], C_["CFM_ERR_BAD_SHAPE"], C_["CFM_ERR_UNSUPPORTED"]

    name = "cfm_confidence_frames_f32"
    good = dict(logits=x.data_ptr(), ld_slot=k_max * V, ld_row=V, k=k.data_ptr(), k_max=k_max, V=V, method=METHODS["tsallis"],
                alpha=0.33, conf=conf.data_ptr(), ids=ids.data_ptr(), total=total.data_ptr(), R=Rr, S=S, stream=None)
    assert list(good) == _lib.PARAMS[name]
    for p in ("logits", "k", "conf", "ids", "total"):
        assert _status(name, good, **{p: None}) == NULL, p
    for kw in (dict(S=0), dict(k_max=-1), dict(V=1), dict(R=0), dict(k_max=9, ld_slot=9 * V), dict(R=2), dict(ld_row=V - 1),
               dict(ld_slot=k_max * V - 1), dict(method=-1), dict(method=4), dict(alpha=1.0), dict(alpha=0.0), dict(alpha=1.03),
               dict(alpha=9.0), dict(alpha=math.nan), dict(method=METHODS["renyi"], alpha=0.05)):
        assert _status(name, good, **kw) == BAD, kw
    for kw in (dict(S=65535), dict(V=65537, ld_row=65537, ld_slot=k_max * 65537)):
        assert _status(name, good, **kw) == UNSUP, kw
    assert _status(name, good, k_max=0, logits=None, ld_slot=0) == 0          # nothing to do: no launch, no error
    assert _status(name, good, method=METHODS["entropy"], alpha=1.0, k_max=0) == 0      # (alpha ignored)

    name = "cfm_confidence_spans_f32"
    good = dict(conf=conf.data_ptr(), ids=ids.data_ptr(), total=total.data_ptr(), R=Rr, starts=starts.data_ptr(),
                ends=ends.data_ptr(), n_spans=k.data_ptr(), L=L, aggregation=AGGREGATIONS["min"], exclude_ids=ex.data_ptr(),
                n_exclude=1, out=out.data_ptr(), S=S, stream=None)
    assert list(good) == _lib.PARAMS[name]
    for p in ("conf", "ids", "total", "starts", "ends", "n_spans", "out", "exclude_ids"):
        assert _status(name, good, **{p: None}) == NULL, p
    for kw in (dict(S=0), dict(L=-1), dict(R=0), dict(aggregation=-1), dict(aggregation=4), dict(n_exclude=-1), dict(n_exclude=9)):
        assert _status(name, good, **kw) == BAD, kw
    assert _status(name, good, S=65536, L=32768) == UNSUP
    assert _status(name, good, L=0) == 0 and _status(name, good, L=0, exclude_ids=None, n_exclude=0) == 0

    name = "cfm_confidence_greedy_spans_i64"
    good = dict(frame_ids=ids.data_ptr(), lengths_or_null=None, token_start=starts.data_ptr(), token_end=ends.data_ptr(), B=S, T=L,
                pad_id=0, unk_id=1, stream=None)
    assert list(good) == _lib.PARAMS[name]
    for p in ("frame_ids", "token_start", "token_end"):
        assert _status(name, good, **{p: None}) == NULL, p
    for kw in (dict(B=0), dict(T=0), dict(T=-1)):
        assert _status(name, good, **kw) == BAD, kw
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((conf, ids, total, out, starts), keep))     # nothing was launched


# ---- the transcribers -----------------------------------------------------------------------------------------------------------------
def _drive_slots(tr, dev, segments):
    """SCHED (tests/test_endpoint_gpu.py): slots 0 and 1 open from the start, slot 2 before step 2.  Returns the logits of
    every step, per slot its logits from open(s) on, the Words of its segments, finish_words(), and per segmented slot the
    frame of its first cut."""
    g = torch.Generator().manual_seed(9)
    steps, fed, seg, cuts = [], {s: [] for s in range(3)}, {s: [] for s in range(3)}, {}
    tr.open(0), tr.open(1)
    for i, fr in enumerate(SCHED):
        if i == 2:
            tr.open(2)
        logits, k = tr.step(torch.randn(3, 80, 64, generator=g).mul(3.0).to(dev), fr)
        steps.append(logits.clone())
        for s in range(3):
            if k[s]:
                fed[s].append(logits[s, :k[s]].clone())
        for s in segments.get(i, []):
            cuts.setdefault(s, tr.encoder.n0[s])
            seg[s] += tr.segment_words(s)
    return steps, {s: torch.cat(c) for s, c in fed.items()}, seg, tr.finish_words(), cuts


def _offline(words, logits, blank, cfg):
    """word_confidence on one slot's concatenated logits (T, V)"""
    conf, ids = frame_confidence(logits[None], None, cfg)
    return word_confidence([words], conf, ids, blank, None, cfg)[0]


@pytest.mark.parametrize("segments", [{}, SEGMENTS], ids=["whole", "segmented"])
def test_slot_transcriber_word_confidence(dev, segments):
    from conformer_amd.slots import SlotTranscriber
    m = _tiny_model(71, dev)
    dec = BeamCTCDecoder(VOCAB, 0, skip_ids=(16,), beam_width=16)
    cfg = ConfidenceConfig()
    plain = SlotTranscriber(m, dec, 3, 800, times=True)
    assert plain.confidence is None
    p_steps, _, p_seg, p_final, _ = _drive_slots(plain, dev, segments)
    tr = SlotTranscriber(m, dec, 3, 800, times=True, confidence=cfg)
    steps, fed, seg, final, cuts = _drive_slots(tr, dev, segments)
    assert all(torch.equal(a, b) for a, b in zip(steps, p_steps)) and seg == p_seg and final == p_final
    assert set(final) == {0, 1, 2} and sum(len(w) for w in final.values()) + sum(len(w) for w in seg.values()) >= 3
    assert tr.confidence.total.tolist() == [fed[s].shape[0] for s in range(3)]          # slot 2, opened late, from its open
    got = tr.word_confidence(final)
    got_seg = tr.word_confidence({s: w for s, w in seg.items() if w})
    for s in range(3):
        want = _offline(final[s] + seg[s], fed[s], 0, cfg)
        assert got[s] == want[:len(final[s])] and got_seg.get(s, []) == want[len(final[s]):]
        assert all(0.0 <= v <= 1.0 for v in want)
    if segments:                                            # words of later segments: their frames still count from open(s)
        assert sorted(cuts) == [0, 2] and any(w.start_frame >= cuts[s] for s in cuts for w in final[s] + seg[s])
    # a slot opened again starts its history again
    tr.open(1)
    assert tr.confidence.total.tolist()[1] == 0 and tr.confidence.total.tolist()[0] == fed[0].shape[0]
    with pytest.raises(ValueError, match="times=True"):
        SlotTranscriber(m, dec, 3, 800, confidence=cfg)
    with pytest.raises(RuntimeError, match="confidence="):
        plain.word_confidence({})


def test_streaming_transcriber_word_confidence(dev):
    from conformer_amd.transcribe import StreamingTranscriber
    m = _tiny_model(71, dev)
    dec = BeamCTCDecoder(VOCAB, 0, skip_ids=(16,), beam_width=16)
    cfg = ConfidenceConfig(method="entropy", aggregation="mean")
    mel = torch.randn(2, 80, 300, generator=torch.Generator().manual_seed(9)).mul(3.0).to(dev)

    def drive(tr):
        chunks = [tr.step(mel[:, :, a:a + n]) for a, n in ((0, 64), (64, 100), (164, 7), (171, 129))]
        return torch.cat(chunks, dim=1), tr.finish_words()

    p_logits, p_words = drive(StreamingTranscriber(m, dec, 2, 300, times=True))
    tr = StreamingTranscriber(m, dec, 2, 300, times=True, confidence=cfg, confidence_history=256)
    logits, words = drive(tr)
    assert torch.equal(logits, p_logits) and words == p_words and sum(len(w) for w in words) >= 2
    assert tr.confidence.total.tolist() == [logits.shape[1]] * 2
    got = tr.word_confidence(words)
    assert got == [_offline(words[b], logits[b], 0, cfg) for b in range(2)]
    tr.reset()
    assert tr.confidence.total.tolist() == [0, 0]
    with pytest.raises(ValueError, match="times=True"):
        StreamingTranscriber(m, dec, 2, 300, confidence=cfg)
