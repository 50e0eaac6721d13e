"""Endpointing on the MI355X (conformer_amd/endpoint.py, cfm_endpoint_step_f32).

All outputs are integers: the (S, 8) state equals the float64 restatement (tests/endpoint_restatement.py) integer for integer on
inputs whose every frame keeps |log p_sil - log thr| >= 1e-3 (fp32 log-softmax over V <= 370 errs by about 1e-6), any chunking
gives the same bits with no margin at all, rows behind k[b] are never read, the rules fire at exactly their frame, and
SlotTranscriber(endpoint=...) changes no logit and no text while segment(s) cuts a slot's stream into utterances."""
import math

import numpy as np
import pytest
import torch

from conformer_amd import _lib
from conformer_amd.decode import BeamCTCDecoder
from conformer_amd.endpoint import Endpoint, EndpointConfig, EndpointRule, StreamingEndpointer, ctc_endpoints
from tests import endpoint_restatement as R

pytestmark = pytest.mark.gpu

THR = 0.8
# in frames (the endpointers below run at frame_seconds = 1): rules that latch part way through a 130-frame slot
FRAME_RULES = (EndpointRule(4, 40, 3), EndpointRule(3, 0, 10), EndpointRule(0, 100, 0, False))
MARGIN = 1e-3


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _rows(rules, fs=1.0):
    return [r.frames(fs) for r in rules]


def _margin_frames(T, V, seed, blank=0, thr=THR):
    """(T, V) fp32 logits: Gaussian non-blank logits, the blank set in float64 so that p_blank is one of the five values."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((T, V))
    ps = np.array([0.05, 0.5, thr - 0.02, thr + 0.02, 0.99])[rng.integers(0, 5, T)]
    others = np.delete(x, blank, axis=1)
    lse = np.log(np.exp(others).sum(axis=1))
    x[:, blank] = np.log(ps / (1.0 - ps)) + lse
    return torch.from_numpy(x.astype(np.float32))


def _assert_margin(frames, ids, thr):
    """float64, on the cast inputs, every frame: the construction keeps the threshold a thousand fp32 errors away."""
    for t in range(frames.shape[0]):
        lp = R.log_p_silence(frames[t].numpy(), ids)
        assert abs(lp - math.log(thr)) >= MARGIN, (t, lp)


def _feed(ep, slots, parts, dev, fill=0.0):
    """slots: per slot its (T_b, V) frames; parts: per slot the frame counts of the steps.  Rows behind k[b] hold `fill`."""
    pos = [0] * len(slots)
    V = slots[0].shape[1]
    for i in range(len(parts[0])):
        ks = [p[i] for p in parts]
        x = torch.full((len(slots), max(ks), V), fill)
        for b, f in enumerate(slots):
            x[b, :ks[b]] = f[pos[b]:pos[b] + ks[b]]
            pos[b] += ks[b]
        ep.step(x.to(dev), torch.tensor(ks, dtype=torch.int64, device=dev))
    assert pos == [f.shape[0] for f in slots]


def _want(slots, ids, thr, rules):
    return [R.run_frames(f.numpy(), ids, thr, rules) for f in slots]


# ---- exactness ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts", [(130, 0, 1), (63, 0, 65), (64, 130, 0)], ids=str)
@pytest.mark.parametrize("V", [5, 67, 370, 512, 513])      # odd V: every second row off 8-byte alignment; 512 | 513: the kernel
def test_state_equals_the_restatement(dev, V, counts):     # holds a row in registers up to 512 and walks it twice beyond
    blank = V - 2
    slots = [_margin_frames(T, V, seed=7 * V + T + b, blank=blank) for b, T in enumerate(counts)]
    for f in slots:
        _assert_margin(f, [blank], THR)
    want = _want(slots, [blank], THR, _rows(FRAME_RULES))
    assert any(w[3] >= 0 for w in want) or max(counts) < 130
    cfg = EndpointConfig(rules=FRAME_RULES, blank_threshold=THR)
    one = StreamingEndpointer(3, blank, cfg, 1.0, dev)
    _feed(one, slots, [[T] for T in counts], dev)
    assert one.state.cpu().tolist() == want
    three = StreamingEndpointer(3, blank, cfg, 1.0, dev)
    _feed(three, slots, [[T // 4, T // 2, T - T // 4 - T // 2] for T in counts], dev)
    assert three.state.cpu().tolist() == want
    got = one.read()
    for b, w in enumerate(want):
        assert got[b] == (None if w[3] < 0 else Endpoint(w[3], w[4], float(w[4] + 1), w[5]))


def test_rows_behind_k_are_never_read_and_an_idle_slot_is_untouched(dev):
    V, counts = 67, (65, 0, 130)
    slots = [_margin_frames(T, V, seed=11 + b) for b, T in enumerate(counts)]
    cfg = EndpointConfig(rules=FRAME_RULES, blank_threshold=THR)
    parts = [[T // 4, T // 2, T - T // 4 - T // 2] for T in counts]
    states = []
    sentinel = torch.tensor([5, 4, 3, -1, 9, 8, 77, 88], dtype=torch.int32)
    for fill in (0.0, math.nan):
        ep = StreamingEndpointer(3, 0, cfg, 1.0, dev)
        ep.state[1] = sentinel.to(dev)
        _feed(ep, slots, parts, dev, fill=fill)
        states.append(ep.state.cpu())
    assert torch.equal(states[0], states[1])
    assert torch.equal(states[1][1], sentinel)                                # k = 0 in every step: bit for bit as it was
    assert states[1].tolist()[0] == R.run_frames(slots[0].numpy(), [0], THR, _rows(FRAME_RULES))
    # a logits tensor with no rows at all is a step of nothing
    ep.step(torch.empty(3, 0, V, device=dev))
    assert torch.equal(ep.state.cpu(), states[1])


# ---- the rules' boundaries ------------------------------------------------------------------------------------------------------
def _flag_frames(flags, V=5, blank=0):
    x = torch.zeros(len(flags), V)
    x[:, blank] = torch.tensor([10.0 if f else -10.0 for f in flags])
    return x


SIL, SPK = [True], [False]


@pytest.mark.parametrize("rule,met,short,frame", [
    (EndpointRule(5, 0, 0, False), SPK * 3 + SIL * 5, SPK * 3 + SIL * 4 + SPK * 1, 7),            # min_trailing
    (EndpointRule(0, 10, 0, False), SPK * 4 + SIL * 6, SPK * 4 + SIL * 5, 9),                     # min_frames
    (EndpointRule(0, 0, 4, False), SIL * 2 + SPK * 3 + SIL * 2 + SPK * 1, SIL * 2 + SPK * 3 + SIL * 3, 7),   # min_speech
    (EndpointRule(2, 6, 3, True), SPK * 3 + SIL * 3, SPK * 2 + SIL * 4, 5)], ids=["trailing", "frames", "speech", "all"])
def test_a_rule_fires_at_exactly_its_frame_and_not_one_short(dev, rule, met, short, frame):
    ep = StreamingEndpointer(2, 0, EndpointConfig(rules=[rule], blank_threshold=THR), 1.0, dev)
    _feed(ep, [_flag_frames(met), _flag_frames(short)], [[len(met)], [len(short)]], dev)
    st = ep.state.cpu().tolist()
    assert st[0] == R.run_flags(met, _rows([rule])) and st[1] == R.run_flags(short, _rows([rule]))
    assert st[0][3] == 0 and st[0][4] == frame and st[1][3] == -1


def test_an_all_silent_stream_fires_the_first_default_rule_only(dev):
    ep = StreamingEndpointer(2, 0, EndpointConfig(), 0.04, dev)              # DEFAULT_RULES: 125, 25 after speech, 500 frames
    _feed(ep, [_flag_frames(SIL * 124), _flag_frames(SIL * 130)], [[100, 24], [100, 30]], dev)
    assert ep.read() == [None, Endpoint(0, 124, 125 * 0.04, 125)]
    assert ep.state.cpu().tolist() == [[124, 124, 0, -1, 0, 0, 0, 0], [130, 130, 0, 0, 124, 125, 0, 0]]
    ep.reset_slots([1])                                                       # armed again: the counters start over
    assert ep.state.cpu().tolist()[1] == [0, 0, 0, -1, 0, 0, 0, 0] and ep.state.cpu().tolist()[0][0] == 124
    _feed(ep, [_flag_frames(SPK * 1 + SIL * 25), _flag_frames(SPK * 1 + SIL * 24)], [[26], [25]], dev)
    assert ep.read() == [Endpoint(1, 149, 150 * 0.04, 25), None]


# ---- special values, silence_ids ----------------------------------------------------------------------------------------------
def test_special_values(dev):
    inf, nan = math.inf, math.nan
    frames = torch.tensor([[-inf, 0.0, 1.0, 2.0, 0.5],          # blank = -inf: not silent
                           [3.0, -inf, -inf, -inf, -inf],        # all others -inf: p = 1, silent
                           [9.0, 0.0, nan, 0.0, 0.0],            # a NaN beside a dominant blank: not silent
                           [nan, 0.0, 0.0, 0.0, 0.0],            # the blank itself a NaN: not silent
                           [9.0, 0.0, 0.0, 0.0, 0.0],            # (a plain silent frame)
                           [-inf, -inf, -inf, -inf, -inf]])      # nothing at all: blank = -inf, not silent
    want = [False, True, False, False, True, False]
    assert [R.is_silent(f.numpy(), [0], THR) for f in frames] == want
    ep = StreamingEndpointer(6, 0, EndpointConfig(rules=[EndpointRule(1, 0, 0, False)], blank_threshold=THR), 1.0, dev)
    ep.step(frames[:, None, :].contiguous().to(dev))                          # k=None: every row
    st = ep.state.cpu().tolist()
    assert [s[1] == 1 and s[2] == 0 for s in st] == want and all(s[0] == 1 for s in st)
    assert [s[3] for s in st] == [0 if w else -1 for w in want]


def test_two_silence_ids_below_the_threshold_are_silent_together(dev):
    V = 67
    x = torch.randn(1, V, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    rest = torch.logsumexp(x[0, 2:], 0)
    x[0, 0] = x[0, 1] = math.log(0.45 / 0.10) + rest                          # p_0 = p_1 = 0.45, the rest 0.10
    x = x.float()
    assert not R.is_silent(x[0].numpy(), [0], THR) and not R.is_silent(x[0].numpy(), [1], THR)
    assert R.is_silent(x[0].numpy(), [0, 1], THR) and abs(R.log_p_silence(x[0].numpy(), [0, 1]) - math.log(0.9)) < 1e-6
    rule = [EndpointRule(1, 0, 0, False)]
    alone = StreamingEndpointer(1, 0, EndpointConfig(rules=rule, blank_threshold=THR), 1.0, dev)
    both = StreamingEndpointer(1, 0, EndpointConfig(rules=rule, blank_threshold=THR, silence_ids=(1,)), 1.0, dev)
    swapped = StreamingEndpointer(1, 1, EndpointConfig(rules=rule, blank_threshold=THR, silence_ids=(0, 1)), 1.0, dev)
    for ep in (alone, both, swapped):
        ep.step(x[None].to(dev))
    assert alone.state.cpu().tolist() == [[1, 0, 1, -1, 0, 0, 0, 0]]
    assert both.state.cpu().tolist() == swapped.state.cpu().tolist() == [[1, 1, 0, 0, 0, 1, 0, 0]]
    with pytest.raises(ValueError, match="outside"):                          # an id the vocabulary does not have: before any launch
        StreamingEndpointer(1, 0, EndpointConfig(silence_ids=(V,)), 1.0, dev).step(x[None].to(dev))


# ---- chunk invariance, no margin --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [370, 513])                   # (either side of the kernel's row-in-registers limit)
def test_any_chunking_gives_the_same_bits(dev, V):
    S, T = 3, 200
    x = torch.randn(S, T, V, generator=torch.Generator().manual_seed(21)).to(dev)
    # plain Gaussian logits: p_blank is around 1 / (V sqrt(e)); a threshold there makes about half the frames silent, and
    # nothing keeps a frame away from it
    cfg = EndpointConfig(rules=FRAME_RULES, blank_threshold=0.74 / V)
    states = []
    for c in (T, 1, 7, 64, 65):
        ep = StreamingEndpointer(S, 0, cfg, 1.0, dev)
        for t0 in range(0, T, c):
            ep.step(x[:, t0:t0 + c])                                          # (a view: its strides are the entry's pitches)
        states.append(ep.state.cpu())
    assert all(0 < s < T for s in states[0][:, 2].tolist())                  # both kinds of frame occur in every slot
    assert all(f == T for f in states[0][:, 0].tolist())
    for s in states[1:]:
        assert torch.equal(s, states[0])


def test_a_step_is_capturable(dev):
    """One step captured in a graph (nothing allocates or synchronises in it), replayed over three chunks written into its
    static buffers: the state an eager endpointer reaches."""
    S, V, c = 3, 67, 50
    frames = torch.stack([_margin_frames(3 * c, V, seed=41 + b) for b in range(S)]).to(dev)
    ks = [[50, 0, 7], [1, 50, 0], [50, 50, 50]]
    cfg = EndpointConfig(rules=FRAME_RULES, blank_threshold=THR)
    eager, ep = StreamingEndpointer(S, 0, cfg, 1.0, dev), StreamingEndpointer(S, 0, cfg, 1.0, dev)
    x, k = torch.zeros(S, c, V, device=dev), torch.zeros(S, dtype=torch.int64, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ep.step(x, k)                                                         # (warm-up outside the capture: k = 0, a no-op)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ep.step(x, k)
    for i, kk in enumerate(ks):
        x.copy_(frames[:, i * c:(i + 1) * c])
        k.copy_(torch.tensor(kk, device=dev))
        graph.replay()
        eager.step(frames[:, i * c:(i + 1) * c], kk)
    assert torch.equal(ep.state.cpu(), eager.state.cpu()) and ep.state.cpu()[:, 0].tolist() == [101, 100, 57]


# ---- the offline form ---------------------------------------------------------------------------------------------------------------
def test_ctc_endpoints_is_one_step_of_a_fresh_endpointer(dev):
    V, counts = 67, (130, 0, 65)
    slots = [_margin_frames(130, V, seed=31 + b) for b in range(3)]
    x = torch.stack(slots).to(dev)
    lengths = torch.tensor(counts, dtype=torch.int64, device=dev)
    cfg = EndpointConfig(rules=FRAME_RULES, blank_threshold=THR)
    end, rule = ctc_endpoints(x, 0, lengths, cfg, 1.0)
    ep = StreamingEndpointer(3, 0, cfg, 1.0, dev)
    ep.step(x, lengths)
    st = ep.state.cpu()
    assert end.dtype == rule.dtype == torch.int64 and end.is_cuda and rule.is_cuda
    assert rule.cpu().tolist() == st[:, 3].tolist() and rule.cpu().tolist()[1] == -1 and max(rule.cpu().tolist()) >= 0
    assert end.cpu().tolist() == [int(e) if r >= 0 else -1 for e, r in zip(st[:, 4], st[:, 3])]
    assert st.tolist() == _want([f[:T] for f, T in zip(slots, counts)], [0], THR, _rows(FRAME_RULES))
    # longer than one launch takes (4096 frames per slot): the same as steps of any other size
    long = torch.randn(2, 4100, 5, generator=torch.Generator().manual_seed(5)).to(dev)
    # the first rule fires at frame 4097, behind the launch boundary, for the utterance that has that frame
    cfg = EndpointConfig(rules=[EndpointRule(0, 4098, 0, False), EndpointRule(7, 0, 3000, False)], blank_threshold=0.2)
    end, rule = ctc_endpoints(long, 0, torch.tensor([4100, 4097], device=dev), cfg, 1.0)
    ep = StreamingEndpointer(2, 0, cfg, 1.0, dev)
    for t0 in range(0, 4100, 1000):
        n = min(1000, 4100 - t0)
        ep.step(long[:, t0:t0 + n], [n, min(n, 4097 - t0)])
    st = ep.state.cpu()
    assert st[:, 0].tolist() == [4100, 4097] and rule.cpu().tolist() == st[:, 3].tolist() == [0, -1]
    assert end.cpu().tolist() == [int(e) if r >= 0 else -1 for e, r in zip(st[:, 4], st[:, 3])]


def test_host_tensors_and_other_types_are_refused(dev):
    ep = StreamingEndpointer(2, 0, EndpointConfig(), 0.04, dev)
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        ep.step(torch.zeros(2, 3, 5))
    with pytest.raises(_lib.ConformerHipError, match="float32"):
        ep.step(torch.zeros(2, 3, 5, device=dev, dtype=torch.bfloat16))
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        ctc_endpoints(torch.zeros(2, 3, 5), 0)
    with pytest.raises(ValueError, match="expected"):
        ep.step(torch.zeros(3, 3, 5, device=dev))
    with pytest.raises(ValueError, match="frame counts"):
        ep.step(torch.zeros(2, 3, 5, device=dev), [1, 2, 3])
    assert ep.state.cpu().tolist() == [[0, 0, 0, -1, 0, 0, 0, 0]] * 2


# ---- the C entry's refusals -------------------------------------------------------------------------------------------------------
def test_the_entry_refuses_before_any_launch(dev):
    S, k_max, V = 2, 3, 5
    x = torch.zeros(S, k_max, V, device=dev)
    k = torch.zeros(S, dtype=torch.int64, device=dev)
    ids = torch.zeros(8, dtype=torch.int32, device=dev)
    rules = torch.zeros(4, 4, dtype=torch.int32, device=dev)
    state = torch.tensor([[1, 2, 3, -1, 5, 6, 7, 8]] * S, dtype=torch.int32, device=dev)
    keep = state.clone()
    good = dict(logits=x.data_ptr(), ld_slot=k_max * V, ld_row=V, k=k.data_ptr(), k_max=k_max, V=V, silence_ids=ids.data_ptr(),
                n_silence=1, log_threshold=math.log(0.8), rules=rules.data_ptr(), n_rules=1, state=state.data_ptr(), S=S,
                stream=None)
    assert list(good) == _lib.PARAMS["cfm_endpoint_step_f32"]

    def status(**kw):
        try:
            _lib.call("cfm_endpoint_step_f32", *{**good, **kw}.values())
        except _lib.ConformerHipError as e:
            return int(str(e).rsplit("status ", 1)[1].rstrip(")"))
        return 0

    C = _lib.CONSTANTS
    NULL, BAD, UNSUP = C["CFM_ERR_NULL"], C["CFM_ERR_BAD_SHAPE"], C["CFM_ERR_UNSUPPORTED"]
    for name in ("logits", "k", "silence_ids", "rules", "state"):
        assert status(**{name: None}) == NULL, name
    for kw in (dict(S=0), dict(S=-1), dict(k_max=-1), dict(V=1), dict(n_rules=0), dict(n_rules=5), dict(n_silence=0),
               dict(n_silence=9), dict(ld_row=V - 1), dict(ld_slot=k_max * V - 1), dict(log_threshold=math.nan)):
        assert status(**kw) == BAD, kw
    for kw in (dict(k_max=4097, ld_slot=4097 * V), dict(S=65535), dict(V=65537, ld_row=65537, ld_slot=k_max * 65537)):
        assert status(**kw) == UNSUP, kw
    assert status(k_max=0, logits=None, ld_slot=0) == 0                       # nothing to do: no launch, no error
    assert status() == 0                                                      # (k = 0 everywhere: the launch touches nothing)
    torch.cuda.synchronize()
    assert torch.equal(state, keep)


# ---- SlotTranscriber(endpoint=...) ---------------------------------------------------------------------------------------------------
VOCAB = ["<pad>"] + [chr(ord("a") + i) for i in range(14)] + ["|", "<unk>"]
# mel frames per step for slots 0, 1, 2; slot 2 opens before step 2; slot 0 is segmented after steps 2 and 5, slot 2 after step 4
SCHED = [[64, 40, 0], [33, 64, 0], [64, 5, 64], [7, 64, 64], [64, 0, 30], [64, 64, 64], [40, 64, 1], [64, 30, 64]]
SEGMENTS = {2: [0], 4: [2], 5: [0]}


def _tiny_model(seed, dev):
    from model.conformer import Conformer
    from oracle import conformer_oracle as O
    P = O.make_params(vocab=len(VOCAB), n_mel=80, n_blocks=2, d=32, n_heads=4, ksize=31, lstm_hidden=24, seed=seed)
    m = Conformer(len(VOCAB), 80, 2, 32, 4, 31, 24, 1, 0.0)
    m.load_state_dict(P, strict=True)
    return m.to(dev).eval()


def _run(tr, dev, segments, words=False, on_step=None):
    """Drive SCHED.  Per slot the list of its segments, each (text or Words, [its logits chunks (1, k, V)])."""
    g = torch.Generator().manual_seed(9)
    S = 3
    fed = {s: [] for s in range(S)}
    done = {s: [] for s in range(S)}
    logits_all = []
    tr.open(0), tr.open(1)
    for i, fr in enumerate(SCHED):
        if i == 2:
            tr.open(2)
        logits, k = tr.step(torch.randn(S, 80, 64, generator=g).mul(3.0).to(dev), fr)
        logits_all.append(logits.clone())
        for s in range(S):
            if k[s]:
                fed[s].append(logits[s:s + 1, :k[s]].clone())
        if on_step is not None:
            on_step(i, fed)
        for s in segments.get(i, []):
            done[s].append((tr.segment_words(s) if words else tr.segment(s), fed[s]))
            fed[s] = []
            assert tr.is_open[s]
    for s in range(S):
        done[s].append((tr.close_words(s) if words else tr.close(s), fed[s]))
    assert not any(tr.is_open)
    return done, logits_all


def _threshold_in_a_gap(chunks, blank):
    """A threshold no frame of the run comes near: the middle of the widest gap in the central half of the sorted float64
    log p_blank of every frame the run produces (the half-gap is asserted against the fp32 classification error)."""
    lp = sorted(R.log_p_silence(f.numpy(), [blank]) for c in chunks for f in c[0].cpu())
    n = len(lp)
    gap, at = max((lp[i + 1] - lp[i], i) for i in range(n // 4, 3 * n // 4))
    assert gap / 2 >= 1e-4, gap
    return math.exp((lp[at] + lp[at + 1]) / 2)


def test_slot_transcriber_with_endpoints_and_segments(dev):
    from conformer_amd.slots import SlotTranscriber
    m = _tiny_model(71, dev)
    dec = BeamCTCDecoder(VOCAB, 0, skip_ids=(16,), beam_width=16)
    plain, plain_logits = _run(SlotTranscriber(m, dec, 3, 800), dev, SEGMENTS)
    whole, _ = _run(SlotTranscriber(m, dec, 3, 800), dev, {})
    thr = _threshold_in_a_gap([c for s in plain for _, chunks in plain[s] for c in chunks], 0)
    rules = (EndpointRule(0.08, 0.4, 0.08), EndpointRule(0.0, 1.2, 0.0, False))     # 2 silent of >= 10 with 2 spoken; 30 frames
    assert _rows(rules, 0.04) == [(2, 10, 2, 0), (0, 30, 0, 0)]
    cfg = EndpointConfig(rules=rules, blank_threshold=thr)
    tr = SlotTranscriber(m, dec, 3, 800, endpoint=cfg)
    assert tr.endpointer is not None and SlotTranscriber(m, dec, 3, 800).endpointer is None
    seen = []

    def check(i, fed):
        """endpoints() against the restatement over each open slot's logits since its open or last segment"""
        want, off = {}, {}
        for s in range(3):
            if not tr.is_open[s]:
                continue
            frames = torch.cat([c[0] for c in fed[s]]).cpu().numpy() if fed[s] else np.zeros((0, len(VOCAB)))
            st = R.run_frames(frames, [0], thr, _rows(rules, 0.04))
            off[s] = tr.encoder.n0[s] - len(frames)                           # where the slot's current segment began
            if st[3] >= 0:
                want[s] = Endpoint(st[3], st[4] + off[s], (st[4] + off[s] + 1) * 0.04, st[5])
        assert tr.endpoints() == want, i
        assert [off.get(s, 0) for s in range(3)] == [tr.seg_start[s] if s in off else 0 for s in range(3)]
        seen.append((want, off))

    got, got_logits = _run(tr, dev, SEGMENTS, on_step=check)
    assert all(torch.equal(a, b) for a, b in zip(got_logits, plain_logits)) and len(got_logits) == len(SCHED)
    assert {s: [t for t, _ in segs] for s, segs in got.items()} == {s: [t for t, _ in segs] for s, segs in plain.items()}
    assert any(s in w and o[s] > 0 for w, o in seen for s in range(3))        # some fired in a later segment: counted from open
    assert [len(got[s]) for s in range(3)] == [3, 1, 2]
    for s in range(3):
        for text, chunks in got[s]:                                           # every segment: the decoder on its own logits alone
            assert text == dec(torch.cat(chunks, dim=1))[0], s
    assert got[1][0][0] == whole[1][0][0]                                     # the neighbour's text does not know of the segments
    assert " ".join(t for t, _ in got[0]) != "" and whole[0][0][0] != ""
    with pytest.raises(RuntimeError, match="endpoint="):
        SlotTranscriber(m, dec, 3, 800).endpoints()


def test_segments_under_max_pending(dev):
    from conformer_amd.slots import SlotTranscriber
    m = _tiny_model(71, dev)
    dec = BeamCTCDecoder(VOCAB, 0, skip_ids=(16,), beam_width=16)
    kw = dict(left_context=8, max_chunk_mel_frames=64, max_pending=4)
    tr = SlotTranscriber(m, dec, 3, None, endpoint=EndpointConfig(), **kw)
    k_cap = tr.commit[1]
    popped = {}                                                               # (slot, its segment's index): token ids

    def pop(i, fed):
        if i in (1, 3, 6):                                                    # what is popped is no longer part of segment()'s text
            for s, ids in tr.pop_committed().items():
                j = sum(1 for at, slots in SEGMENTS.items() if at < i and s in slots)
                popped[s, j] = popped.get((s, j), []) + ids
    got, _ = _run(tr, dev, SEGMENTS, on_step=pop)
    plain, _ = _run(SlotTranscriber(m, dec, 3, None, **kw), dev, SEGMENTS, on_step=None)
    committed_any = False
    for s in range(3):
        for j, (text, chunks) in enumerate(plain[s]):                         # without pops: a one-utterance committing search
            ref = dec.stream(1, None, dev, max_pending=4, max_chunk_frames=k_cap)
            for c in chunks:
                ref.step(c)
            committed_any |= int(ref.state.total[0]) > 0
            assert ref.finish() == [text], (s, j)
    assert committed_any and int(tr.beam.state.total.sum()) == 0
    # with pops: a segment's text lost the prefix popped during it and nothing else (words are joined again across the cut)
    assert sum(len(ids) > 0 for ids in popped.values()) >= 2
    for s in range(3):
        assert len(got[s]) == len(plain[s])
        for j, ((text, _), (whole, _)) in enumerate(zip(got[s], plain[s])):
            assert (dec.text(popped.get((s, j), [])) + text).replace(" ", "") == whole.replace(" ", ""), (s, j)


def test_segment_words_count_from_open(dev):
    from conformer_amd.slots import SlotTranscriber
    m = _tiny_model(71, dev)
    dec = BeamCTCDecoder(VOCAB, 0, skip_ids=(16,), beam_width=16)
    tr = SlotTranscriber(m, dec, 3, 800, times=True, endpoint=EndpointConfig())
    got, _ = _run(tr, dev, SEGMENTS, words=True)
    texts, _ = _run(SlotTranscriber(m, dec, 3, 800), dev, SEGMENTS)
    shifted = 0
    for s in range(3):
        first = 0                                                             # the segment's first frame, counted from open(s)
        for (words, chunks), (text, _) in zip(got[s], texts[s]):
            assert " ".join(w.text for w in words) == text
            ref = dec.stream(1, 800, dev, times=True)
            for c in chunks:
                ref.step(c)
            sec = first * 0.04
            want = [w._replace(start_frame=w.start_frame + first, end_frame=w.end_frame + first, start=w.start + sec,
                               end=w.end + sec) for w in ref.finish_words()[0]]
            assert words == want, s
            n = sum(c.shape[1] for c in chunks)
            assert all(first <= w.start_frame < w.end_frame <= first + n for w in words)
            shifted += bool(first and words)
            first += n
    assert shifted >= 2                                                       # later segments with words in them
