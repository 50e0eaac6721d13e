"""Bounded-history streaming (left_context) on the MI355X: cfm_relpos_attention_window_f32 over ring K/V caches, and the
streaming objects on top of it.

The window kernel against a float64 row-by-row restatement that reads only the keys of each window (tests/window_restatement.py)
for every head-dim class and window length around the 32-key tile, against the reference's MultiHeadSelfAttentionModule under
the banded mask (goldens), through a ring that turns over six times, over a ring full of NaN, at positions past 2^40, with
out-of-range device values, and against the full-context slots kernel when the window covers everything; StreamingEncoder,
SlotStreamingEncoder and the transcribers with left_context against the windowed float64 encoder and against each other; a stream
several rings long that allocates nothing as it goes; the three refusals."""
import pytest
import torch

from conformer_amd import ops
from oracle import conformer_oracle as O
from tests import window_restatement as W
from tests.test_stream_slots_gpu import SCHEDULE, UTT_LEN, _decoder, _drive, _guarded, _model, _utts
from tests.util import cfg_params, load_golden, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ---- 1. the kernel -------------------------------------------------------------------------------------------------------------

def _inputs(S, T, H, dh, P, seed):
    """A linear history lin (S,T,3d) of every slot's stream, a projected table for P positions, the two biases (CPU)."""
    d = H * dh
    g = torch.Generator().manual_seed(seed)
    lin = torch.randn(S, T, 3 * d, generator=g)
    pos = torch.randn(2 * P - 1, d, generator=g) * 0.5
    return lin, pos, torch.randn(d, generator=g) * 0.3, torch.randn(d, generator=g) * 0.3


def _ring(lin, ends, R, fill=0.0, at=None):
    """The ring (S,R,3d) after slot b has streamed the frames 0 .. ends[b]-1 of lin[b] (frame n in row (at[b] + n) mod R; the rest
    keeps `fill`)."""
    S, _, d3 = lin.shape
    ring = torch.full((S, R, d3), fill)
    for b in range(S):
        for n in range(ends[b]):
            ring[b, ((at[b] if at else 0) + n) % R] = lin[b, n]
    return ring


def _restate(lin, pos, u, v, H, b, begin, count, left):
    """float64: the queries begin .. begin+count-1 of slot b under the windowed rule, (count, d)"""
    d = lin.shape[2] // 3
    dh, e = d // H, begin + count
    x = lin[b:b + 1, :e]
    q, k, val = (x[..., j * d:(j + 1) * d].reshape(1, e, H, dh) for j in range(3))
    pp = pos.view(pos.shape[0], H, dh)
    rows = list(range(begin, e))
    return W.window_attention_core(q[:, begin:e], k, val, pp, u.view(H, dh), v.view(H, dh), [e] * count, left, q_pos=rows)[0]


def _window(ring, pos, u, v, H, qb, qc, q_max, left, dev, ctx=None):
    t = lambda x: torch.tensor(x, dtype=torch.int64, device=dev)
    with torch.no_grad():
        out = ops.relpos_attention_window(ring.to(dev), pos.to(dev), u.to(dev), v.to(dev), H, t(qb), t(qc), q_max, left, ctx)
    torch.cuda.synchronize()
    return out.cpu()


QB, QC = [0, 77, 5, 203], [40, 0, 13, 40]        # a fresh stream of 40 rows (two waves), an idle slot, 13 rows, 40 rows far along


@pytest.mark.parametrize("left", [0, 1, 31, 32, 33, 40])
@pytest.mark.parametrize("H,dh", [(4, 16), (4, 36), (8, 64)])
def test_window_kernel_vs_float64(dev, H, dh, left):
    """left = 1 with 40 rows: the second wave's rows 32 .. 39 start at the key tile 32 .. 63 whose keys < 40 only some see."""
    q_max = 40
    R, P = 32 * ((left + q_max + 31) // 32), max(left + 1, q_max)
    ends = [b + c for b, c in zip(QB, QC)]
    lin, pos, u, v = _inputs(4, max(ends), H, dh, P, seed=dh + left)
    got = _window(_ring(lin, ends, R), pos, u, v, H, QB, QC, q_max, left, dev)
    assert torch.isfinite(got).all()
    for b in range(4):
        assert torch.all(got[b, QC[b]:] == 0.0), b                               # padded rows exactly zero
        if QC[b]:
            err = rel_l2(got[b, :QC[b]], _restate(lin, pos, u, v, H, b, QB[b], QC[b], left))
            print(f"H={H} dh={dh} left={left} slot {b}: {err:.3g}")
            assert err < 2e-6, (b, err)


@pytest.mark.parametrize("case", ["stream_window_mhsa_d64_t70_l24", "stream_window_mhsa_d144_t49_l7"])
def test_window_kernel_vs_reference_banded_mask(dev, case):
    """Chunk by chunk through ONE ring, against the reference's MultiHeadSelfAttentionModule under the banded (1,1,T',T') mask
    (tests/golden/make_golden_window.py)."""
    from conformer_amd.streaming import ring_rows
    meta, g = load_golden(case)
    P = {k: v.to(dev) for k, v in cfg_params(meta).items()}
    a = "encoder.layers.0.attention."
    x = g["x"].to(dev)
    B, T, d = x.shape
    H, left = meta["n_heads"], meta["left"]
    xn = ops.layernorm(x, P[a + "layer_norm.weight"], P[a + "layer_norm.bias"])
    wqkv = torch.cat([P[a + f"attention.{n}_proj.weight"] for n in ("query", "key", "value")]).contiguous()
    bqkv = torch.cat([P[a + f"attention.{n}_proj.bias"] for n in ("query", "key", "value")]).contiguous()
    qkv = ops.linear(xn, wqkv, bqkv)                                     # (B, T, 3d): every frame's rows, fed chunk by chunk
    ends = g["chunk_ends"].tolist()
    k_cap = max(e - s for s, e in zip([0] + ends, ends))
    R, n_pos = 32 * ((left + k_cap + 31) // 32), max(left + 1, k_cap)
    assert R < T                                                         # the ring wraps inside the utterance
    pe = ops.relpos_table(P["encoder.rel_pe.div_term"][None], n_pos)
    pos = ops.linear(pe, P[a + "attention.pos_proj.weight"], P[a + "attention.pos_proj.bias"])
    ring = torch.full((B, R, 3 * d), float("nan"), device=dev)
    ctx = torch.zeros(B, T, d, device=dev)
    start = 0
    for e in ends:
        for dst, src, n in ring_rows(start, e - start, R):
            ring[:, dst:dst + n] = qkv[:, start + src:start + src + n]
        ctx[:, start:e] = ops.relpos_attention_window(ring, pos, P[a + "attention.content_bias"], P[a + "attention.position_bias"], H,
                                                      torch.full((B,), start, dtype=torch.int64, device=dev),
                                                      torch.full((B,), e - start, dtype=torch.int64, device=dev), e - start, left)
        start = e
    y = ops.linear(ctx, P[a + "attention.out_proj.weight"], P[a + "attention.out_proj.bias"])
    err = rel_l2(y, g["mhsa_y"])
    print(f"{case}: {err:.3g}")
    assert err < 2e-5


def test_ring_turns_over_six_times(dev):
    """T' = 200, left = 20, chunks of at most 12 rows: R = 32, every row of the ring is rewritten six times."""
    from conformer_amd.streaming import ring_rows
    H, dh, T, left, R = 4, 16, 200, 20, 32
    d = H * dh
    lin, pos, u, v = _inputs(2, T, H, dh, 21, seed=77)
    sizes, ends = [12, 1, 7, 12, 11, 3], []
    while not ends or ends[-1] < T:
        ends.append(min(T, (ends[-1] if ends else 0) + sizes[len(ends) % len(sizes)]))
    assert ends[-1] == T and max(e - s for s, e in zip([0] + ends, ends)) <= 12 and T // R == 6
    ring = torch.full((2, R, 3 * d), float("nan"), device=dev)
    lin_d, pos_d, u_d, v_d = (t.to(dev) for t in (lin, pos, u, v))
    outs, start = [], 0
    for e in ends:
        k = e - start
        for dst, src, n in ring_rows(start, k, R):
            ring[:, dst:dst + n] = lin_d[:, start + src:start + src + n]
        # (q_max = 12 whatever the chunk: the rows past k are padding)
        outs.append(ops.relpos_attention_window(ring, pos_d, u_d, v_d, H, torch.full((2,), start, dtype=torch.int64, device=dev),
                                                torch.full((2,), k, dtype=torch.int64, device=dev), 12, left)[:, :k])
        start = e
    got = torch.cat(outs, dim=1).cpu()
    q, k_, val = (lin[..., j * d:(j + 1) * d].reshape(2, T, H, dh) for j in range(3))
    want = W.window_attention_core(q, k_, val, pos.view(-1, H, dh), u.view(H, dh), v.view(H, dh), W.visible_ends(ends, T), left)
    err = rel_l2(got, want)
    print(f"ring wrap: {err:.3g}")
    assert torch.isfinite(got).all() and err < 2e-6


@pytest.mark.parametrize("H,dh", [(4, 16), (2, 64)])
def test_masked_ring_rows_never_reach_a_result(dev, H, dh):
    """A ring full of NaN in which only the rows a fresh stream owns are written: finite, and bit for bit the zero-filled run.
    Slot 0 starts at frame 0 (its window is cut at frame 0), slot 1 is 9 frames in (left = 33 reaches before frame 0), slot 2
    has 70 frames behind it of which the first ones are overwritten garbage."""
    left, q_max, R = 33, 40, 96
    qb, qc = [0, 9, 70], [40, 12, 33]
    ends = [b + c for b, c in zip(qb, qc)]
    lin, pos, u, v = _inputs(3, max(ends), H, dh, 40, seed=5)
    runs = []
    for fill in (float("nan"), 0.0, float("inf")):
        ring = _ring(lin, ends, R, fill=fill)
        ring[2, 7:37] = fill           # slot 2: the rows its last key tile covers past the chunk's end (frames 7 .. 36: outside every window)
        runs.append(_window(ring, pos, u, v, H, qb, qc, q_max, left, dev))
    assert torch.isfinite(runs[0]).all()
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[2], runs[1])
    for b in range(3):
        assert rel_l2(runs[0][b, :qc[b]], _restate(lin, pos, u, v, H, b, qb[b], qc[b], left)) < 2e-6


def test_positions_past_2_to_the_40(dev):
    """q_begin = 2^40 + 5 with the data at n mod R equals the same ring at q_begin = 5 + 3R (R = 64 divides 2^40)."""
    H, dh, left, q_max, R = 4, 16, 24, 40, 64
    small = 5 + 3 * R
    lin, pos, u, v = _inputs(2, small + q_max, H, dh, 40, seed=9)
    ring = _ring(lin, [small + q_max, small + 17], R)
    a = _window(ring, pos, u, v, H, [small, small], [q_max, 17], q_max, left, dev)
    big = 2 ** 40 + 5
    assert big % R == small % R
    b = _window(ring, pos, u, v, H, [big, big], [q_max, 17], q_max, left, dev)
    assert torch.equal(a, b)
    assert rel_l2(a[0], _restate(lin, pos, u, v, H, 0, small, q_max, left)) < 2e-6
    assert rel_l2(a[1, :17], _restate(lin, pos, u, v, H, 1, small, 17, left)) < 2e-6 and torch.all(a[1, 17:] == 0.0)


def test_window_kernel_clamps_device_values(dev):
    """A negative q_begin is frame 0, an oversized q_count is q_max, a negative one is 0: ctx sits inside a sentinel-filled buffer
    whose sentinels survive, and the ring, exactly R rows inside guard bands of NaN, is all the kernel reads."""
    H, dh, left, q_max, R = 4, 16, 24, 8, 32
    d = H * dh
    lin, pos, u, v = _inputs(4, 8, H, dh, 25, seed=13)
    qb, qc = [-3, 0, 5, -(2 ** 40)], [2 ** 40, 8, -7, 100]
    rbuf, ring, G = _guarded((4, R, 3 * d), dev, fill=0.0)
    rbuf[:G] = float("nan")
    rbuf[G + ring.numel():] = float("nan")
    ring.copy_(_ring(lin, [8, 8, 8, 8], R).to(dev))
    buf, ctx, G = _guarded((4, q_max, d), dev)
    got = _window(ring, pos, u, v, H, qb, qc, q_max, left, dev, ctx=ctx)
    assert torch.all(buf[:G] == 777.0) and torch.all(buf[G + ctx.numel():] == 777.0)
    assert torch.isfinite(got).all() and torch.all(got[2] == 0.0)
    for b in (0, 1, 3):
        assert rel_l2(got[b], _restate(lin, pos, u, v, H, b, 0, 8, left)) < 2e-6


@pytest.mark.parametrize("H,dh", [(4, 16), (2, 64)])
def test_window_over_all_history_is_the_slots_kernel(dev, H, dh):
    """left >= the history of every slot, ring not yet wrapped: cfm_relpos_attention_slots_f32 on the same buffer as a linear cache."""
    left, q_max, R = 88, 40, 128
    qb, qc = [0, 50, 13], [40, 37, 0]
    ends = [b + c for b, c in zip(qb, qc)]
    assert left >= max(ends) - 1                                         # the last query's window reaches frame 0
    lin, pos, u, v = _inputs(3, R, H, dh, R, seed=17)
    ring = _ring(lin, ends, R).to(dev)
    t = lambda x: torch.tensor(x, dtype=torch.int64, device=dev)
    with torch.no_grad():
        want = ops.relpos_attention_slots(ring, pos.to(dev), u.to(dev), v.to(dev), t(ends), H, t(qb), t(qc), q_max, keys_hint=1)
    got = _window(ring, pos, u, v, H, qb, qc, q_max, left, dev)
    assert rel_l2(got, want) <= 1e-6


# ---- 2. the streaming objects --------------------------------------------------------------------------------------------------

def _encoder(P, n_blocks, d, H, K, dev):
    from model.modules.encoder import Encoder
    enc = Encoder(80, n_blocks, d, H, K, 0.0)
    enc.load_state_dict({k[len("encoder."):]: v.float() for k, v in P.items() if k.startswith("encoder.")}, strict=True)
    return enc.to(dev).eval()


@pytest.mark.parametrize("d,K", [(32, 31), (64, 7)])
def test_streaming_encoder_left_context_vs_windowed_float64(dev, d, K):
    from conformer_amd.streaming import StreamingEncoder, chunk_ends
    H, L, left = 4, 2, 24
    chunks = [64, 3, 130, 1, 7, 100, 98]                                 # T = 403 -> T' = 100; the largest step makes 33 frames
    P = O.make_params(vocab=8, n_mel=80, n_blocks=L, d=d, n_heads=H, ksize=K, lstm_hidden=8, seed=11, dtype=torch.float64,
                      with_decoder=False)
    T = sum(chunks)
    x = torch.randn(2, 80, T, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    ends = chunk_ends(T, chunks)
    ref = W.encoder_forward_windowed(x, P, L, H, ends, left)
    enc = _encoder(P, L, d, H, K, dev)
    st = StreamingEncoder(enc, 2, None, left_context=left, max_chunk_mel_frames=max(chunks))
    assert all(c.shape == (2, st.ring, 3 * d) for c in st.qkv) and st.ring == 64 < ends[-1] and st.ctx is None
    full = StreamingEncoder(enc, 2, T)
    xd = x.float().to(dev)
    outs, outs_full, t0 = [], [], 0
    for c in chunks:
        outs.append(st.step(xd[:, :, t0:t0 + c]))
        outs_full.append(full.step(xd[:, :, t0:t0 + c]))
        t0 += c
    got, got_full = torch.cat(outs, dim=1), torch.cat(outs_full, dim=1)
    assert got.shape == ref.shape and st.frames == ends[-1] == 100
    err = rel_l2(got, ref)
    print(f"d={d} K={K}: windowed stream vs float64 {err:.3g}; vs full-context stream {rel_l2(got, got_full):.3g}")
    assert err < 2e-5
    assert rel_l2(got, got_full) > 1e-3                                  # the bound really changes the numbers


def test_endless_stream_allocates_nothing_as_it_goes(dev):
    from conformer_amd.streaming import StreamingEncoder
    P = O.make_params(vocab=8, n_mel=80, n_blocks=2, d=32, n_heads=4, ksize=31, lstm_hidden=8, seed=12, with_decoder=False)
    enc = _encoder(P, 2, 32, 4, 31, dev)
    st = StreamingEncoder(enc, 2, None, left_context=24, max_chunk_mel_frames=64)
    assert st.t_max is None and st.ring == 64
    x = torch.randn(2, 80, 64, device=dev)
    mem, out = [], None
    for i in range(24):                                                  # 24 x 16 frames = 6 rings
        out = st.step(x)
        torch.cuda.synchronize()
        mem.append(torch.cuda.memory_allocated())
    assert st.frames == 24 * 16 - 1 > 5 * st.ring
    assert all(c.shape == (2, 64, 96) for c in st.qkv) and torch.isfinite(out).all()
    assert mem[-1] == mem[2], mem
    with pytest.raises(ValueError):
        st.step(torch.randn(2, 80, 65, device=dev))                      # more than the ring was sized for
    assert st.frames == 24 * 16 - 1


def _single_windowed(enc, x, chunks, left, max_chunk, dev):
    from conformer_amd.streaming import StreamingEncoder
    st = StreamingEncoder(enc, 1, None, left_context=left, max_chunk_mel_frames=max_chunk)
    outs, t0 = [], 0
    with torch.no_grad():
        for c in chunks:
            outs.append(st.step(x[None, :, t0:t0 + c].float().to(dev)))
            t0 += c
    return torch.cat(outs, dim=1)[0]


def test_slot_encoder_left_context_is_the_single_stream(dev):
    """Ragged per-slot chunks, staggered opens, slot 3 closed and reopened over a ring that still holds the previous stream:
    every utterance equals a one-utterance windowed StreamingEncoder fed the same chunks."""
    from conformer_amd.slots import SlotStreamingEncoder
    from conformer_amd.streaming import chunk_ends
    m, P = _model(32, 4, 61, dev, hidden=8)
    utts = _utts(UTT_LEN, 3)
    enc = SlotStreamingEncoder(m.encoder, 4, None, left_context=24, max_chunk_mel_frames=300)
    assert enc.ring == 128 and all(c.shape == (4, 128, 96) for c in enc.qkv)
    chunks, rows, _ = _drive(enc, 4, utts, SCHEDULE, dev)
    for u, x in enumerate(utts):
        assert sum(chunks[u]) == x.shape[1]
        one = _single_windowed(m.encoder, x, chunks[u], 24, 300, dev)
        err = rel_l2(rows[u], one)
        print(f"utterance {u}: {err:.3g}")
        assert rows[u].shape == one.shape and err < 1e-5, (u, err)
    # and the single stream is the float64 windowed encoder (utterance 0: 700 mel frames, T' = 174 > R)
    ref = W.encoder_forward_windowed(utts[0][None], P, 2, 4, chunk_ends(700, chunks[0]), 24)[0]
    assert rel_l2(rows[0], ref) < 2e-5


def test_slot_transcriber_left_context_is_the_lockstep_transcriber(dev):
    from conformer_amd.slots import SlotTranscriber
    from conformer_amd.transcribe import StreamingTranscriber
    m, _ = _model(32, 4, 91, dev)
    dec = _decoder("plain", None)
    chunks = [64, 64, 7, 1, 130, 64, 130, 100]
    T, S = sum(chunks), 3
    x = torch.randn(S, 80, T, generator=torch.Generator().manual_seed(4)).to(dev)
    kw = dict(left_context=16, max_chunk_mel_frames=130)
    ref_tr, tr = StreamingTranscriber(m, dec, S, T, **kw), SlotTranscriber(m, dec, S, T, **kw)
    assert ref_tr.encoder.ring == tr.encoder.ring == 64
    for s in range(S):
        tr.open(s)
    t0 = 0
    for c in chunks:
        want = ref_tr.step(x[:, :, t0:t0 + c])
        got, k = tr.step(x[:, :, t0:t0 + c], [c] * S)
        assert k == [want.shape[1]] * S and got.shape == want.shape
        if want.shape[1]:
            assert rel_l2(got, want) < 1e-5
        t0 += c
    assert ref_tr.encoder.frames > 2 * 64
    want_text = ref_tr.finish()
    assert [tr.close(s) for s in range(S)] == want_text


def test_the_three_refusals_leave_the_state_alone(dev):
    from conformer_amd.slots import SlotStreamingEncoder
    from conformer_amd.streaming import StreamingEncoder
    P = O.make_params(vocab=8, n_mel=80, n_blocks=1, d=32, n_heads=4, ksize=31, lstm_hidden=8, seed=14, with_decoder=False)
    enc = _encoder(P, 1, 32, 4, 31, dev)
    kw = dict(left_context=8, max_chunk_mel_frames=64)
    with pytest.raises(NotImplementedError):
        StreamingEncoder(enc, 2, None, graphs=True, **kw)
    with pytest.raises(NotImplementedError):
        SlotStreamingEncoder(enc, 2, None, dtype=torch.bfloat16, **kw)
    st, twin = StreamingEncoder(enc, 2, None, **kw), StreamingEncoder(enc, 2, None, **kw)
    x = torch.randn(2, 80, 150, device=dev)
    a = [st.step(x[:, :, :64])]
    keep = [c.clone() for c in st.qkv] + [c.clone() for c in st.conv_state] + [st.mel_tail_buf.clone()]
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(NotImplementedError):
            with torch.autocast("cuda", dtype=dt):
                st.step(x[:, :, 64:128])
    now = list(st.qkv) + list(st.conv_state) + [st.mel_tail_buf]
    assert st.frames == 15 and all(torch.equal(p, q) for p, q in zip(keep, now))
    a += [st.step(x[:, :, 64:128]), st.step(x[:, :, 128:])]
    b = [twin.step(x[:, :, :64]), twin.step(x[:, :, 64:128]), twin.step(x[:, :, 128:])]
    assert torch.equal(torch.cat(a, dim=1), torch.cat(b, dim=1))
    sl = SlotStreamingEncoder(enc, 2, None, **kw)
    sl.open(0)
    with pytest.raises(NotImplementedError):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            sl.step(x[:, :, :64], [64, 0])
    with pytest.raises(ValueError):
        sl.step(x[:, :, :65], [65, 0])                                   # more than max_chunk_mel_frames
    assert sl.n0 == [0, 0] and sl.mel_seen == [0, 0]
