"""Independent streams under autocast (conformer_amd/slots.py with dtype=) on the MI355X.

The 16-bit slots attention kernel (cfm_relpos_attention_slots_mfma16_f32): per-element softmax-mass probes (tests/attention_probe.py:
exact operands, the derived bound (u_t + F) * ref + floor, unchanged for the key split -- each slice's partial is a sum of rounded
non-negative p's over the unrounded slice sum and the merge is a convex combination in fp32), with the fp32 and the 16-bit cache,
ragged offsets, two row blocks, dh = 36, a single key, an empty slot, and a key split with an empty slice; guard bands and clamped
device offsets; the reduction to the rows kernel at identical offsets.  Then SlotStreamingEncoder / SlotTranscriber with
dtype=bf16 / fp16: the 16-bit bar (rel-L2 < 1e-2) against the float64 chunked restatement, text on close against BeamCTCDecoder on
the returned logits, the lockstep reduction, neighbours, and the refusals."""
import functools
import math

import pytest
import torch

from conformer_amd import _lib, ops
from conformer_amd.decode import BeamCTCDecoder
from oracle import conformer_oracle as O
from tests import attention_probe as AP
from tests.util import Calls, rel_l2

pytestmark = pytest.mark.gpu

ENTRY = "cfm_relpos_attention_slots_mfma16_f32"
F32 = torch.float32
DT = pytest.mark.parametrize("dt", AP.DT16, ids=["bf16", "fp16"])
CACHE = pytest.mark.parametrize("q16", [False, True], ids=["cache32", "cache16"])
BAR = {torch.bfloat16: 1e-2, torch.float16: 3e-3}            # 16-bit operand bars of test_attention_rows_16bit_form_vs_float64

VOCAB = ["<pad>"] + [chr(ord("a") + i) for i in range(14)] + ["|", "<unk>"]
UNK = 16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def _L(values, dev):
    return torch.tensor(values, dtype=torch.int64, device=dev)


# ---- 1. per-element probe ------------------------------------------------------------------------------------------------

# name -> ((B, T, H, dh), q_begin, q_count); lengths = q_begin + q_count, keys_hint = 1
GEOMETRIES = {
    "ragged_three_blocks": ((2, 300, 2, 64), [33, 190], [31, 67]),
    "two_row_blocks_ring_wrap": ((2, 161, 2, 64), [0, 31], [161, 130]),
    "dh36": ((2, 249, 4, 36), [1, 131], [32, 118]),
    "single_key_empty_slot": ((2, 1, 2, 8), [0, 0], [1, 0]),
}
SPLIT = ((3, 520, 2, 16), [505, 3, 100], [15, 17, 0])         # default hint: 2 key slices; slot 1 has one key tile, slot 2 no rows


def _probe(dev, shape, qb, qc, dt, q16, keys_hint, what):
    B, T, H, dh = shape
    lengths = tuple(b + c for b, c in zip(qb, qc))
    q_max = max(qc)
    worst = 0.0
    for pattern in AP.PATTERNS:
        op = AP.operands(B, T, H, dh, pattern)
        qkv, pos, u, v = AP.device_inputs(op, dev, dt if q16 else F32)
        ref = AP.reference(op, lengths)
        with Calls(ENTRY, "cfm_relpos_attention_slots_f32") as seen, torch.autocast("cuda", dtype=dt):
            ctx = ops.relpos_attention_slots(qkv, pos, u, v, _L(lengths, dev), H, _L(qb, dev), _L(qc, dev), q_max,
                                             keys_hint=keys_hint)
        assert seen == {ENTRY}, seen
        assert ctx.dtype == F32 and ctx.shape == (B, q_max, H * dh)
        got = ref.clone()                                  # the compact rows put back at their cache rows; the rest is not under test
        for b in range(B):
            got[b, qb[b]:qb[b] + qc[b]] = ctx[b, :qc[b]].double().cpu()
            assert torch.all(ctx[b, qc[b]:] == 0.0), (what, pattern, b)
        worst = max(worst, AP.check(got, ref, op, dt, ctx16=False, what=f"{ENTRY} {what}"))
    print(f"probe slots16 {what} {str(dt).replace('torch.', '')} cache16={int(q16)}: worst element at {worst:.3f} of the bound")


@DT
@CACHE
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_probe_slots16(dev, name, q16, dt):
    shape, qb, qc = GEOMETRIES[name]
    _probe(dev, shape, qb, qc, dt, q16, 1, name)


@DT
@CACHE
def test_probe_slots16_key_split(dev, q16, dt):
    (B, T, H, dh), qb, qc = SPLIT
    assert ops._key_split(B, H, max(qc), T, None) == 2 and ops._key_split16(B, H, max(qc), T, None) == 2
    _probe(dev, (B, T, H, dh), qb, qc, dt, q16, None, "2 key slices")


# ---- 2. guard bands, clamping --------------------------------------------------------------------------------------------

def _restate(qkv, pos, u, v, H, b, rows, L):
    """float64 relative-position attention of cache rows `rows` of slot b against its keys < L: (len(rows), d)"""
    T, d = qkv.shape[1], qkv.shape[2] // 3
    dh = d // H
    x = qkv[b].double().cpu()
    q, k, val = x[:, :d].view(T, H, dh), x[:L, d:2 * d].view(L, H, dh), x[:L, 2 * d:].view(L, H, dh)
    p = pos.double().cpu().view(2 * T - 1, H, dh)
    uu, vv = u.double().cpu().view(H, dh), v.double().cpu().view(H, dh)
    out = []
    for i in rows:
        r = T - 1 - (i - torch.arange(L))
        s = ((q[i] + uu)[None] * k).sum(-1) + ((q[i] + vv)[None] * p[r]).sum(-1)     # (L, H)
        w = torch.softmax(s / math.sqrt(dh), dim=0)
        out.append((w[:, :, None] * val).sum(0).reshape(d))
    return torch.stack(out) if out else torch.zeros(0, d, dtype=torch.float64)


def _inputs(S, T, H, dh, dev, seed, dt=F32):
    d = H * dh
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(S, T, 3 * d, generator=g).to(dt).to(dev)
    pos = (torch.randn(2 * T - 1, d, generator=g) * 0.5).to(dev)
    u, v = (torch.randn(d, generator=g) * 0.3).to(dev), (torch.randn(d, generator=g) * 0.3).to(dev)
    return qkv, pos, u, v


def _guarded(shape, dev, fill=float("nan"), G=4096):
    n = math.prod(shape)
    buf = torch.full((G + n + G,), 777.0, device=dev)
    buf[G:G + n] = fill
    return buf, buf[G:G + n].view(*shape), G


SPLITS = pytest.mark.parametrize("split", [False, True], ids=["nsplit1", "keysplit"])


@DT
@SPLITS
@pytest.mark.parametrize("H,dh", [(4, 16), (2, 64)])
def test_slots16_guard_bands_vs_float64(dev, H, dh, split, dt):
    S, T, q_max = 5, 1000, 10
    d = H * dh
    qkv, pos, u, v = _inputs(S, T, H, dh, dev, seed=dh + 3, dt=dt)
    qb = [0, 37, 990, 500, 700]
    qc = [5, 0, 10, 3, 7]
    L = [b + c for b, c in zip(qb, qc)]
    assert ops._key_split16(S, H, q_max, T, None) == 4 and ops._key_split16(S, H, q_max, T, 1) == 1
    keep = qkv.clone()
    buf, ctx, G = _guarded((S, q_max, d), dev)
    with torch.no_grad(), Calls(ENTRY) as seen, torch.autocast("cuda", dtype=dt):
        ops.relpos_attention_slots(qkv, pos, u, v, _L(L, dev), H, _L(qb, dev), _L(qc, dev), q_max, ctx, keys_hint=None if split else 1)
    torch.cuda.synchronize()
    assert seen == {ENTRY}
    assert torch.all(buf[:G] == 777.0) and torch.all(buf[G + ctx.numel():] == 777.0)        # guard bands untouched
    assert torch.equal(qkv, keep)
    got = ctx.cpu()
    for b in range(S):
        assert torch.all(got[b, qc[b]:] == 0.0), b                                           # padded rows exactly zero
        if qc[b]:
            want = _restate(qkv, pos, u, v, H, b, range(qb[b], qb[b] + qc[b]), L[b])
            assert rel_l2(got[b, :qc[b]], want) < BAR[dt], (b, rel_l2(got[b, :qc[b]], want))


@DT
@SPLITS
def test_slots16_clamps_device_offsets(dev, split, dt):
    """Out-of-range device values: the kernel clamps them (q_begin to [0,T], q_count to [0, min(q_max, T - q_begin)], lengths
    to T); nothing outside the cache, the table or ctx is touched and the clamped slots compute their clamped rows."""
    S, T, H, dh, q_max = 5, 1000, 4, 16, 8
    qkv, pos, u, v = _inputs(S, T, H, dh, dev, seed=5, dt=dt)
    big = 1 << 40
    qb = _L([-3, T + 5, big, 995, 0], dev)
    qc = _L([big, 4, 3, 100, -7], dev)
    L = _L([big, -1, 5, T, 0], dev)
    keep = qkv.clone()
    buf, ctx, G = _guarded((S, q_max, H * dh), dev)
    with torch.no_grad(), Calls(ENTRY) as seen, torch.autocast("cuda", dtype=dt):
        ops.relpos_attention_slots(qkv, pos, u, v, L, H, qb, qc, q_max, ctx, keys_hint=None if split else 1)
    torch.cuda.synchronize()
    assert seen == {ENTRY}
    assert torch.all(buf[:G] == 777.0) and torch.all(buf[G + ctx.numel():] == 777.0)
    assert torch.equal(qkv, keep)
    got = ctx.cpu()
    assert torch.all(got[1:3] == 0.0) and torch.all(got[4] == 0.0) and torch.all(got[3, 5:] == 0.0)
    assert rel_l2(got[0], _restate(qkv, pos, u, v, H, 0, range(0, q_max), T)) < BAR[dt]
    assert rel_l2(got[3, :5], _restate(qkv, pos, u, v, H, 3, range(995, 1000), T)) < BAR[dt]


# ---- 3. identical offsets: the rows kernel -------------------------------------------------------------------------------

@DT
@pytest.mark.parametrize("H,dh", [(4, 16), (2, 64)])
def test_slots16_with_identical_offsets_is_the_rows_kernel(dev, H, dh, dt):
    S, T, n0, k = 5, 1000, 600, 8
    qkv, pos, u, v = _inputs(S, T, H, dh, dev, seed=3)
    lengths = torch.full((S,), n0 + k, device=dev, dtype=torch.int64)
    qb, qc = torch.full((S,), n0, device=dev, dtype=torch.int64), torch.full((S,), k, device=dev, dtype=torch.int64)
    rounded = qkv.to(dt)                                           # the same values in an fp32 and in a 16-bit cache
    with torch.no_grad(), torch.autocast("cuda", dtype=dt):
        full = torch.zeros(S, T, H * dh, device=dev)
        ops.relpos_attention_rows(qkv, pos, u, v, lengths, H, n0, k, full, keys_hint=1)
        got = ops.relpos_attention_slots(qkv, pos, u, v, lengths, H, qb, qc, k, keys_hint=1)
        full_r = torch.zeros(S, T, H * dh, device=dev)
        ops.relpos_attention_rows(rounded.float(), pos, u, v, lengths, H, n0, k, full_r, keys_hint=1)
        got_r = ops.relpos_attention_slots(rounded, pos, u, v, lengths, H, qb, qc, k, keys_hint=1)
    assert rel_l2(got, full[:, n0:n0 + k]) <= 1e-6
    assert rel_l2(got_r, full_r[:, n0:n0 + k]) <= 1e-6


def test_slots16_refuses_a_cache_of_the_wrong_type(dev):
    S, T, H, dh = 2, 64, 2, 16
    qkv, pos, u, v = _inputs(S, T, H, dh, dev, seed=1, dt=torch.bfloat16)
    z = torch.zeros(S, device=dev, dtype=torch.int64)
    with pytest.raises(_lib.ConformerHipError):
        ops.relpos_attention_slots(qkv, pos, u, v, z, H, z, z, 1)                  # 16-bit cache outside autocast
    with pytest.raises(_lib.ConformerHipError), torch.autocast("cuda", dtype=torch.float16):
        ops.relpos_attention_slots(qkv, pos, u, v, z, H, z, z, 1)                  # the other 16-bit type


# ---- 4.-8. encoder, transcriber ------------------------------------------------------------------------------------------

def _model(d, heads, seed, dev, hidden=24, n_blocks=2):
    from model.conformer import Conformer
    P = O.make_params(vocab=len(VOCAB), n_mel=80, n_blocks=n_blocks, d=d, n_heads=heads, ksize=31, lstm_hidden=hidden,
                      seed=seed, dtype=torch.float64)
    m = Conformer(len(VOCAB), 80, n_blocks, d, heads, 31, hidden, 1, 0.0)
    m.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in P.items()}, strict=True)
    return m.to(dev).eval(), P


def _utts(lengths, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(80, n, generator=g, dtype=torch.float64) for n in lengths]


# every step: closes (slot list), then opens ({slot: utterance}), then the frames each slot takes ({slot: count})
SCHEDULE = [
    dict(open={0: 0, 1: 1, 3: 3}, frames={0: 64, 1: 5, 3: 100}),
    dict(frames={0: 130, 1: 3, 3: 0}),                         # slot 1: 8 frames in all -> its first encoder frame
    dict(frames={0: 64, 1: 200, 3: 7}),
    dict(open={2: 2}, frames={0: 1, 2: 6, 3: 193}),            # slot 2 opens after slot 0 took three chunks; 6 only buffer
    dict(close=[3], open={3: 4}, frames={0: 200, 1: 242, 2: 300, 3: 60}),   # slot 3 reused for a new utterance
    dict(frames={0: 241, 2: 0, 3: 200}),
    dict(frames={2: 214}),
]
UTT_LEN = [700, 450, 520, 300, 260]


def _drive(obj, S, utts, schedule, dev, seed=0):
    """Run a schedule on a SlotStreamingEncoder or SlotTranscriber: per utterance its chunks and its rows (the text too for
    a transcriber: closes at the end of the schedule).  Columns of the chunk a slot does not take hold noise."""
    is_tr = hasattr(obj, "partial_text")
    g = torch.Generator().manual_seed(1000 + seed)
    owner, pos = [None] * S, {}
    chunks = {u: [] for u in range(len(utts))}
    rows = {u: [] for u in range(len(utts))}
    texts = {}
    for st in schedule:
        for s in st.get("close", []):
            texts[owner[s]] = obj.close(s)
            owner[s] = None
        for s, u in st.get("open", {}).items():
            obj.open(s)
            owner[s], pos[u] = u, 0
        fr = [0] * S
        Tc = max([1] + list(st["frames"].values()))
        mel = torch.randn(S, 80, Tc, generator=g, dtype=torch.float64) * 3.0
        for s, n in st["frames"].items():
            u = owner[s]
            mel[s, :, :n] = utts[u][:, pos[u]:pos[u] + n]
            pos[u] += n
            fr[s] = n
            if n:
                chunks[u].append(n)
        out, k = obj.step(mel.float().to(dev), fr)
        assert out.shape[:2] == (S, max(k)) and out.dtype == F32
        for s in range(S):
            if owner[s] is not None and k[s]:
                rows[owner[s]].append(out[s, :k[s]])
    for s in range(S):
        if owner[s] is not None and is_tr:
            texts[owner[s]] = obj.close(s)
    cat = {u: torch.cat(r, dim=0) if r else None for u, r in rows.items()}
    return chunks, cat, texts


@functools.lru_cache(maxsize=None)
def _encoder_references(d, heads):
    """Per (d, heads), once: the model, the utterances, the float64 chunked restatement and the fp32 slot encoder's rows (CPU)."""
    from conformer_amd.slots import SlotStreamingEncoder
    from conformer_amd.streaming import chunk_ends
    dev = torch.device("cuda:0")
    m, P = _model(d, heads, 61, dev, hidden=8)
    utts = _utts(UTT_LEN, 3)
    chunks, rows32, _ = _drive(SlotStreamingEncoder(m.encoder, 4, 800), 4, utts, SCHEDULE, dev)
    refs = [O.encoder_forward_chunked(x[None], P, 2, heads, chunk_ends(x.shape[1], chunks[u]))[0] for u, x in enumerate(utts)]
    return m, utts, refs, {u: r.cpu() for u, r in rows32.items()}


@DT
@pytest.mark.parametrize("d,heads", [(32, 4), (512, 8)], ids=["small", "cfg5_width"])
def test_slot_encoder16_matches_chunked_oracle(dev, d, heads, dt):
    from conformer_amd.slots import SlotStreamingEncoder
    m, utts, refs, rows32 = _encoder_references(d, heads)
    enc = SlotStreamingEncoder(m.encoder, 4, 800, dtype=dt)
    assert enc.qkv[0].dtype == dt and all(t.dtype == dt for t in enc.qkv)
    assert all(t.dtype == F32 for t in enc.conv_state)
    with Calls(ENTRY, "cfm_relpos_attention_slots_f32") as seen:
        chunks, rows, _ = _drive(enc, 4, utts, SCHEDULE, dev)
    assert seen == {ENTRY}
    assert enc.mel_tail_buf.dtype == F32
    for u, x in enumerate(utts):
        assert sum(chunks[u]) == x.shape[1]
        assert rows[u].shape == refs[u].shape, u
        e = rel_l2(rows[u], refs[u])
        print(f"slot encoder d={d} {str(dt).replace('torch.', '')} utterance {u}: rel-L2 {e:.3e} against float64, "
              f"{rel_l2(rows[u], rows32[u]):.3e} against the fp32 slot encoder")
        assert e < 1e-2, (u, e)
        assert rel_l2(rows[u], rows32[u]) > 1e-5, u                    # the 16-bit path really ran


@pytest.fixture(scope="module")
def lm(tmp_path_factory):
    from conformer_amd.lm import NgramLanguageModel, write_synthetic_arpa
    p = tmp_path_factory.mktemp("lm") / "slots16.arpa"
    write_synthetic_arpa(p, VOCAB[1:15], 30, [0, 150, 150], seed=4, max_tokens_per_word=2)
    return NgramLanguageModel.from_arpa(p)


def _decoder(mode, lm):
    return BeamCTCDecoder(VOCAB, 0, skip_ids=(UNK,), beam_width=16, lm=lm if "lm" in mode else None,
                          hotwords=["ab", "c d", "e"] if "hw" in mode else None, alpha=1.1, beta=2.0, hotword_weight=3.0)


@pytest.mark.parametrize("mode", ["plain", "lm", "hw", "lm_hw"])
def test_slot_transcriber16_text_on_close(dev, lm, mode):
    from conformer_amd.slots import SlotTranscriber
    m, _ = _model(32, 4, 71, dev)
    dec = _decoder(mode, lm)
    utts = _utts(UTT_LEN, 5)
    tr = SlotTranscriber(m, dec, 4, 800, dtype=torch.bfloat16)
    _, logits, texts = _drive(tr, 4, utts, SCHEDULE, dev, seed=1)
    assert all(h.dtype == F32 and c.dtype == F32 for h, c in tr.state)
    assert set(texts) == set(range(len(utts)))
    for u in range(len(utts)):
        assert texts[u] == dec(logits[u]), (mode, u)


@DT
def test_lockstep16_tracks_the_streaming_transcriber(dev, dt):
    from conformer_amd.slots import SlotTranscriber
    from conformer_amd.transcribe import StreamingTranscriber
    m, _ = _model(32, 4, 91, dev)
    dec = _decoder("plain", None)
    chunks = [64, 64, 7, 1, 130, 64]
    T, S = sum(chunks), 3
    x = torch.randn(S, 80, T, generator=torch.Generator().manual_seed(4)).to(dev)
    ref_tr, tr = StreamingTranscriber(m, dec, S, T), SlotTranscriber(m, dec, S, T, dtype=dt)
    for s in range(S):
        tr.open(s)
    t0 = 0
    for c in chunks:
        with torch.autocast("cuda", dtype=dt):
            want = ref_tr.step(x[:, :, t0:t0 + c])
        got, k = tr.step(x[:, :, t0:t0 + c], [c] * S)
        assert k == [want.shape[1]] * S and got.shape == want.shape
        if want.shape[1]:
            assert rel_l2(got, want) < 1e-2, rel_l2(got, want)
        t0 += c


def test_neighbours16_stay_within_the_logits_bar(dev):
    """Text equality between runs with different neighbours is not promised in 16 bits (compact rows may tile the GEMMs
    differently and a rounding can flip a near-tie): only the logits bar."""
    from conformer_amd.slots import SlotTranscriber
    m, _ = _model(32, 4, 81, dev)
    dec = _decoder("plain", None)
    utts = _utts([400, 300, 350, 500, 200], 9)
    mine = [64, 0, 3, 130, 7, 196]                              # utterance 0 in slot 1, the same frames in both runs
    a = [dict(open={1: 0, 0: 1}, frames={1: mine[0], 0: 100})] + \
        [dict(frames={1: f, 0: 40}) for f in mine[1:5]] + [dict(frames={1: mine[5]})]
    b = [dict(open={1: 0, 2: 2, 0: 3}, frames={1: mine[0], 2: 350, 0: 7})] + \
        [dict(frames={1: mine[1], 0: 200}), dict(close=[2], open={2: 4}, frames={1: mine[2], 2: 200, 0: 13}),
         dict(frames={1: mine[3], 0: 280}), dict(frames={1: mine[4]}), dict(frames={1: mine[5]})]
    bf = torch.bfloat16
    _, la, _ = _drive(SlotTranscriber(m, dec, 3, 600, dtype=bf), 3, utts, a, dev, seed=2)
    _, lb, _ = _drive(SlotTranscriber(m, dec, 3, 600, dtype=bf), 3, utts, b, dev, seed=3)
    assert rel_l2(la[0], lb[0]) < 1e-2, rel_l2(la[0], lb[0])


def test_refusals16_leave_the_state_alone(dev):
    from conformer_amd.slots import SlotStreamingEncoder, SlotTranscriber
    from conformer_amd.streaming import chunk_ends
    m, P = _model(32, 4, 101, dev)
    dec = _decoder("plain", None)
    with pytest.raises(ValueError):
        SlotTranscriber(m, dec, 2, 300, dtype=torch.float64)
    with pytest.raises(ValueError):
        SlotStreamingEncoder(m.encoder, 2, 300, dtype=torch.float64)
    m36, _ = _model(36, 3, 102, dev, hidden=8)
    for dt in AP.DT16:
        with pytest.raises(ValueError):
            SlotStreamingEncoder(m36.encoder, 2, 300, dtype=dt)                # a 16-bit cache needs d % 8 == 0
    tr = SlotTranscriber(m, dec, 2, 300, dtype=torch.bfloat16)
    x = _utts([300], 12)[0]
    xd = x.float().to(dev)
    tr.open(0)
    outs, chunks = [], []

    def feed(n, t0):
        mel = torch.zeros(2, 80, n, device=dev)
        mel[0] = xd[:, t0:t0 + n]
        lg, k = tr.step(mel, [n, 0])
        outs.append(lg[0, :k[0]])
        chunks.append(n)

    feed(100, 0)
    with pytest.raises(RuntimeError):
        with torch.autocast("cuda", dtype=torch.float16):                  # the other 16-bit type
            tr.step(torch.zeros(2, 80, 10, device=dev), [10, 0])
    with pytest.raises(RuntimeError):
        with torch.autocast("cuda", dtype=torch.float16):
            tr.encoder.step(torch.zeros(2, 80, 10, device=dev), [10, 0])
    with pytest.raises(RuntimeError):
        tr.step(torch.zeros(2, 80, 10, device=dev), [10, 5])               # frames for free slot 1
    with torch.autocast("cuda", dtype=torch.bfloat16):                      # its own type: works
        feed(150, 100)
    feed(50, 250)
    got = torch.cat(outs, dim=0)
    assert got.dtype == F32
    ref = O.decoder_forward(O.encoder_forward_chunked(x[None], P, 2, 4, chunk_ends(300, chunks)), None, P)[0]
    assert rel_l2(got, ref) < 1e-2, rel_l2(got, ref)
    assert tr.close(0) == dec(got)
