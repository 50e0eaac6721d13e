"""Independent streams in one batch (conformer_amd/slots.py) on the MI355X.

Pinned here: the slots attention kernel against a float64 restatement (every head-dim class, both workgroup shapes, with and
without the key split, padded rows exactly zero, guard bands untouched, device offsets clamped); SlotStreamingEncoder against
the chunked float64 oracle and a one-utterance StreamingEncoder per utterance under staggered opens, ragged per-slot chunks,
buffering-only chunks and slot reuse; SlotTranscriber's text on close against BeamCTCDecoder in all four modes; neighbour
independence; the lockstep reduction to StreamingTranscriber; and the refusals, which leave the state as it was."""
import math

import pytest
import torch

from conformer_amd import _lib, ops
from conformer_amd.decode import BeamCTCDecoder
from oracle import conformer_oracle as O
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

VOCAB = ["<pad>"] + [chr(ord("a") + i) for i in range(14)] + ["|", "<unk>"]
UNK = 16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ---- 1. the attention kernel ---------------------------------------------------------------------------------------------

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


def _inputs(S, T, H, dh, dev, seed):
    d = H * dh
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(S, T, 3 * d, generator=g).to(dev)
    pos = (torch.randn(2 * T - 1, d, generator=g) * 0.5).to(dev)
    u, v = (torch.randn(d, generator=g) * 0.3).to(dev), (torch.randn(d, generator=g) * 0.3).to(dev)
    return qkv, pos, u, v


def _guarded(shape, dev, fill=float("nan"), G=4096):
    n = math.prod(shape)
    buf = torch.full((G + n + G,), 777.0, device=dev)
    buf[G:G + n] = fill
    return buf, buf[G:G + n].view(*shape), G


def _waves(nw):
    return _lib.load().cfm_debug_set_attention_waves(nw)


@pytest.mark.parametrize("nw", [4, 8])
@pytest.mark.parametrize("split", [False, True], ids=["nsplit1", "keysplit"])
@pytest.mark.parametrize("H,dh", [(4, 8), (4, 16), (2, 32), (2, 40), (2, 64)])
def test_attention_slots_vs_float64(dev, H, dh, split, nw):
    S, T, q_max = 5, 1000, 10
    d = H * dh
    qkv, pos, u, v = _inputs(S, T, H, dh, dev, seed=dh + 7 * nw)
    qb = [0, 37, 990, 500, 700]
    qc = [5, 0, 10, 3, 7]
    L = [b + c for b, c in zip(qb, qc)]
    keep = qkv.clone()
    buf, ctx, G = _guarded((S, q_max, d), dev)
    prev = _waves(nw)
    try:
        with torch.no_grad():
            ops.relpos_attention_slots(qkv, pos, u, v, torch.tensor(L, device=dev), H, torch.tensor(qb, device=dev),
                                       torch.tensor(qc, device=dev), q_max, ctx, keys_hint=None if split else 1)
        torch.cuda.synchronize()
    finally:
        _waves(prev)
    assert torch.all(buf[:G] == 777.0) and torch.all(buf[G + ctx.numel():] == 777.0)        # guard bands untouched
    assert torch.equal(qkv, keep)
    got = ctx.cpu()
    for b in range(S):
        assert torch.all(got[b, qc[b]:] == 0.0), b                                           # padded rows exactly zero
        if qc[b]:
            want = _restate(qkv, pos, u, v, H, b, range(qb[b], qb[b] + qc[b]), L[b])
            assert rel_l2(got[b, :qc[b]], want) < 2e-6, (b, rel_l2(got[b, :qc[b]], want))


@pytest.mark.parametrize("H,dh", [(4, 16), (2, 64)])
@pytest.mark.parametrize("split", [False, True], ids=["nsplit1", "keysplit"])
def test_attention_slots_with_identical_offsets_is_the_rows_kernel(dev, H, dh, split):
    S, T, n0, k = 5, 1000, 600, 8
    qkv, pos, u, v = _inputs(S, T, H, dh, dev, seed=3)
    lengths = torch.full((S,), n0 + k, device=dev, dtype=torch.int64)
    hint = None if split else 1
    with torch.no_grad():
        full = torch.zeros(S, T, H * dh, device=dev)
        ops.relpos_attention_rows(qkv, pos, u, v, lengths, H, n0, k, full, keys_hint=hint)
        got = ops.relpos_attention_slots(qkv, pos, u, v, lengths, H, torch.full((S,), n0, device=dev, dtype=torch.int64),
                                         torch.full((S,), k, device=dev, dtype=torch.int64), k, keys_hint=hint)
    assert rel_l2(got, full[:, n0:n0 + k]) <= 1e-6


@pytest.mark.parametrize("split", [False, True], ids=["nsplit1", "keysplit"])
def test_attention_slots_clamps_device_offsets(dev, split):
    """Out-of-range device values: the kernel clamps them (q_begin to [0,T], q_count to [0, min(q_max, T - q_begin)], lengths
    to T); nothing outside the cache, the table or ctx is touched and the clamped slots compute their clamped rows."""
    S, T, H, dh, q_max = 5, 1000, 4, 16, 8
    qkv, pos, u, v = _inputs(S, T, H, dh, dev, seed=5)
    big = 1 << 40
    qb = torch.tensor([-3, T + 5, big, 995, 0], device=dev)
    qc = torch.tensor([big, 4, 3, 100, -7], device=dev)
    L = torch.tensor([big, -1, 5, T, 0], device=dev)
    buf, ctx, G = _guarded((S, q_max, H * dh), dev)
    with torch.no_grad():
        ops.relpos_attention_slots(qkv, pos, u, v, L, H, qb, qc, q_max, ctx, keys_hint=None if split else 1)
    torch.cuda.synchronize()
    assert torch.all(buf[:G] == 777.0) and torch.all(buf[G + ctx.numel():] == 777.0)
    got = ctx.cpu()
    assert torch.all(got[1:3] == 0.0) and torch.all(got[4] == 0.0) and torch.all(got[3, 5:] == 0.0)
    assert rel_l2(got[0], _restate(qkv, pos, u, v, H, 0, range(0, q_max), T)) < 2e-6
    assert rel_l2(got[3, :5], _restate(qkv, pos, u, v, H, 3, range(995, 1000), T)) < 2e-6


# ---- 2.-6. encoder, transcriber ------------------------------------------------------------------------------------------

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
            u = owner[s]
            texts[u] = obj.close(s) if is_tr else obj.close(s)
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
        assert out.shape[:2] == (S, max(k))
        for s in range(S):
            if owner[s] is not None and k[s]:
                rows[owner[s]].append(out[s, :k[s]])
    for s in range(S):
        if owner[s] is not None and is_tr:
            texts[owner[s]] = obj.close(s)
    cat = {u: torch.cat(r, dim=0) if r else None for u, r in rows.items()}
    return chunks, cat, texts


def _single_stream_encoder(enc, x, chunks, dev):
    from conformer_amd.streaming import StreamingEncoder
    st = StreamingEncoder(enc, 1, x.shape[1])
    outs, t0 = [], 0
    with torch.no_grad():
        for c in chunks:
            outs.append(st.step(x[None, :, t0:t0 + c].float().to(dev)))
            t0 += c
    return torch.cat(outs, dim=1)[0]


@pytest.mark.parametrize("d,heads", [(32, 4), (48, 4), (512, 8)], ids=["small", "unfolded", "cfg5_width"])  # 48: not ln_fold_ok
def test_slot_encoder_matches_chunked_oracle(dev, d, heads):
    from conformer_amd.slots import SlotStreamingEncoder
    from conformer_amd.streaming import StreamingEncoder, chunk_ends
    m, P = _model(d, heads, 61, dev, hidden=8)
    utts = _utts(UTT_LEN, 3)
    enc = SlotStreamingEncoder(m.encoder, 4, 800)
    # it shares a base with the lockstep encoder but is not one: no (S, T'max, d) context scratch, no lockstep position, no graphs
    assert not isinstance(enc, StreamingEncoder)
    assert not any(hasattr(enc, name) for name in ("ctx", "frames", "tail_len", "use_graphs", "_graphs"))
    chunks, rows, _ = _drive(enc, 4, utts, SCHEDULE, dev)
    for u, x in enumerate(utts):
        assert sum(chunks[u]) == x.shape[1]
        ref = O.encoder_forward_chunked(x[None], P, 2, heads, chunk_ends(x.shape[1], chunks[u]))[0]
        assert rows[u].shape == ref.shape, u
        assert rel_l2(rows[u], ref) < 2e-5, (u, rel_l2(rows[u], ref))
        one = _single_stream_encoder(m.encoder, x, chunks[u], dev)
        assert rel_l2(rows[u], one) < 1e-5, (u, rel_l2(rows[u], one))


@pytest.fixture(scope="module")
def lm(tmp_path_factory):
    from conformer_amd.lm import NgramLanguageModel, write_synthetic_arpa
    p = tmp_path_factory.mktemp("lm") / "slots.arpa"
    write_synthetic_arpa(p, VOCAB[1:15], 30, [0, 150, 150], seed=4, max_tokens_per_word=2)
    return NgramLanguageModel.from_arpa(p)


def _decoder(mode, lm):
    return BeamCTCDecoder(VOCAB, 0, skip_ids=(UNK,), beam_width=16, lm=lm if "lm" in mode else None,
                          hotwords=["ab", "c d", "e"] if "hw" in mode else None, alpha=1.1, beta=2.0, hotword_weight=3.0)


@pytest.mark.parametrize("mode", ["plain", "lm", "hw", "lm_hw"])
def test_slot_transcriber_text_on_close(dev, lm, mode):
    from conformer_amd.slots import SlotTranscriber
    m, _ = _model(32, 4, 71, dev)
    dec = _decoder(mode, lm)
    utts = _utts(UTT_LEN, 5)
    tr = SlotTranscriber(m, dec, 4, 800)
    _, logits, texts = _drive(tr, 4, utts, SCHEDULE, dev, seed=1)
    assert set(texts) == set(range(len(utts)))
    for u in range(len(utts)):
        assert texts[u] == dec(logits[u]), (mode, u)


def test_neighbours_do_not_matter(dev):
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
    _, la, ta = _drive(SlotTranscriber(m, dec, 3, 600), 3, utts, a, dev, seed=2)
    _, lb, tb = _drive(SlotTranscriber(m, dec, 3, 600), 3, utts, b, dev, seed=3)
    assert rel_l2(la[0], lb[0]) < 1e-5 and ta[0] == tb[0]


def test_lockstep_is_the_streaming_transcriber(dev):
    from conformer_amd.slots import SlotTranscriber
    from conformer_amd.transcribe import StreamingTranscriber
    m, _ = _model(32, 4, 91, dev)
    dec = _decoder("plain", None)
    chunks = [64, 64, 7, 1, 130, 64]
    T, S = sum(chunks), 3
    x = torch.randn(S, 80, T, generator=torch.Generator().manual_seed(4)).to(dev)
    ref_tr, tr = StreamingTranscriber(m, dec, S, T), SlotTranscriber(m, dec, S, T)
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
    want_text = ref_tr.finish()
    assert [tr.close(s) for s in range(S)] == want_text


def test_refusals_leave_the_state_alone(dev):
    from conformer_amd.slots import SlotTranscriber
    from conformer_amd.streaming import chunk_ends
    m, P = _model(32, 4, 101, dev)
    dec = _decoder("plain", None)
    with pytest.raises(RuntimeError):
        SlotTranscriber(m.train(), dec, 2, 300)
    m.eval()
    tr = SlotTranscriber(m, dec, 2, 300)
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
        tr.step(torch.zeros(2, 80, 10, device=dev), [10, 5])           # frames for free slot 1
    with pytest.raises(RuntimeError):
        tr.open(0)                                                      # already open
    with pytest.raises(RuntimeError):
        tr.close(1)                                                     # free
    with pytest.raises(RuntimeError):
        tr.step(torch.zeros(2, 80, 201, device=dev), [201, 0])         # 301 > max_mel_frames
    with pytest.raises(RuntimeError):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            tr.step(torch.zeros(2, 80, 10, device=dev), [10, 0])
    m.train()
    with pytest.raises(RuntimeError):
        tr.step(torch.zeros(2, 80, 10, device=dev), [10, 0])
    m.eval()
    feed(150, 100)
    feed(50, 250)
    got = torch.cat(outs, dim=0)
    ref = O.decoder_forward(O.encoder_forward_chunked(x[None], P, 2, 4, chunk_ends(300, chunks)), None, P)[0]
    assert rel_l2(got, ref) < 2e-5
    assert tr.partial_text().keys() == {0}
    assert tr.close(0) == dec(got)
