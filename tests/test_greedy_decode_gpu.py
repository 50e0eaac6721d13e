"""The greedy CTC decode (csrc/train_aux.hip: frame_argmax_kernel + ctc_collapse_kernel) bit for bit against torch.argmax on
the CPU and the oracle's collapse (O.greedy_decode_ids), at the edges random logits never arrange: the arg-max at every
vocabulary size around the 64-lane stride with the maximum, exact ties, infinities, signed zeros and NaNs placed by lane and
by stride iteration (NaN is the greatest value and the first one wins, as in torch.argmax: every id lies in [0, V)); the
collapse on designed id sequences whose pads line up with the 64-frame blocks (a whole block skipped, a block whose first
valid frame must read the carry, the reference's no-reset rule across blocks); `lengths` at 0, 1, the block edges, T, beyond
T and negative; and the entry's writes next to sentinels."""
import numpy as np
import pytest
import torch

from oracle import conformer_oracle as O

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def decode(logits, pad_id, unk_id, dev, lengths=None):
    from conformer_amd.decode import greedy_ctc_decode
    out = greedy_ctc_decode(logits.to(dev), pad_id, unk_id, None if lengths is None else lengths.to(dev))
    return [t.cpu() for t in out]


# ---- arg-max ------------------------------------------------------------------------------------------------------------------
def argmax_rows(V):
    """Designed rows of V logits, (name, row); a design that needs more columns than V is left out."""
    g = torch.Generator().manual_seed(V)
    rows = []

    def base():
        return torch.randn(V, generator=g)                       # (|x| < 6: below every planted value)

    def plant(name, cols, value, fill=None):
        if cols and max(cols) < V and len(set(cols)) == len(cols):
            row = base() if fill is None else torch.full((V,), fill)
            row[list(cols)] = value
            rows.append((name, row))

    rows.append(("random", base()))
    for c in (0, 63, 64, V - 1):
        plant(f"maximum at {c}", (c,), 10.0)
    plant("tie in two lanes of one iteration", (3, 17), 7.0)
    plant("tie in one lane across iterations", (5, 69), 7.0)
    plant("tie in one lane, three iterations", (6, 70, 134), 7.0)
    plant("tie across the shuffle halves", (5, 37), 7.0)
    plant("tie, later lane in the earlier iteration", (40, 66), 7.0)
    plant("tie with column 0", (0, V - 1), 7.0)
    plant("tie with column 0 and 64", (0, 64), 7.0)
    rows.append(("all equal", torch.zeros(V)))
    rows.append(("all -inf", torch.full((V,), -INF)))
    plant("one finite among -inf", (V - 1,), -3.0e38, fill=-INF)
    plant("one +inf", (V // 2,), INF)
    plant("two +inf", (1, V - 1), INF)
    plant("all +inf", tuple(range(V)), INF)
    if V >= 2:
        z = torch.full((V,), -1.0)
        z[0], z[V - 1] = -0.0, 0.0
        rows.append(("-0.0 before 0.0", z))
        z = torch.full((V,), -1.0)
        z[0], z[V - 1] = 0.0, -0.0
        rows.append(("0.0 before -0.0", z))
    plant("one NaN", (V // 3,), NAN)
    plant("one NaN, last column", (V - 1,), NAN)
    if V >= 3:
        r = base()
        r[0], r[V // 2], r[V - 1] = NAN, INF, NAN
        rows.append(("NaN before and after +inf", r))
        r = base()
        r[0], r[V - 1] = INF, NAN
        rows.append(("NaN after +inf", r))
    plant("NaNs in two lanes", (2, 9), NAN)
    plant("NaNs across the shuffle halves", (37, 5), NAN)
    plant("NaNs in one lane", (5, 69), NAN)
    plant("NaNs, later lane in the earlier iteration", (40, 66), NAN)
    plant("NaN at 64 against a maximum at 0", (64,), NAN)
    rows.append(("all NaN", torch.full((V,), NAN)))
    plant("all NaN but column 0", tuple(range(1, V)), NAN)
    return rows


@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 127, 128, 129, 370])
def test_argmax_is_torch_argmax(dev, V):
    names, rows = zip(*argmax_rows(V))
    x = torch.stack(rows)
    want = torch.argmax(x, dim=-1)
    nan_rows = torch.isnan(x).any(-1)
    first_nan = torch.isnan(x).float().argmax(-1)
    assert torch.equal(want[nan_rows], first_nan[nan_rows])       # (the reference's rule, restated: the first NaN)
    n = x.shape[0]
    # the rows as one utterance of n frames, as n utterances of one frame, and the first 1 and 9 alone (B T = 1, 9: no multiple of 4)
    for shape, sel in (((1, n), slice(None)), ((n, 1), slice(None)), ((1, 1), slice(0, 1)), ((3, 3), slice(0, 9)), ((1, 9), slice(n - 9, n))):
        sub = x[sel]
        if sub.shape[0] != shape[0] * shape[1]:
            continue
        ids, tokens, counts = decode(sub.reshape(*shape, V), V, V + 1, dev)       # pad / unk outside the vocabulary: nothing skipped
        got = ids.reshape(-1)
        bad = [(names[sel][i], int(got[i]), int(want[sel][i])) for i in range(got.numel()) if got[i] != want[sel][i]]
        assert not bad, f"V={V} shape={shape}: (row, frame_ids, torch.argmax) {bad}"
        assert int(got.min()) >= 0 and int(got.max()) < V
        assert int(tokens.max()) < V and int(tokens.min()) >= -1


# ---- collapse ---------------------------------------------------------------------------------------------------------------
V6, PAD, UNK = 6, 0, 1


def one_hot(ids, V=V6):
    """(B, T, V) logits whose arg-max is ids (B, T)"""
    ids = torch.as_tensor(ids)
    x = torch.zeros(*ids.shape, V)
    x.scatter_(-1, ids.unsqueeze(-1), 5.0)
    return x


def check_collapse(dev, ids, pad_id, unk_id, lengths=None, what=""):
    ids = torch.as_tensor(ids)
    B, T = ids.shape
    x = one_hot(ids)
    frame_ids, tokens, counts = decode(x, pad_id, unk_id, dev, lengths)
    assert torch.equal(frame_ids, ids), what                     # all T frames, whatever the lengths
    for b in range(B):
        n = T if lengths is None else min(T, max(0, int(lengths[b])))
        _, want = O.greedy_decode_ids(x[b, :n], pad_id, unk_id)
        c = int(counts[b])
        assert c == len(want) and tokens[b, :c].tolist() == want, f"{what} row {b}: {tokens[b, :c].tolist()} vs {want}"
        assert (tokens[b, c:] == -1).all(), f"{what} row {b}: tokens behind the count"
    return tokens, counts


def designed(T):
    """name -> id sequence of T frames over {pad 0, unk 1, labels 2..5}; designs are cut at T"""
    def seq(fill=PAD):
        return [fill] * 260

    out = {}
    s = seq()
    s[60:68] = [2] * 8
    s[124:132] = [3] * 8
    out["runs across 63|64 and 127|128"] = s
    out["one run through every block"] = seq(2)
    s = seq()
    s[10], s[128], s[129] = 2, 2, 3                               # block 1 is all pads: the carry survives it, the 2 at 128 is dropped
    out["no reset across a whole skipped block"] = s
    s = seq()
    s[63], s[128], s[129] = 2, 2, 3                               # ... with the label in the block's last lane
    out["no reset, label in lane 63"] = s
    s = seq(UNK)
    s[50], s[70], s[71] = 4, 4, 5                                 # trailing skips behind 50; 70 is its block's first valid frame
    out["first valid frame continues the previous block"] = s
    s = seq()
    s[50], s[64], s[65] = 4, 4, 5                                 # ... in lane 0
    out["lane 0 continues the previous block"] = s
    s = seq()
    s[0], s[64], s[128], s[192] = 2, 3, 3, 2                      # lane 0 of every block reads the carry
    out["lane 0 of every block"] = s
    out["pads and unks only"] = [PAD, UNK] * 130
    out["labels alternating every frame"] = [2, 3] * 130
    out["three labels, runs of three"] = ([2] * 3 + [3] * 3 + [4] * 3) * 29
    return {k: v[:T] for k, v in out.items()}


@pytest.mark.parametrize("T", [1, 63, 64, 65, 127, 128, 129, 200])
def test_collapse_on_designed_sequences(dev, T):
    d = designed(T)
    names, ids = list(d), torch.tensor(list(d.values()))
    tokens, counts = check_collapse(dev, ids, PAD, UNK, what=f"T={T}")
    c = dict(zip(names, counts.tolist()))
    assert c["pads and unks only"] == 0 and (tokens[names.index("pads and unks only")] == -1).all()
    assert c["labels alternating every frame"] == T and (tokens[names.index("labels alternating every frame")] != -1).all()
    assert c["one run through every block"] == 1
    if T >= 130:
        assert tokens[names.index("no reset across a whole skipped block"), :3].tolist() == [2, 3, -1]
        assert tokens[names.index("no reset, label in lane 63"), :3].tolist() == [2, 3, -1]
        assert tokens[names.index("first valid frame continues the previous block"), :3].tolist() == [4, 5, -1]
        assert tokens[names.index("lane 0 of every block"), :4].tolist() == [2, 3, 2, -1]
    # the same sequences with pad_id == unk_id (unk frames are then labels), and with pad ids no frame can hold
    check_collapse(dev, ids, PAD, PAD, what=f"T={T} pad == unk")
    _, counts = check_collapse(dev, ids, V6, V6 + 5, what=f"T={T} pad outside the vocabulary")
    assert dict(zip(names, counts.tolist()))["pads and unks only"] == T
    check_collapse(dev, ids, -1, -1, what=f"T={T} pad = unk = -1")


@pytest.mark.parametrize("seed", range(6))
def test_collapse_on_random_sequences_with_many_skips(dev, seed):
    g = torch.Generator().manual_seed(seed)
    B, T = 8, 200
    skip = torch.rand(B, T, generator=g) < 0.7
    ids = torch.where(skip, torch.randint(0, 2, (B, T), generator=g), torch.randint(2, 4, (B, T), generator=g))
    check_collapse(dev, ids, PAD, UNK, what=f"seed {seed}")
    lengths = torch.randint(0, T + 1, (B,), generator=g)
    check_collapse(dev, ids, PAD, UNK, lengths, what=f"seed {seed} with lengths")


# ---- lengths ------------------------------------------------------------------------------------------------------------------
def test_lengths_are_clamped_and_nothing_behind_them_is_decoded(dev):
    T = 130
    lengths = torch.tensor([0, 1, 63, 64, 65, T, T + 5, -3])
    ids = torch.tensor([[2, 3] * (T // 2)] * len(lengths))
    ids[:, 40:50] = PAD
    for b, n in enumerate(lengths.tolist()):
        ids[b, max(0, n):] = 5                                   # the label 5 only ever sits behind the length
    tokens, counts = check_collapse(dev, ids, PAD, UNK, lengths)
    assert not (tokens == 5).any()
    assert counts.tolist() == [0, 1, 53, 54, 55, 120, 120, 0]
    x = one_hot(ids)
    assert torch.equal(decode(x, PAD, UNK, dev, lengths)[0], x.argmax(-1))


# ---- write guard ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,V", [(3, 70, 6), (1, 1, 1), (2, 129, 65)])
def test_entry_writes_stay_inside_its_outputs(dev, B, T, V):
    from conformer_amd import _lib, ops
    GUARD, SENT = 64, -0x0123456789ABCDEF
    g = torch.Generator().manual_seed(B + T)
    x = (torch.randn(B, T, V, generator=g) * 3).to(dev)
    lengths = torch.randint(0, T + 2, (B,), generator=g).to(dev)

    def guarded(n):
        buf = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.int64, device=dev)
        return buf, buf[GUARD:GUARD + n]
    (bf, frame_ids), (bt, tokens), (bc, counts) = guarded(B * T), guarded(B * T), guarded(B)
    _lib.call("cfm_greedy_ctc_decode_f32", x.data_ptr(), lengths.data_ptr(), frame_ids.data_ptr(), tokens.data_ptr(),
              counts.data_ptr(), B, T, V, 0, 1 % V, ops._stream())
    for name, buf in (("frame_ids", bf), ("tokens", bt), ("counts", bc)):
        assert (buf[:GUARD] == SENT).all() and (buf[-GUARD:] == SENT).all(), f"a write outside {name}"
        assert not (buf[GUARD:-GUARD] == SENT).any(), f"{name} not written everywhere"
    want = decode(x.cpu(), 0, 1 % V, dev, lengths.cpu())
    assert torch.equal(frame_ids.cpu().view(B, T), want[0]) and torch.equal(tokens.cpu().view(B, T), want[1])
    assert torch.equal(counts.cpu(), want[2]) and torch.equal(want[0], x.cpu().argmax(-1))
