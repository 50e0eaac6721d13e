"""The resampler (conformer_amd/resample.py, csrc/resample.hip) on the MI355X.

Pinned here: the offline call against the float64 restatement at the worst-case fp32 bound, ragged lengths around every edge of
the bank and of the kernel's workgroup run, NaN behind every length; streams cut into chunks against the whole utterance bit
for bit under staggered opens, slot reuse, zero-count steps and every kind of flush; the kernel alone on a hand-built table with
an integer bank (every sum exact, so outputs, zero fill and tails are compared exactly), its clamping of a corrupt table and its
refusals; int16 and interleaved input against the float path bit for bit; the composed front end against the float64 log-mel of
the float64-resampled utterance alone, and SlotTranscriber.step_audio at 48 kHz int16 stereo against the 16 kHz stream; the
refusals, which leave the state as it was.

The restatement and the CPU half are tests/resample_restatement.py and tests/test_resample_cpu.py.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import frontend_oracle as FO
from tests import resample_restatement as R
from tests import test_frontend_cpu as C
from tests import test_resample_cpu as RC
from tests.test_frontend_stages_gpu import carved, e2e_check, status
from tests.test_stream_frontend_gpu import _decoder, _model
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
OK, BAD_SHAPE, UNSUPPORTED, NULL, ALIGN = 0, -1, -2, -3, -6
RUN, XS_FLOATS = 1024, 12288          # csrc/resample.hip: outputs per workgroup at most, LDS floats of its staged input span


def workgroup_run(o, n, width):
    """The outputs one workgroup computes: whole blocks of n, RUN at most, their input span inside the LDS buffer."""
    return min(max(1, RUN // n), (XS_FLOATS - 2 * width) // o) * n


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conformer_amd import _lib
    assert _lib.load().cfm_device_check() == 0, "not a gfx950 device"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def resampler(r_in, dev):
    from conformer_amd.resample import Resampler
    return Resampler(r_in, 16000, device=dev)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


# ---- 1. offline against the restatement --------------------------------------------------------------------------------------
def launch_offline(dev, rs, x, lengths, ld_y):
    """The offline launch (no tails, lead = width, every row flushed) into a NaN-filled carved y: (y on the host, band ok)."""
    B = x.shape[0]
    y, band = carved(B * ld_y, dev)
    table = torch.tensor([(0, v, rs.width, rs.output_length(v), 1, 0, 0, 0) for v in lengths], dtype=torch.int32).to(dev)
    rs.launch(x, x.shape[2] if x.dim() == 3 else 1, x.shape[1], None, table, y.view(B, ld_y))
    torch.cuda.synchronize()
    assert bool(torch.isnan(band).all()), "a write behind the end of y"
    return y.view(B, ld_y).cpu().numpy()


@pytest.mark.parametrize("r_in", [8000, 11025, 32000, 44100, 48000])
def test_offline_against_float64(dev, r_in):
    k, o, n, width = RC.bank(r_in)
    K = k.shape[1]
    run = workgroup_run(o, n, width)
    past_run = next(L for L in range(1, 1 << 20) if R.out_len(L, o, n) > run)          # ends in the second workgroup, as early as can be
    assert R.out_len(past_run - 1, o, n) <= run < R.out_len(past_run, o, n) <= run + max(1, -(-n // o))
    pool = [1, o - 1, o, o + 1, width, width + 1, K - 1, K, K + 1, 2999, past_run, 1]
    rng = np.random.default_rng(r_in)
    rng.shuffle(pool)
    rs = resampler(r_in, dev)
    worst = 0.0
    for lengths in (pool[i:i + 3] for i in range(0, 12, 3)):
        Lmax = max(lengths)
        x = np.full((3, Lmax), np.nan, np.float32)
        for b, L in enumerate(lengths):
            x[b, :L] = rng.standard_normal(L)
        ld_y = (R.out_len(Lmax, o, n) + 3) // 4 * 4
        xd = torch.from_numpy(x).to(dev)
        y = launch_offline(dev, rs, xd, lengths, ld_y)
        assert np.isfinite(y).all(), "an output read a sample behind its row's length, or was never written"
        for b, L in enumerate(lengths):
            want, mass = R.resample64(x[b, :L].astype(np.float64), k, o, width)
            assert len(want) == R.out_len(L, o, n)
            err = np.abs(y[b, :len(want)].astype(np.float64) - want)
            bound = (K + 2) * 2.0 ** -24 * mass + 1e-30
            worst = max(worst, float((err / bound).max()) if len(want) else 0.0)
            assert (err <= bound).all(), (r_in, L, float((err / bound).max()))
            assert not y[b, len(want):].any(), "outputs behind ceil(n len / o) must be zero"
        got, out = rs(xd, lengths)                                        # the public call: the same launch
        assert out == [R.out_len(L, o, n) for L in lengths] and got.shape == (3, R.out_len(Lmax, o, n))
        assert np.array_equal(bits(got.cpu().numpy()), bits(y[:, :got.shape[1]]))
    print(f"offline {r_in}: worst error / bound = {worst:.3f}")


# ---- 2. chunked equals whole, bit for bit ------------------------------------------------------------------------------------
def schedule(o):
    """Every step: closes (slot list), then opens ({slot: utterance}), the samples each slot takes, the slots flushed with it."""
    return [
        dict(open={0: 0, 1: 1, 2: 2}, samples={0: 1, 1: 1, 2: o + 5}, flush=[1, 2]),   # a 1-sample stream and one of o + 5, flushed at once
        dict(open={1: 3, 3: 4}, samples={0: o - 1, 1: 300, 3: o}),                     # slot 1 reused; utterance 3 is dropped below
        dict(samples={0: o, 3: 0}),
        dict(close=[1], open={1: 5, 2: 6}, samples={0: 3000, 1: 2 * o + 1, 2: 7, 3: 1234}),
        dict(samples={0: 0, 1: 4000, 3: 0}, flush=[3]),                                # a flush with no samples
        dict(samples={}),                                                              # nobody brings anything
        dict(samples={0: 2500, 1: 1777, 2: 0}, flush=[0, 1, 2]),
    ]


def utterances(sched, seed):
    """One noise stream per utterance of the schedule, as long as the schedule feeds it."""
    owner, total = {}, {}
    for st in sched:
        for s, u in st.get("open", {}).items():
            owner[s] = u
        for s, c in st["samples"].items():
            total[owner[s]] = total.get(owner[s], 0) + c
    return {u: C.noise(1, L, seed + u)[0].numpy() for u, L in total.items()}


def drive(step, is_open, open_, close, S, sched, utts, dev):
    """Run a schedule: {utterance: what its slot returned, step by step}.  Samples a slot does not take are NaN."""
    owner, pos, got = [None] * S, {}, {}
    for st in sched:
        for s in st.get("close", []):
            close(s)
            owner[s] = None
        for s, u in st.get("open", {}).items():
            assert not is_open()[s]
            open_(s)
            owner[s], pos[u], got[u] = u, 0, []
        counts = [0] * S
        N = max([0] + list(st["samples"].values()))
        x = np.full((S, N), np.nan, np.float32)
        for s, c in st["samples"].items():
            u = owner[s]
            x[s, :c] = utts[u][pos[u]:pos[u] + c]
            pos[u] += c
            counts[s] = c
        flush = st.get("flush", [])
        out, k = step(torch.from_numpy(x).to(dev), counts, flush)
        for s in range(S):
            if owner[s] is not None:
                got[owner[s]].append((out[s], k[s]))
        for s in flush:
            assert not is_open()[s]                                       # a flushed slot is free
            owner[s] = None
    assert all(pos[u] == len(utts[u]) for u in utts)
    return got


@pytest.mark.parametrize("r_in", [44100, 48000])
def test_chunked_equals_whole(dev, r_in):
    from conformer_amd.resample import StreamingResampler
    rs = resampler(r_in, dev)
    o, n, width = rs.o, rs.n, rs.width
    sched = schedule(o)
    utts = utterances(sched, 300)
    counts = {c for st in sched for c in st["samples"].values()}
    assert {0, 1, o - 1, o, 3000, 4000} <= counts and len(utts[1]) == 1 and len(utts[2]) == o + 5
    srs = StreamingResampler(rs, 4, 4000)

    def step(x, counts, flush):
        y, k = srs.step(x, counts, flush)
        assert y.shape == (4, srs.out_cap) and max(k) <= srs.out_cap
        y = y.cpu().numpy()
        assert np.isfinite(y).all(), "a neighbour's unused samples were read, or a float of y was not written"
        for s in range(4):
            assert not y[s, k[s]:].any(), "zeros behind a slot's outputs"
        return y, k

    got = drive(step, lambda: srs.is_open, srs.open, srs.close, 4, sched, utts, dev)
    assert srs.is_open == [False] * 4
    for u, x in utts.items():
        if u == 3:
            continue                                                      # dropped without a flush
        whole, (total,) = rs(torch.from_numpy(x[None].copy()).to(dev))
        whole = whole[0].cpu().numpy()
        mine = np.concatenate([y[:k] for y, k in got[u]])
        assert total == R.out_len(len(x), o, n) == len(mine), (u, total, len(mine))
        assert np.array_equal(bits(mine), bits(whole)), f"utterance {u}: chunking changed a bit"
    # the dropped stream: what it emitted before the close is the head of its whole
    x = utts[3]
    whole = rs(torch.from_numpy(x[None].copy()).to(dev))[0][0].cpu().numpy()
    mine = np.concatenate([y[:k] for y, k in got[3]])
    assert len(mine) == n * R.blocks_emitted(300, width, o) and np.array_equal(bits(mine), bits(whole[:len(mine)]))


# ---- 3. the kernel alone -----------------------------------------------------------------------------------------------------
def integer_case(o, n, width, seed):
    """An integer bank and integer streams: every product and partial sum is an integer below 2^24, so fp32 is exact in any
    order.  Rows: a stream's first step past the workgroup run, a first step with no output, mid-stream, two flushes (one of a
    1-sample stream), no new samples, a free slot."""
    rng = np.random.default_rng(seed)
    K = 2 * width + o
    k = rng.integers(-8, 9, (n, K)).astype(np.float64)
    run = workgroup_run(o, n, width)
    big = (run // n + 1 + (run // n) * 4 // 10) * o + width               # 1.4 runs of blocks, two at the least
    rows = [(0, big, False), (2, 1, False), (5 * o + 3, 3 * o + width, False), (4 * o, 3, True), (0, 1, True), (6 * o + 1, 0, False),
            None]
    S, N = len(rows), big + 3
    samples = rng.integers(-8, 9, (S, N)).astype(np.float32)              # (columns behind a slot's count: never read)
    tail_in = np.full((S, R.TAIL_LD), 9.0, np.float32)                    # (floats behind a slot's tail length: never read)
    steps = []
    for b, r in enumerate(rows):
        if r is None:
            steps.append(None)
            continue
        before, n_new, flush = r
        st = R.Stream(k, o, width, np.float32)
        st.step(rng.integers(-8, 9, before).astype(np.float32))
        tail_in[b, :len(st.tail)] = st.tail
        steps.append(st.step(samples[b, :n_new], flush))
    return k, samples, tail_in, steps, run


def launch(dev, name, samples, C_, tail_in, table, bank_t, o, n, width, ld_y, n_max=None):
    """One launch into NaN-filled carved buffers: (y (S, ld_y), tail_out (S, 1024)) on the host, bands checked."""
    from conformer_amd import _lib, ops
    S = table.shape[0]
    y, yband = carved(S * ld_y, dev)
    tails, tband = carved(S * R.TAIL_LD, dev)
    sd, td = torch.from_numpy(samples).to(dev), torch.from_numpy(tail_in).to(dev)
    tab, bk = torch.from_numpy(table).to(dev), torch.from_numpy(bank_t).to(dev)
    frames = samples.shape[1]
    _lib.call(name, sd.data_ptr(), frames * C_, frames if n_max is None else n_max, C_, td.data_ptr(), tails.data_ptr(),
              tab.data_ptr(), bk.data_ptr(), o, n, width, y.data_ptr(), ld_y, S, ops._stream())
    torch.cuda.synchronize()
    assert bool(torch.isnan(yband).all()) and bool(torch.isnan(tband).all()), "a write behind the end of y or of the tails"
    return y.view(S, ld_y).cpu().numpy(), tails.view(S, R.TAIL_LD).cpu().numpy()


def expected(steps, ld_y):
    S = len(steps)
    y, tails, table = np.zeros((S, ld_y), np.float32), np.zeros((S, R.TAIL_LD), np.float32), np.zeros((S, 8), np.int32)
    for b, st in enumerate(steps):
        if st is not None:
            y[b, :len(st["y"])] = st["y"]
            tails[b, :len(st["tail_out"])] = st["tail_out"]
            table[b] = st["row"]
    return y, tails, table


# (o, n, width): a bank held in LDS, one read from memory (n K > 2048), one with many phases and a one-block run
@pytest.mark.parametrize("o,n,width", [(3, 2, 4), (9, 40, 30), (7, 600, 3), (1, 1, 0)])
def test_kernel_bit_exact(dev, o, n, width):
    k, samples, tail_in, steps, run = integer_case(o, n, width, 7 * o + n)
    most = max(len(s["y"]) for s in steps if s is not None)
    assert most > run, "a row must reach into a second workgroup"
    ld_y = (most + 3) // 4 * 4 + 8
    want_y, want_tails, table = expected(steps, ld_y)
    assert table[0][2] == width and table[3][4] == table[4][4] == 1 and table[5][1] == 0 and (width == 0 or table[1][3] == 0)
    assert width == 0 or (table[5][0] == table[5][6] > 0 and table[5][5] == 0)      # 0 new samples: the tail goes across unchanged
    y, tails = launch(dev, "cfm_resample_f32", samples, 1, tail_in, table, np.ascontiguousarray(k.T, np.float32), o, n, width, ld_y)
    assert np.isfinite(y).all() and np.isfinite(tails).all(), "a float of a pitch or a tail row was never written"
    assert np.array_equal(y, want_y)
    assert np.array_equal(tails, want_tails)
    assert not tails[3].any() and not tails[4].any() and not tails[6].any() and not y[6].any()


def test_kernel_clamps_a_corrupt_table(dev):
    """Table values out of range are clamped before they index anything: the launch stays inside its buffers (bands untouched,
    everything written and finite) and the rows that are in range come out as without the neighbours' junk."""
    o, n, width = 9, 40, 30
    k, samples, tail_in, steps, run = integer_case(o, n, width, 99)
    N = samples.shape[1]
    tail_in = np.random.default_rng(3).integers(-8, 9, tail_in.shape).astype(np.float32)
    tail_in[2, :len(steps[2]["tail_in"])] = steps[2]["tail_in"]
    tail_in[3, :len(steps[3]["tail_in"])] = steps[3]["tail_in"]
    big = 1 << 30
    ld_y = 2 * run + 8
    table = np.array([(big, big, big, big, 0, big, big, big),
                      (-5, -5, -5, -5, -5, -5, -5, -5),
                      steps[2]["row"],
                      steps[3]["row"],
                      (0, 0, 0, 3, 1, 0, 0, 0),                           # outputs asked of an empty slot
                      (1024, N, 0, big, 1, -big, big, 0),
                      (100, 10, big, -1, 0, 200, 1024, 7)], np.int32)
    y, tails = launch(dev, "cfm_resample_f32", samples, 1, tail_in, table, np.ascontiguousarray(k.T, np.float32), o, n, width, ld_y)
    assert np.isfinite(y).all() and np.isfinite(tails).all()
    for b in (2, 3):
        want = np.zeros(ld_y, np.float32)
        want[:len(steps[b]["y"])] = steps[b]["y"]
        assert np.array_equal(y[b], want) and np.array_equal(tails[b, :len(steps[b]["tail_out"])], steps[b]["tail_out"])
    assert not y[1].any() and not tails[1].any() and not y[4].any() and not tails[4].any() and not tails[5].any()
    assert not y[6].any() and not tails[6].any()                         # keep clamps to m = 110: nothing left to carry


def test_kernel_refusals(dev):
    S, N, ld_y = 2, 64, 64
    smp = torch.zeros(S * N * 2, device=dev)
    tin, tab = torch.zeros(S * 1024, device=dev), torch.zeros(S * 8, device=dev, dtype=torch.int32)
    bk = torch.zeros(1024 * 4 + 4, device=dev)
    y, yband = carved(S * ld_y, dev)
    tout, tband = carved(S * 1024, dev)
    s, i, t_, k, t, yy = smp.data_ptr(), tin.data_ptr(), tout.data_ptr(), bk.data_ptr(), tab.data_ptr(), y.data_ptr()
    for name in ("cfm_resample_f32", "cfm_resample_i16"):
        def st(samples=s, ld=N, n_max=N, C_=1, ti=i, to=t_, table=t, bank=k, o=3, n=2, width=4, out=yy, ldy=ld_y, S_=S):
            return status(name, samples, ld, n_max, C_, ti, to, table, bank, o, n, width, out, ldy, S_)
        assert st(samples=None) == NULL and st(table=None) == NULL and st(bank=None) == NULL and st(out=None) == NULL
        assert st(ti=None) == NULL and st(to=None) == NULL                  # one tail without the other
        assert st(S_=0) == BAD_SHAPE and st(n_max=-1) == BAD_SHAPE and st(C_=0) == BAD_SHAPE and st(o=0) == BAD_SHAPE
        assert st(n=0) == BAD_SHAPE and st(width=-1) == BAD_SHAPE and st(ldy=62) == BAD_SHAPE and st(ldy=-4) == BAD_SHAPE
        assert st(ld=N - 1) == BAD_SHAPE and st(C_=2, ld=2 * N - 1) == BAD_SHAPE
        assert st(o=1000, width=13) == UNSUPPORTED and st(o=1, width=512) == UNSUPPORTED      # K = 1026, 1025
        assert st(n=641) == UNSUPPORTED and st(C_=9, ld=9 * N) == UNSUPPORTED
        assert st(to=i) == UNSUPPORTED and st(to=i + 4 * 1024) == UNSUPPORTED                  # the tails in place, overlapping
        assert st(out=yy + 4) == ALIGN and st(bank=k + 4) == ALIGN and st(ti=i + 4, to=t_ + 4) == ALIGN
        assert st(samples=s + 1) == ALIGN
        torch.cuda.synchronize()
        assert bool(torch.isnan(y).all()) and bool(torch.isnan(tout).all())               # the refused calls wrote nothing
        assert st() == OK and st(C_=2, ld=2 * N) == OK and st(o=1022, width=1, n=1) == OK and st(o=1, n=640, width=511) == OK
        assert st(samples=None, ld=0, n_max=0) == OK                                     # no samples at all: null is allowed
        assert st(ti=None, to=None) == OK                                                # the offline form: no tails
        torch.cuda.synchronize()
        assert not y.any() and not tout.any() and bool(torch.isnan(yband).all()) and bool(torch.isnan(tband).all())
        y.fill_(float("nan")), tout.fill_(float("nan"))


# ---- 4. formats --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r_in", [44100, 8000])
def test_int16_and_interleaved_equal_the_float_path(dev, r_in):
    rs = resampler(r_in, dev)
    rng = np.random.default_rng(4)
    lengths = [1500, 1499, 640]
    for Cn in (1, 2, 3):
        v = rng.integers(-32768, 32768, (3, 1500, Cn)).astype(np.int16)
        f = rng.standard_normal((3, 1500, Cn)).astype(np.float32)
        f[0, 0], f[0, 1] = [1.0, 2.0 ** -24, 2.0 ** -24][:Cn], [2.0 ** -24, 2.0 ** -24, 1.0][:Cn]   # (the order of the sum shows)
        for x, mono in ((v, R.downmix(R.from_int16(v))), (f, R.downmix(f))):
            xin = torch.from_numpy(x[:, :, 0].copy() if Cn == 1 else x).to(dev)
            got, out = rs(xin, lengths)
            want, out2 = rs(torch.from_numpy(mono).to(dev), lengths)
            assert out == out2 and np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy())), (Cn, x.dtype)
            assert bool(got.abs().sum() > 0)


def test_equal_rates_pass_through(dev):
    rs = resampler(16000, dev)
    assert (rs.o, rs.n, rs.width, rs.K) == (1, 1, 0, 1)
    rng = np.random.default_rng(5)
    lengths = [1300, 1, 1025]
    f = rng.standard_normal((3, 1300)).astype(np.float32)
    f[0, :4] = [-0.0, 0.0, np.float32(1e-45), -np.float32(3e38)]
    v = rng.integers(-32768, 32768, (3, 1300, 2)).astype(np.int16)
    for x, mono in ((f, f), (v, R.downmix(R.from_int16(v)))):
        xin = x.copy()
        for b, L in enumerate(lengths):
            xin[b, L:] = np.nan if x.dtype == np.float32 else 77
        got, out = rs(torch.from_numpy(xin).to(dev), lengths)
        got = got.cpu().numpy()
        assert out == lengths and got.shape == (3, 1300)
        for b, L in enumerate(lengths):
            assert np.array_equal(bits(got[b, :L]), bits(mono[b, :L])) and not bits(got[b, L:]).any()


# ---- 5. end to end -----------------------------------------------------------------------------------------------------------
def composed(dev, r_in, slots, max_chunk):
    from conformer_amd.frontend import ConformerAudioFrontend
    from conformer_amd.stream_frontend import StreamingAudioFrontend
    return StreamingAudioFrontend(ConformerAudioFrontend(device=dev), slots, max_chunk, input=resampler(r_in, dev))


@functools.lru_cache(maxsize=None)
def e2e_reference(r_in, L, seed):
    """(the stream at r_in, the float64 log-mel of its float64 resampling alone): computed once, shared, never changed."""
    k, o, n, width = RC.bank(r_in)
    x = C.noise(1, L, seed)[0].numpy()
    y64, _ = R.resample64(x.astype(np.float64), k, o, width)
    ref = FO.log_mel_numpy64(y64[None])[0]
    ref.setflags(write=False)
    assert C.floor_share(ref) == 0.0
    return x, ref


@pytest.mark.parametrize("r_in", [48000, 44100])
def test_composed_front_end_against_float64(dev, r_in):
    """Two streams in uneven chunks, one flushed with its last samples and one in a step of its own."""
    fe = composed(dev, r_in, 2, 6000)
    Ls = (15001, 9000)
    streams = [e2e_reference(r_in, L, 40 + i) for i, L in enumerate(Ls)]
    steps = [(1, 0), (700, 441), (0, 3), (4999, 2556), (6000, 6000), (3301, 0), (0, 0)]
    assert tuple(sum(c) for c in zip(*steps)) == Ls
    flushes = {5: [0], 6: [1]}
    fe.open(0), fe.open(1)
    got, pos = [[], []], [0, 0]
    for i, counts in enumerate(steps):
        x = np.full((2, max(counts)), np.nan, np.float32)
        for s, c in enumerate(counts):
            x[s, :c] = streams[s][0][pos[s]:pos[s] + c]
            pos[s] += c
        mel, frames = fe.step(torch.from_numpy(x).to(dev), counts, flushes.get(i, []))
        assert mel.shape == (2, 80, max(frames))
        for s in range(2):
            got[s].append(mel[s, :, :frames[s]].cpu())
    assert fe.is_open == [False, False] == fe.input.is_open
    o, n = fe.input.rs.o, fe.input.rs.n
    for s, L in enumerate(Ls):
        mel = torch.cat(got[s], dim=1).numpy()
        ref = streams[s][1]
        assert mel.shape == ref.shape == (80, R.out_len(L, o, n) // 160 + 1)
        e2e_check(mel, ref, f"{r_in} Hz stream {s}")


def test_slot_transcriber_at_48k_int16_stereo(dev):
    """step_audio fed 48 kHz int16 stereo returns the logits and the text of step_audio fed the 16 kHz float32 stream the offline
    Resampler makes of the same audio, cut where the streaming resampler cuts it: exactly."""
    from conformer_amd.frontend import ConformerAudioFrontend
    from conformer_amd.slots import SlotTranscriber
    from conformer_amd.stream_frontend import StreamingAudioFrontend
    m, _ = _model(32, 4, 71, dev)
    S = 2
    rs = resampler(48000, dev)
    tr = SlotTranscriber(m, _decoder(), S, 200, audio=composed(dev, 48000, S, 20000))
    ref = SlotTranscriber(m, _decoder(), S, 200, audio=StreamingAudioFrontend(ConformerAudioFrontend(device=dev), S, 8000))
    Ls = [31000, 16001]
    rng = np.random.default_rng(8)
    audio = [(rng.standard_normal((L, 2)) * 6000).clip(-32768, 32767).astype(np.int16) for L in Ls]
    lows = []
    for a in audio:
        y, (k,) = rs(torch.from_numpy(a[None]).to(dev))
        lows.append(y[0, :k])
    steps = [dict(open=[0], counts=[20000, 0]), dict(open=[1], counts=[1, 16001], flush=[1]), dict(counts=[10999, 0]),
             dict(counts=[0, 0], flush=[0])]
    pos, low_pos, seen, n_logits = [0, 0], [0, 0], [0, 0], 0
    for st in steps:
        for s in st.get("open", []):
            tr.open(s), ref.open(s)
        counts, flush = st["counts"], st.get("flush", [])
        x = torch.zeros(S, max(counts), 2, dtype=torch.int16)
        low_counts = []
        for s, c in enumerate(counts):
            x[s, :c] = torch.from_numpy(audio[s][pos[s]:pos[s] + c])
            pos[s] += c
            seen[s] += c
            total = R.out_len(seen[s], rs.o, rs.n) if s in flush else rs.n * R.blocks_emitted(seen[s], rs.width, rs.o)
            low_counts.append(total - low_pos[s] if tr.audio.is_open[s] else 0)
        xl = torch.zeros(S, max(low_counts), device=dev)
        for s, c in enumerate(low_counts):
            xl[s, :c] = lows[s][low_pos[s]:low_pos[s] + c]
            low_pos[s] += c
        got, k = tr.step_audio(x.to(dev), counts, flush)
        want, k2 = ref.step_audio(xl, low_counts, flush)
        assert k == k2 and got.shape == want.shape
        if max(k):
            n_logits += 1
            assert torch.equal(got, want)
    assert n_logits >= 2 and pos == Ls and low_pos == [len(v) for v in lows]
    assert tr.audio.is_open == [False] * S == tr.audio.input.is_open
    assert [tr.close(s) for s in range(S)] == [ref.close(s) for s in range(S)]


def test_streaming_transcriber_at_44k_stereo(dev):
    """The lockstep transcriber takes the same front end: (B, N, 2) float32 at 44.1 kHz against the 16 kHz stream, exactly."""
    from conformer_amd.frontend import ConformerAudioFrontend
    from conformer_amd.stream_frontend import StreamingAudioFrontend
    from conformer_amd.transcribe import StreamingTranscriber
    m, _ = _model(32, 4, 91, dev)
    B, L = 2, 20000
    rs = resampler(44100, dev)
    tr = StreamingTranscriber(m, _decoder(), B, 200, audio=composed(dev, 44100, B, 12000))
    ref = StreamingTranscriber(m, _decoder(), B, 200, audio=StreamingAudioFrontend(ConformerAudioFrontend(device=dev), B, 6000))
    x = (0.3 * torch.randn(B, L, 2, generator=torch.Generator().manual_seed(12))).to(dev)
    low, (total, _) = rs(x)
    t0 = l0 = 0
    for i, c in enumerate([440, 12000, 0, 7560]):
        last = i == 3
        t0 += c
        l1 = total if last else rs.n * R.blocks_emitted(t0, rs.width, rs.o)
        got = tr.step_audio(x[:, t0 - c:t0], flush=last)
        want = ref.step_audio(low[:, l0:l1], flush=last)
        assert got.shape == want.shape and torch.equal(got, want)
        l0 = l1
    assert t0 == L and l0 == R.out_len(L, rs.o, rs.n) and tr.encoder.frames == ref.encoder.frames > 0
    assert tr.finish() == ref.finish()


def test_offline_call_with_sample_rates(dev):
    """ConformerAudioFrontend.__call__(sample_rates=): rows at another rate (or not float32 mono) are resampled first."""
    from conformer_amd.frontend import ConformerAudioFrontend
    fe = ConformerAudioFrontend(device=dev)
    rng = np.random.default_rng(9)
    a16 = torch.from_numpy(rng.standard_normal(3000).astype(np.float32) * 0.3)
    a48 = torch.from_numpy((rng.standard_normal((9001, 2)) * 6000).astype(np.int16))
    a8 = torch.from_numpy(rng.standard_normal(1600).astype(np.float32) * 0.3)
    b48 = torch.from_numpy((rng.standard_normal((4000, 2)) * 6000).astype(np.int16))
    mels, lengths = fe([a16, a48, a8, b48], sample_rates=[16000, 48000, 8000, 48000])
    y48, (k48,) = resampler(48000, dev)(a48[None].to(dev))
    z48, (j48,) = resampler(48000, dev)(b48[None].to(dev))
    y8, (k8,) = resampler(8000, dev)(a8[None].to(dev))
    assert (k48, j48, k8) == (3001, 1334, 3200)
    want, want_lengths = fe([a16, y48[0, :k48], y8[0, :k8], z48[0, :j48]])
    assert torch.equal(lengths, want_lengths) and lengths.tolist() == [19, 19, 21, 9] and torch.equal(mels, want)
    plain, _ = fe([a16, a8])
    same, _ = fe([a16, a8], sample_rates=[16000, 16000])
    assert torch.equal(plain, same)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_state_alone(dev):
    from conformer_amd.resample import Resampler
    with pytest.raises(NotImplementedError):
        Resampler(16001, 16000, device=dev)                              # 16001 phases in, K far past 1024
    with pytest.raises(NotImplementedError):
        Resampler(16000, 16001, device=dev)                              # 16001 phases out
    with pytest.raises(NotImplementedError):
        resampler(48000, dev)(torch.zeros(1, 10, 9, device=dev))         # 9 channels
    x, ref = e2e_reference(48000, 15001, 40)
    chunks = [300, 1, 6000, 8700]

    def run(refuse):
        fe = composed(dev, 48000, 2, 9000)
        fe.open(0)
        out, t0 = [], 0
        for i, c in enumerate(chunks):
            if refuse:
                z = torch.zeros(2, 9000, device=dev)
                rsm = fe.input
                state = (list(fe.is_open), list(fe.received), list(fe.emitted), fe.tails[0].data_ptr(), list(rsm.is_open),
                         list(rsm.received), rsm.tails[0].data_ptr())
                short = i < 2                                             # 300 samples at 48 kHz at most: 100 at 16 kHz, not past the padding
                for exc, args in [(RuntimeError, (z, [10, 5])), (RuntimeError, (z, [10, 0], [1])),
                                  (ValueError, (torch.zeros(2, 9001, device=dev), [9001, 0])), (ValueError, (z, [9001, 0])),
                                  (ValueError, (z, [10], [0])), (Exception, (z.double(), [10, 0])),
                                  (ValueError, (z, [0, 0], [0])) if short else (ValueError, (z, [-1, 0]))]:
                    with pytest.raises(exc):
                        fe.step(*args)
                    assert (fe.is_open, fe.received, fe.emitted, fe.tails[0].data_ptr(), rsm.is_open, rsm.received,
                            rsm.tails[0].data_ptr()) == state
            xs = torch.zeros(2, c)
            xs[0] = torch.from_numpy(x[t0:t0 + c])
            mel, frames = fe.step(xs.to(dev), [c, 0], [0] if i == len(chunks) - 1 else [])
            out.append(mel[0, :, :frames[0]])
            t0 += c
        return torch.cat(out, dim=1).cpu()

    plain, refused = run(False), run(True)
    assert plain.shape == refused.shape == ref.shape
    assert rel_l2(refused, plain) <= 1e-6                  # the same launches on the same data
    e2e_check(refused.numpy(), ref, "after refusals")
