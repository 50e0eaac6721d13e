"""Bounded-history streaming (left_context), CPU side: the float64 windowed restatement against the reference goldens, the window
entry's argument checks on host pointers it never dereferences, the extension header's binding, the ring arithmetic of the host
path and the refusals that need no device."""
import ctypes
import os

import pytest
import torch

from oracle import conformer_oracle as O
from tests import window_restatement as W
from tests.util import cfg_params, load_golden, rel_l2

CASES = [("stream_window_mhsa_d64_t70_l24", "stream_mhsa_d64_t70"), ("stream_window_mhsa_d144_t49_l7", "stream_mhsa_d144_t49")]


@pytest.mark.parametrize("case,sibling", CASES)
def test_restatement_matches_reference_under_banded_mask(case, sibling):
    """The row-by-row float64 core (keys of the window only, table rows by i - j) against the reference's
    MultiHeadSelfAttentionModule under the (1,1,T',T') mask (j >= visible_end[i]) | (j < i - left), which ran in fp32."""
    meta, g = load_golden(case)
    P = cfg_params(meta, dtype=torch.float64)
    x = g["x"].double()
    T = x.shape[1]
    pe = O.relpos_table(T, P["encoder.rel_pe.div_term"])
    ve = W.visible_ends(g["chunk_ends"].tolist(), T)
    y = W.mhsa_module_windowed(x, pe, P, "encoder.layers.0.attention.", meta["n_heads"], ve, meta["left"])
    err = rel_l2(y, g["mhsa_y"])
    print(f"{case}: restatement vs reference rel-L2 {err:.3g}")
    assert err < 2e-6
    # and the band really changes the numbers: the sibling golden has the same weights and inputs under a block-triangular mask
    meta_s, gs = load_golden(sibling)
    assert torch.equal(gs["x"], g["x"])
    diff = rel_l2(g["mhsa_y"], gs["mhsa_y"])
    print(f"{case}: vs {sibling} rel-L2 {diff:.3g}")
    assert diff > 1e-3


def test_window_that_covers_everything_is_the_prefix_rule():
    """left >= T': encoder_forward_windowed is oracle.encoder_forward_chunked.  The windowed core sums each softmax row over its
    visible keys only, the oracle's over all T' keys with exact zeros at the hidden ones, so the two differ by float64 summation
    order alone: a few ulp per operation (2.2e-16) through two blocks, bounded here at 1e-12; an error of the rule itself (one
    key more or less) shows at 1e-3 and above."""
    P = O.make_params(vocab=8, n_mel=80, n_blocks=2, d=32, n_heads=4, ksize=7, lstm_hidden=8, seed=21, dtype=torch.float64,
                      with_decoder=False)
    x = torch.randn(2, 80, 131, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    ends = [3, 4, 17, 32]
    ref = O.encoder_forward_chunked(x, P, 2, 4, ends)
    for left in (32, 1000):
        assert rel_l2(W.encoder_forward_windowed(x, P, 2, 4, ends, left), ref) < 1e-12
    assert rel_l2(W.encoder_forward_windowed(x, P, 2, 4, ends, 5), ref) > 1e-3


# ---- the C entry ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from conformer_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


_BUF = (ctypes.c_float * 4096)()                              # host memory the refused calls never touch


@pytest.fixture(scope="module")
def ptr():
    return (ctypes.addressof(_BUF) + 15) // 16 * 16


def _call(lib, p, **kw):
    a = dict(q=p, k=p, v=p, ld=3 * 64, pos=p, ldp=64, P=40, u=p, vb=p, qb=p, qc=p, ctx=p, ldo=64, B=2, R=64, H=4, dh=16, q_max=8,
             left=24)
    a.update(kw)
    return lib.cfm_relpos_attention_window_f32(a["q"], a["k"], a["v"], a["ld"], a["pos"], a["ldp"], a["P"], a["u"], a["vb"], a["qb"],
                                               a["qc"], a["ctx"], a["ldo"], a["B"], a["R"], a["H"], a["dh"], a["q_max"], a["left"],
                                               None)


def test_window_entry_validates_without_gpu(lib, ptr):
    p = ptr
    for name in ("q", "k", "v", "pos", "u", "vb", "qb", "qc", "ctx"):
        assert _call(lib, p, **{name: None}) == -3, name                         # NULL
    assert _call(lib, p, R=48) == -1                                             # R % 32
    assert _call(lib, p, R=0) == -1
    assert _call(lib, p, R=32, left=24, q_max=9) == -1                           # R < left + q_max
    assert _call(lib, p, R=64, left=57, q_max=8, P=64) == -1
    assert _call(lib, p, left=24, P=24) == -1                                    # P < left + 1
    assert _call(lib, p, left=2, q_max=8, P=7) == -1                             # P < q_max
    assert _call(lib, p, left=-1) == -1
    assert _call(lib, p, q_max=0) == -1
    assert _call(lib, p, dh=18, ldo=72, ld=216) == -1                            # dh % 4
    assert _call(lib, p, dh=68, H=1, ldo=68, ld=204) == -2                       # dh > 64
    assert _call(lib, p, ldo=60) == -1                                           # ldo < H*dh
    assert _call(lib, p, ld=3 * 64 + 2) == -1 and _call(lib, p, ldp=66) == -1    # leading dimensions % 4
    assert _call(lib, p, B=0) == -1
    assert _call(lib, p, B=20000) == -2                                          # B*H past the grid limit
    for name in ("q", "k", "v", "pos", "u", "vb", "ctx"):
        assert _call(lib, p, **{name: p + 4}) == -6, name                        # not 16-byte aligned


def test_extension_header_is_bound_separately(lib):
    """what every header shares (record, names, binding, rebuild message, build) is asserted in test_abi_binding_cpu"""
    from conformer_amd import _lib
    header = _lib.HEADERS["conformer_hip_window.h"]
    assert "cfm_relpos_attention_window_f32" not in _lib.SIGNATURES and len(_lib.SIGNATURES) == 144
    res, args = header.signatures["cfm_relpos_attention_window_f32"]
    vp, i64, i32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    assert res is i32 and args == [vp, vp, vp, i64, vp, i64, i32, vp, vp, vp, vp, vp, i64, i32, i32, i32, i32, i32, i32, vp]
    assert _lib.ENTRIES["cfm_relpos_attention_window_f32"] == (res, args)
    assert _lib.PARAMS["cfm_relpos_attention_window_f32"] == header.params["cfm_relpos_attention_window_f32"] == [
        "q", "k", "v", "ld", "pos", "ldp", "P", "u", "vbias", "q_begin", "q_count", "ctx", "ldo", "B", "R", "H", "dh", "q_max",
        "left", "stream"]
    assert _lib.ABI_VERSION == 4 and lib.cfm_abi_version() == 4                  # nothing existing moved
    with pytest.raises(_lib.ConformerHipError, match="argument 7 .`P`."):        # `call` names the parameters of this header too
        _lib.call("cfm_relpos_attention_window_f32", None, None, None, 0, None, 0, "x", None, None, None, None, None, 0, 1, 32, 1,
                  4, 1, 0, None)


# ---- host arithmetic -----------------------------------------------------------------------------------------------------------
def test_ring_plan_and_rows():
    from conformer_amd.slots import append_rows
    from conformer_amd.streaming import encoder_frames, ring_plan, ring_rows
    assert ring_plan(24, 64) == (64, 25, 16)                  # k_cap = frames(70) = 16; R = 32 ceil(40/32); P = max(25, 16)
    assert ring_plan(20, 45) == (32, 21, 12)                  # k_cap = frames(51) = 12: 20 + 12 = 32, a full ring
    assert ring_plan(0, 640) == (160, 160, 160)               # no history: the step's own rows, P = k_cap
    assert ring_plan(256, 640) == (416, 257, 160)             # cfg-5: 16 layers x 8 x 416 x 1536 x 4 B = 0.33 GB
    assert 16 * 8 * 416 * 1536 * 4 == 327_155_712
    for L, mc in [(0, 1), (1, 1), (31, 7), (33, 200)]:
        R, P, k_cap = ring_plan(L, mc)
        assert R % 32 == 0 and L + k_cap <= R < L + k_cap + 32 and P >= max(L + 1, k_cap) and k_cap == encoder_frames(mc + 6) >= 1
    for bad in [(-1, 64), (4, 0)]:
        with pytest.raises(ValueError):
            ring_plan(*bad)
    assert ring_rows(0, 12, 32) == [(0, 0, 12)]
    assert ring_rows(20, 12, 32) == [(20, 0, 12)]             # ends exactly at the last row
    assert ring_rows(30, 12, 32) == [(30, 0, 2), (0, 2, 10)]  # wraps
    assert ring_rows(2 ** 40 + 31, 3, 32) == [(31, 0, 1), (0, 1, 2)]
    for n0, k, R in [(0, 1, 32), (95, 32, 32), (1000, 17, 64)]:
        rows = [d + r for d, s, n in ring_rows(n0, k, R) for r in range(n)]
        assert rows == [(n0 + r) % R for r in range(k)]
        assert [s + r for d, s, n in ring_rows(n0, k, R) for r in range(n)] == list(range(k))
    # slots: compact row -> ring row of its own slot
    src, dst = append_rows([30, 0, 2 ** 40 + 5], [3, 0, 2], k_max=3, t_max=None, ring=32)
    assert src == [0, 1, 2, 6, 7] and dst == [30, 31, 0, 64 + 5, 64 + 6]
    assert append_rows([30, 0], [2, 1], k_max=2, t_max=100) == ([0, 1, 2], [30, 31, 100])      # the linear cache, as before


def test_refusals_that_need_no_device():
    from conformer_amd.slots import SlotStreamingEncoder, SlotTranscriber
    from conformer_amd.streaming import StreamingEncoder
    with pytest.raises(NotImplementedError, match="graphs"):
        StreamingEncoder(None, 2, None, graphs=True, left_context=24, max_chunk_mel_frames=64)
    with pytest.raises(NotImplementedError, match="graphs"):
        StreamingEncoder(None, 2, 4000, graphs=True, left_context=0, max_chunk_mel_frames=1)
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(NotImplementedError, match="16-bit"):
            SlotStreamingEncoder(None, 2, 4000, dtype=dt, left_context=24, max_chunk_mel_frames=64)
        with pytest.raises(NotImplementedError, match="16-bit"):
            SlotTranscriber(None, None, 2, 4000, dtype=dt, left_context=24, max_chunk_mel_frames=64)
    with pytest.raises(ValueError, match="max_chunk_mel_frames"):
        StreamingEncoder(None, 2, 4000, left_context=24)                         # a ring needs the largest step
    with pytest.raises(ValueError, match="left_context"):
        StreamingEncoder(None, 2, 4000, max_chunk_mel_frames=64)
    with pytest.raises(ValueError, match="left_context"):
        StreamingEncoder(None, 2, None)                                          # no end only with bounded history
    with pytest.raises(ValueError):
        StreamingEncoder(None, 2, None, left_context=-1, max_chunk_mel_frames=64)
    with pytest.raises(ValueError):
        SlotStreamingEncoder(None, 2, None, left_context=8, max_chunk_mel_frames=0)
