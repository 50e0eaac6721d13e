"""The 16-bit slots attention entry (cfm_relpos_attention_slots_mfma16_f32), CPU side: it refuses every bad argument with the sibling
entries' status codes before any HIP call, on host pointers it never dereferences; and the `dtype=` keyword of the slot objects is
checked before anything touches a device."""
import ctypes
import os

import pytest

BF16, FP16 = 1, 2                                             # CFM_PREC_* of include/conformer_hip.h


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
    a = dict(prec=BF16, q=p, k=p, v=p, q16=0, ld=3 * 64, pos=p, ldp=64, u=p, vb=p, qb=p, qc=p, lengths=p, ctx=p, ldo=64, B=2, T=100,
             H=4, dh=16, q_max=8, nsplit=1, ws=None)
    a.update(kw)
    return lib.cfm_relpos_attention_slots_mfma16_f32(a["prec"], a["q"], a["k"], a["v"], a["q16"], a["ld"], a["pos"], a["ldp"], a["u"],
                                                     a["vb"], a["qb"], a["qc"], a["lengths"], a["ctx"], a["ldo"], a["B"], a["T"],
                                                     a["H"], a["dh"], a["q_max"], a["nsplit"], a["ws"], None)


@pytest.mark.parametrize("prec", [BF16, FP16])
@pytest.mark.parametrize("q16", [0, 1])
def test_slots16_entry_validates_without_gpu(lib, ptr, prec, q16):
    p = ptr
    kw = dict(prec=prec, q16=q16)
    for name in ("q", "k", "v", "pos", "u", "vb", "qb", "qc", "lengths", "ctx"):
        assert _call(lib, p, **kw, **{name: None}) == -3, name                   # NULL
    assert _call(lib, p, **kw, q_max=0) == -1                                    # q_max < 1
    assert _call(lib, p, **kw, q_max=101) == -1                                  # q_max > T
    assert _call(lib, p, **kw, nsplit=0) == -1                                   # nsplit out of range
    assert _call(lib, p, **kw, nsplit=17, ws=p) == -1
    assert _call(lib, p, **kw, nsplit=2, ws=None) == -1                          # key split without a workspace
    assert _call(lib, p, **kw, nsplit=2, ws=p, ldo=68) == -1                     # key split needs ldo == H*dh
    assert _call(lib, p, **kw, dh=18, ldo=72, ld=216) == -1                      # dh % 4
    assert _call(lib, p, **kw, dh=68, H=1, ldo=68, ld=208) == -2                 # dh > 64
    assert _call(lib, p, **kw, ldo=60) == -1                                     # ldo < H*dh
    assert _call(lib, p, **kw, B=0) == -1
    for name in ("q", "k", "v", "pos", "u", "vb", "ctx"):
        assert _call(lib, p, **kw, **{name: p + 4}) == -6, name                  # not 16-byte aligned
    assert _call(lib, p, **kw, nsplit=2, ws=p + 4) == -6


def test_slots16_entry_precision_and_cache_layout(lib, ptr):
    p = ptr
    assert _call(lib, p, prec=0) == -2 and _call(lib, p, prec=3) == -2           # not bf16 / fp16
    assert _call(lib, p, q16=1, ld=3 * 60, H=3, dh=20, ldo=60, ldp=60) == -1     # a 16-bit cache needs ld % 8 == 0
    assert _call(lib, p, q16=0, ld=3 * 60, H=3, dh=20, ldo=60, ldp=60, qb=None) == -3   # (the fp32 cache takes that ld: next refusal)


def test_slot_dtype_keyword_is_checked_on_the_host():
    import torch
    from conformer_amd.slots import _slot_dtype
    assert _slot_dtype("x", None) is None and _slot_dtype("x", torch.float32) is None
    assert _slot_dtype("x", torch.bfloat16) is torch.bfloat16 and _slot_dtype("x", torch.float16) is torch.float16
    for bad in (torch.float64, torch.int32):
        with pytest.raises(ValueError):
            _slot_dtype("x", bad)
