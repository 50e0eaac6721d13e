"""CPU-side checks of cfm_convmod_glu_dwconv_f32 and of the predicate that routes ConvolutionModule to it: the entry point
refuses bad arguments with the documented status BEFORE any HIP call (so this runs without a GPU), and ops.convmod_fused_ok
follows its two rules (workgroups fill rounds of 256 CUs to >= 90 %; enough of a tile's 256 rows are frames of the utterance)."""
import ctypes
import os

import pytest

OK, BAD_SHAPE, UNSUPPORTED, NULL, ALIGN = 0, -1, -2, -3, -6


@pytest.fixture(scope="module")
def lib():
    from conformer_amd import _lib, build
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


def _args():
    buf = (ctypes.c_float * 4096)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16                # a 16-byte aligned address inside the buffer
    #        x  ldx  stats parts eps  Wf bias_f colsum dw_w dw_b bn_w bn_b mean var  eps   y  ldy   B  T    C    K   stream
    return buf, [a, 512, a, 16, 1e-5, a, a, a, a, a, a, a, a, a, 1e-5, a, 512, 32, 249, 512, 31, None]


def test_entry_point_validates_its_arguments_without_gpu(lib):
    buf, args = _args()
    f = lib.cfm_convmod_glu_dwconv_f32
    for i in (0, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15):                                     # every pointer
        bad = list(args); bad[i] = None
        assert f(*bad) == NULL, i
    for i, v in ((17, 0), (18, 0), (19, 0), (1, 256), (16, 256)):                           # B, T, C <= 0; ldx, ldy < C
        bad = list(args); bad[i] = v
        assert f(*bad) == BAD_SHAPE, (i, v)
    for c in (96, 160, 500):                                                                # C % 64 != 0
        bad = list(args); bad[19] = c; bad[1] = bad[16] = 512; bad[3] = 1
        assert f(*bad) == UNSUPPORTED, c
    for c in (192, 1024):                                                                   # C % 64 == 0, but not a width the fold carries
        bad = list(args); bad[19] = c; bad[1] = bad[16] = 1024; bad[3] = 1
        assert f(*bad) == UNSUPPORTED, c
    for k in (1, 5, 9, 33, 63, 30):                                                         # the depthwise kernel's instantiations only
        bad = list(args); bad[20] = k
        assert f(*bad) == UNSUPPORTED, k
    bad = list(args); bad[3] = 3
    assert f(*bad) < OK                                                                     # ln_parts does not divide C
    bad = list(args); bad[3] = 32
    assert f(*bad) == UNSUPPORTED                                                           # ln_parts > 16
    for i in (0, 2, 5, 6, 7):                                                               # x, ln_stats, Wf, bias_f, colsum: 16 bytes
        bad = list(args); bad[i] = args[i] + 4
        assert f(*bad) == ALIGN, i
    bad = list(args); bad[1] = 514
    assert f(*bad) == ALIGN                                                                 # ldx % 4
    assert lib.cfm_debug_convmod_variant(0) == 0                                            # the diagnostics switch: off by default
    del buf


def test_convmod_fused_ok_truth_table():
    from conformer_amd import ops
    assert ops.convmod_chunks(1, 31) == 1 and ops.convmod_chunks(256, 31) == 1 and ops.convmod_chunks(257, 31) == 2
    assert ops.convmod_chunks(482, 31) == 2 and ops.convmod_chunks(483, 31) == 3            # 256 + 226 frames in two tiles
    assert ops.convmod_chunks(483, 3) == 2 and ops.convmod_chunks(300, 15) == 2
    prev = ops.set_convmod_fused(True)
    try:
        assert ops.convmod_fused_ok(32, 249, 512, 31)              # the headline: 256 workgroups, 0.97 of the rows are frames
        assert ops.convmod_fused_ok(64, 249, 512, 31)              # two full rounds
        assert ops.convmod_fused_ok(32, 224, 512, 31) and ops.convmod_fused_ok(32, 256, 512, 31)    # row efficiency 0.875, 1.0
        assert ops.convmod_fused_ok(32, 467, 512, 31)              # two chunks, 0.91 of their rows are frames
        assert not ops.convmod_fused_ok(32, 192, 512, 31)          # row efficiency 0.75: measured slower than the two kernels
        assert not ops.convmod_fused_ok(32, 300, 512, 31)          # two chunks for 300 frames: 0.59
        assert not ops.convmod_fused_ok(32, 499, 512, 31)          # three chunks: 0.65
        assert not ops.convmod_fused_ok(16, 249, 512, 31)          # fill: 128 workgroups on 256 CUs
        assert not ops.convmod_fused_ok(36, 249, 512, 31)          # fill: 288 workgroups = 0.56 of two rounds
        assert not ops.convmod_fused_ok(32, 249, 512, 5)           # no such instantiation
        assert not ops.convmod_fused_ok(32, 249, 96, 31)           # C % 64, and not a fold width
        assert not ops.convmod_fused_ok(32, 249, 1024, 31)         # not a fold width
        assert not ops.convmod_fused_ok(0, 249, 512, 31) and not ops.convmod_fused_ok(32, 0, 512, 31)
        ops.set_convmod_fused(False)
        assert not ops.convmod_fused_ok(32, 249, 512, 31)          # the switch
    finally:
        ops.set_convmod_fused(prev)
