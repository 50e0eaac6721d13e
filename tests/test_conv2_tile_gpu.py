"""The stem's second convolution (cfm_subsample_conv2_relu_f32) on the 8-wave 256x256 tile against the 4-wave 128x128 tile:
same MFMA, same k order, same epilogue arithmetic, so h2 must be BITWISE equal.  The tile is picked through the
cfm_debug_set_conv2_bk diagnostics switch (101: the 128x128 tile, 102: the 256x256 tile for every row wherever C % 256 == 0,
100: by shape -- at the bench shape the 256x256 tile on the leading utterances that fill whole rounds, the 128x128 tile on the rest).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

AUTO, OLD, WIDE = 100, 101, 102


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conformer_amd import _lib, ops
    lib = _lib.load()
    assert lib.cfm_device_check() == 0, "not a gfx950 device"
    yield lib, ops
    lib.cfm_debug_set_conv2_bk(AUTO)


def conv2(lib, ops, B, T1, F1, C, tile, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    h1 = torch.randn(B, T1, F1, C, device="cuda", generator=g).relu_()
    w2 = torch.randn(C, C, 3, 3, device="cuda", generator=g) / (9 * C) ** 0.5
    b2 = torch.randn(C, device="cuda", generator=g) * 0.1
    w2p = ops.pack_conv2_weight(w2)
    T2, F2 = (T1 - 1) // 2, (F1 - 1) // 2
    h2 = torch.full((B, T2, F2, C), float("nan"), device="cuda")
    lib.cfm_debug_set_conv2_bk(tile)
    try:
        st = lib.cfm_subsample_conv2_relu_f32(h1.data_ptr(), w2p.data_ptr(), b2.data_ptr(), h2.data_ptr(), B, F1, T1, C,
                                              torch.cuda.current_stream().cuda_stream)
    finally:
        lib.cfm_debug_set_conv2_bk(AUTO)
    assert st == 0
    torch.cuda.synchronize()
    return h2, h1, w2, b2


@pytest.mark.parametrize("B,T1,F1,C", [
    (32, 499, 39, 512),      # the bench shape: M = 151392 = 591 x 256 + 96 (ragged last row tile)
    (3, 61, 39, 512),        # M = 3 * 30 * 19 = 1710: ragged, a handful of tiles
    (1, 499, 39, 512),       # B = 1
    (4, 3, 39, 512),         # T1 = 3: one output frame
    (2, 5, 39, 512),         # T1 = 5
    (5, 101, 39, 256),       # C = 256: one column tile
])
def test_wide_tile_bitwise(env, B, T1, F1, C):
    lib, ops = env
    old, h1, w2, b2 = conv2(lib, ops, B, T1, F1, C, OLD)
    new, *_ = conv2(lib, ops, B, T1, F1, C, WIDE)
    assert torch.isfinite(old).all()
    assert torch.equal(old, new)
    if B * T1 <= 400:        # and both against the definition (fp32 tolerance)
        ref = torch.nn.functional.conv2d(h1.permute(0, 3, 2, 1).double(), w2.double(), b2.double(), stride=2).relu()
        ref = ref.permute(0, 3, 2, 1)
        assert float((new.double() - ref).norm() / ref.norm()) < 1e-5


@pytest.mark.parametrize("B,T1,F1,C,tile", [
    (32, 499, 39, 512, AUTO),   # eligible: the shape picks the 256x256 tile
    (2, 61, 39, 512, AUTO),     # too few tiles: stays on the 128x128 tile
    (4, 61, 39, 384, AUTO),     # C % 256 != 0
    (4, 61, 39, 384, WIDE),     # ... even when the wide tile is forced
    (3, 21, 39, 128, WIDE),
])
def test_dispatch_matches_old_tile(env, B, T1, F1, C, tile):
    lib, ops = env
    old, *_ = conv2(lib, ops, B, T1, F1, C, OLD)
    got, *_ = conv2(lib, ops, B, T1, F1, C, tile)
    assert torch.isfinite(old).all()
    assert torch.equal(old, got)
