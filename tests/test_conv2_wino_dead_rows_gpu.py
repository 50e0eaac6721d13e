"""The Winograd conv2 with the dead rows of its pattern-2 problems left out (csrc/conv2_wino_f32.hip, "Dead rows"): all four
parities of (T2, F2) at C = 256 against a float64 conv2d, with the bound of test_conv2_winograd_gpu.py (rel-L2 <= 1e-6 and no
worse than 3x the direct kernel's on the same data), h2 and the planes scratch pre-filled with NaN, and guard bands round h2."""
import pytest
import torch

pytestmark = pytest.mark.gpu

C = 256
GUARD = 4096


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conformer_amd import _lib, ops
    lib = _lib.load()
    assert lib.cfm_device_check() == 0, "not a gfx950 device"
    return lib, ops


def tiles(B, T1, F1):
    """Row tiles (256 rows) of a full pattern, of a b = 2 pattern, of an a = 2 pattern and of (2, 2)."""
    T2, F2 = (T1 - 1) // 2, (F1 - 1) // 2
    TI, TJ = (T2 + 1) // 2, (F2 + 1) // 2
    TIs, TJs = TI - T2 % 2, TJ - F2 % 2
    return [(B * i * j + 255) // 256 for i, j in ((TI, TJ), (TI, TJs), (TIs, TJ), (TIs, TJs))]


CASES = [
    # B, T1, F1                 T2, F2
    (16, 19, 15),             # 9, 7    odd / odd: 2 row tiles, every shortened pattern 1
    (24, 17, 11),             # 8, 5    even / odd: 2 row tiles, the b = 2 patterns 1
    (24, 15, 13),             # 7, 6    odd / even: 2 row tiles, the a = 2 patterns 1
    (20, 21, 13),             # 10, 6   even / even: the unchanged path, 2 row tiles
    (3, 499, 39),             # 249, 19 bench geometry: 15 row tiles, 14 for the b = 2 patterns
    (5, 3, 9),                # 1, 4    T2 = 1: the a = 2 patterns have no rows at all
    (5, 4, 4),                # 1, 1    T2 = F2 = 1: only patterns (0, 0), (0, 1), (1, 0), (1, 1) have rows
    (3, 23, 3),               # 11, 1   F2 = 1
    (2, 4, 12),               # 1, 5
    (300, 5, 4),              # 2, 1    F2 = 1 with two row tiles
]


def test_cases_cover_what_they_claim():
    par = {(((T1 - 1) // 2) % 2, ((F1 - 1) // 2) % 2) for _, T1, F1 in CASES}
    assert par == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert tiles(16, 19, 15) == [2, 1, 1, 1] and tiles(24, 17, 11) == [2, 1, 2, 1] and tiles(24, 15, 13) == [2, 2, 1, 1]
    assert tiles(20, 21, 13) == [2, 2, 2, 2] and tiles(3, 499, 39) == [15, 14, 15, 14]
    assert tiles(5, 4, 4) == [1, 0, 0, 0] and tiles(5, 3, 9) == [1, 1, 0, 0] and tiles(300, 5, 4) == [2, 0, 2, 0]


@pytest.mark.parametrize("B,T1,F1", CASES)
def test_vs_float64_with_sentinels(env, B, T1, F1):
    lib, ops = env
    g = torch.Generator(device="cuda").manual_seed(1000 * B + 10 * T1 + F1)
    h1 = torch.randn(B, T1, F1, C, device="cuda", generator=g).relu_()
    w2 = torch.randn(C, C, 3, 3, device="cuda", generator=g) / (9 * C) ** 0.5
    b2 = torch.randn(C, device="cuda", generator=g) * 0.1
    T2, F2 = (T1 - 1) // 2, (F1 - 1) // 2
    n = B * T2 * F2 * C
    st = torch.cuda.current_stream().cuda_stream

    wp = ops.pack_conv2_wino_weight(w2)
    planes = torch.full((int(lib.cfm_conv2_wino_plane_elems(B, F1, T1, C)),), float("nan"), device="cuda")
    buf = torch.full((GUARD + n + GUARD,), float("nan"), device="cuda")
    h2 = buf[GUARD:GUARD + n]
    assert lib.cfm_subsample_conv2_wino_relu_f32(h1.data_ptr(), wp.data_ptr(), b2.data_ptr(), planes.data_ptr(), h2.data_ptr(),
                                                 B, F1, T1, C, st) == 0
    torch.cuda.synchronize()
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + n:]).all()
    assert not torch.isnan(h2).any()                      # every valid output written, from planes that were written
    y = h2.view(B, T2, F2, C).clone()
    # a second run over the (now partly written) scratch gives the same bits
    assert lib.cfm_subsample_conv2_wino_relu_f32(h1.data_ptr(), wp.data_ptr(), b2.data_ptr(), planes.data_ptr(), h2.data_ptr(),
                                                 B, F1, T1, C, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(h2.view(B, T2, F2, C), y)

    d = torch.full((B, T2, F2, C), float("nan"), device="cuda")
    w2p = ops.pack_conv2_weight(w2)
    assert lib.cfm_subsample_conv2_relu_f32(h1.data_ptr(), w2p.data_ptr(), b2.data_ptr(), d.data_ptr(), B, F1, T1, C, st) == 0
    torch.cuda.synchronize()

    x = h1.double().cpu().permute(0, 3, 1, 2)
    ref = torch.nn.functional.conv2d(x, w2.double().cpu().transpose(2, 3), b2.double().cpu(), stride=2).permute(0, 2, 3, 1).relu()
    e_w = float((y.double().cpu() - ref).norm() / ref.norm())
    e_d = float((d.double().cpu() - ref).norm() / ref.norm())
    print(f"B={B} T1={T1} F1={F1}: rel-L2 winograd {e_w:.3e} direct {e_d:.3e}")
    assert e_w <= 1e-6, e_w
    assert e_w <= 3 * e_d, (e_w, e_d)


def test_utterance_independent_of_neighbours(env):
    """Odd / odd with several row tiles: an utterance's h2 is the same bits alone and inside the batch."""
    lib, ops = env
    B, T1, F1 = 16, 19, 15
    g = torch.Generator(device="cuda").manual_seed(11)
    h1 = torch.randn(B, T1, F1, C, device="cuda", generator=g).relu_()
    w2 = torch.randn(C, C, 3, 3, device="cuda", generator=g) / (9 * C) ** 0.5
    b2 = torch.randn(C, device="cuda", generator=g) * 0.1
    wp = ops.pack_conv2_wino_weight(w2)
    T2, F2 = (T1 - 1) // 2, (F1 - 1) // 2

    def run(h):
        n = h.shape[0]
        planes = torch.full((int(lib.cfm_conv2_wino_plane_elems(n, F1, T1, C)),), float("nan"), device="cuda")
        out = torch.full((n, T2, F2, C), float("nan"), device="cuda")
        assert lib.cfm_subsample_conv2_wino_relu_f32(h.data_ptr(), wp.data_ptr(), b2.data_ptr(), planes.data_ptr(), out.data_ptr(),
                                                     n, F1, T1, C, torch.cuda.current_stream().cuda_stream) == 0
        torch.cuda.synchronize()
        return out

    y = run(h1)
    assert torch.equal(run(h1[[15, 0, 7]].contiguous()), y[[15, 0, 7]])
