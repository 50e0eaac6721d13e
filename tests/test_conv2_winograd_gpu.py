"""The stem's conv2 as polyphase Winograd F(2x2,2x2) (cfm_subsample_conv2_wino_relu_f32) against a float64 conv2d, against
the direct implicit GEMM (cfm_subsample_conv2_relu_f32) and inside the encoder.  Not bitwise equal to the direct kernel:
the input subtractions, the tap sums of the weight transform and the plane adds round differently."""
import pytest
import torch

from tests import conv2_winograd_restatement as W

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from conformer_amd import _lib, ops
    lib = _lib.load()
    assert lib.cfm_device_check() == 0, "not a gfx950 device"
    return lib, ops


def data(B, T1, F1, C, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    h1 = torch.randn(B, T1, F1, C, device="cuda", generator=g).relu_()
    w2 = torch.randn(C, C, 3, 3, device="cuda", generator=g) / (9 * C) ** 0.5
    b2 = torch.randn(C, device="cuda", generator=g) * 0.1
    return h1, w2, b2


def wino(lib, ops, h1, w2, b2, wp=None):
    B, T1, F1, C = h1.shape
    T2, F2 = (T1 - 1) // 2, (F1 - 1) // 2
    wp = ops.pack_conv2_wino_weight(w2) if wp is None else wp
    planes = torch.empty(int(lib.cfm_conv2_wino_plane_elems(B, F1, T1, C)), device="cuda")
    h2 = torch.full((B, T2, F2, C), float("nan"), device="cuda")
    st = lib.cfm_subsample_conv2_wino_relu_f32(h1.data_ptr(), wp.data_ptr(), b2.data_ptr(), planes.data_ptr(), h2.data_ptr(),
                                               B, F1, T1, C, torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    return h2


def direct(lib, ops, h1, w2, b2):
    B, T1, F1, C = h1.shape
    T2, F2 = (T1 - 1) // 2, (F1 - 1) // 2
    w2p = ops.pack_conv2_weight(w2)
    h2 = torch.full((B, T2, F2, C), float("nan"), device="cuda")
    st = lib.cfm_subsample_conv2_relu_f32(h1.data_ptr(), w2p.data_ptr(), b2.data_ptr(), h2.data_ptr(), B, F1, T1, C,
                                          torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    return h2


def ref64(h1, w2, b2, pre=False):
    x = h1.double().cpu().permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(x, w2.double().cpu().transpose(2, 3), b2.double().cpu(), stride=2).permute(0, 2, 3, 1)
    return y if pre else y.relu()


def rel(a, b):
    return float((a.double().cpu() - b).norm() / b.norm())


def test_pack_matches_restatement(env):
    lib, ops = env
    _, w2, _ = data(1, 3, 3, 256, seed=1)
    got = ops.pack_conv2_wino_weight(w2).cpu()
    want = W.pack(w2.double().cpu()).float()
    assert torch.equal(got, want)


@pytest.mark.parametrize("B,T1,F1,C", [
    (2, 499, 39, 512),      # bench geometry (T2 = 249 odd, F2 = 19 odd)
    (3, 21, 13, 256),       # T2 = 10 even, F2 = 6 even
    (2, 19, 15, 256),       # T2 = 9 odd, F2 = 7 odd
    (1, 17, 11, 512),       # B = 1, T2 = 8 even, F2 = 5 odd
    (2, 3, 9, 256),         # T1 = 3
    (3, 5, 7, 256),         # T1 = 5
])
def test_vs_float64(env, B, T1, F1, C):
    lib, ops = env
    h1, w2, b2 = data(B, T1, F1, C, seed=B + T1 + F1)
    y = wino(lib, ops, h1, w2, b2)
    assert not torch.isnan(y).any()
    ref = ref64(h1, w2, b2)
    e_w = rel(y, ref)
    e_d = rel(direct(lib, ops, h1, w2, b2), ref)
    assert e_w <= 1e-6, e_w
    assert e_w <= 3 * e_d, (e_w, e_d)
    # the ReLU flips only where the pre-activation is within a few ulps of zero
    pre = ref64(h1, w2, b2, pre=True)
    flip = (y.cpu() > 0) != (pre > 0)
    if flip.any():
        assert float(pre[flip].abs().max()) < 1e-5


def test_bench_shape_slice_of_full_batch(env):
    """B = 32 at the bench geometry: utterances 0, 17 and 31 against float64; a B = 3 sub-batch bitwise; two runs bitwise."""
    lib, ops = env
    h1, w2, b2 = data(32, 499, 39, 512, seed=7)
    wp = ops.pack_conv2_wino_weight(w2)
    y = wino(lib, ops, h1, w2, b2, wp)
    assert not torch.isnan(y).any()
    assert torch.equal(y, wino(lib, ops, h1, w2, b2, wp))
    idx = [0, 17, 31]
    ref = ref64(h1[idx], w2, b2)
    e_w = rel(y[idx], ref)
    e_d = rel(direct(lib, ops, h1[idx].contiguous(), w2, b2), ref)
    assert e_w <= 1e-6 and e_w <= 3 * e_d, (e_w, e_d)
    sub = wino(lib, ops, h1[[31, 0, 17]].contiguous(), w2, b2, wp)
    assert torch.equal(sub, y[[31, 0, 17]])


def test_writes_only_valid_outputs(env):
    lib, ops = env
    B, T1, F1, C = 2, 19, 15, 256
    h1, w2, b2 = data(B, T1, F1, C, seed=3)
    T2, F2 = (T1 - 1) // 2, (F1 - 1) // 2
    wp = ops.pack_conv2_wino_weight(w2)
    planes = torch.empty(int(lib.cfm_conv2_wino_plane_elems(B, F1, T1, C)), device="cuda")
    buf = torch.full((B * T2 * F2 * C + 4096,), float("nan"), device="cuda")
    st = lib.cfm_subsample_conv2_wino_relu_f32(h1.data_ptr(), wp.data_ptr(), b2.data_ptr(), planes.data_ptr(), buf.data_ptr(),
                                               B, F1, T1, C, torch.cuda.current_stream().cuda_stream)
    assert st == 0
    torch.cuda.synchronize()
    assert not torch.isnan(buf[:B * T2 * F2 * C]).any()
    assert torch.isnan(buf[B * T2 * F2 * C:]).all()


def test_encoder_path_on_vs_off(env):
    lib, ops = env
    from oracle import conformer_oracle as O
    from model.modules.encoder import Encoder
    meta = dict(vocab=8, n_mel=80, n_blocks=2, d=512, n_heads=8, ksize=31, lstm_hidden=8, seed=9)
    P = O.make_params(**meta, with_decoder=False)
    enc = Encoder(80, 2, 512, 8, 31, 0.0)
    enc.load_state_dict({k[len("encoder."):]: v for k, v in P.items()}, strict=True)
    enc = enc.to("cuda").eval()
    g = torch.Generator().manual_seed(4)
    x = torch.randn(3, 80, 1000, generator=g).cuda()
    L = torch.tensor([1000, 777, 500]).cuda()
    assert ops.conv2_winograd_ok(512)
    prev = ops.set_conv2_winograd(False)
    try:
        with torch.no_grad():
            y_off, _ = enc(x, L)
        ops.set_conv2_winograd(True)
        with torch.no_grad():
            y_on, _ = enc(x, L)
    finally:
        ops.set_conv2_winograd(prev)
    assert not torch.equal(y_on, y_off)          # the path was taken
    assert float((y_on - y_off).norm() / y_off.norm()) < 1e-4
