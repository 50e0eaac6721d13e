"""End-to-end GPU parity of the nn.Module surface (conformer_amd.model) against (a) golden vectors produced
by the reference itself and (b) the CPU oracle on the same seeded inputs at larger sizes.

fp32 tolerance from the north_star: 1e-3 rel per tensor; asserted here at 1e-4 for whole encoders and 2e-5
per block.  CTC alignment (per-frame argmax) indices must be bit-exact.
"""
import pytest
import torch

from oracle import conformer_oracle as O
from tests.util import cfg_params, load_golden, rel_l2

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def build_model(meta, P, dev):
    from model.conformer import Conformer          # the reference's import path, served by this repo
    m = Conformer(meta["vocab"], meta["n_mel"], meta["n_blocks"], meta["d"], meta["n_heads"], meta["ksize"],
                  meta["lstm_hidden"], 1, 0.0)
    m.load_state_dict(P, strict=True)
    return m.to(dev).eval()


@pytest.mark.parametrize("case", ["modules_d32_t7", "modules_d32_t48", "modules_d32_t1", "modules_d144_t49",
                                  "modules_d64_t70"])
def test_modules_vs_reference_golden(dev, case):
    from model.utils.attention import MultiHeadSelfAttentionModule
    from model.utils.block import ConformerBlock
    from model.utils.convolution import ConvolutionModule
    from model.utils.ffn import FeedForwardModule
    from model.utils.masking import generate_padding_mask
    from model.utils.position import RelativePositionalEncoding
    meta, g = load_golden(case)
    P = cfg_params(meta)
    d, H, K = meta["d"], meta["n_heads"], meta["ksize"]
    blk = "encoder.layers.0."

    def sub(prefix):
        return {k[len(prefix):]: v for k, v in P.items() if k.startswith(prefix)}

    x = g["x"].to(dev)
    L = g["lengths"].to(dev)
    with torch.no_grad():
        rel = RelativePositionalEncoding(d).to(dev)
        rel.load_state_dict({"div_term": P["encoder.rel_pe.div_term"]})
        pe = rel(x)                                                  # reference-style (B,2T-1,d)
        assert pe.shape == (x.shape[0], 2 * meta["T"] - 1, d)
        assert float((pe[0].cpu() - g["pe"]).abs().max()) < 4e-6
        mask = (~generate_padding_mask(L))[:, None, None, :]        # reference-style call sequence (encoder.py:30)
        ffn = FeedForwardModule(d).to(dev).eval(); ffn.load_state_dict(sub(blk + "ffn_1."))
        assert rel_l2(ffn(x), g["ffn_y"]) < 2e-5
        att = MultiHeadSelfAttentionModule(d, H).to(dev).eval(); att.load_state_dict(sub(blk + "attention."))
        assert rel_l2(att(x, pe, mask), g["mhsa_y"]) < 2e-5
        assert rel_l2(att(x, pe, None), g["mhsa_nomask_y"]) < 2e-5
        conv = ConvolutionModule(d, K).to(dev).eval(); conv.load_state_dict(sub(blk + "conv."))
        assert rel_l2(conv(x), g["conv_eval_y"]) < 2e-5
        block = ConformerBlock(d, H, K).to(dev).eval(); block.load_state_dict(sub(blk))
        assert rel_l2(block(x, pe, mask), g["block_y"]) < 2e-5


@pytest.mark.parametrize("case", ["stem_d32", "stem_d144"])
def test_stem_vs_reference_golden(dev, case):
    from model.utils.convolution import ConvolutionSubsampling
    meta, g = load_golden(case)
    P = cfg_params(meta)
    pre = "encoder.downsampling_conv."
    m = ConvolutionSubsampling(meta["d"]).to(dev).eval()
    m.load_state_dict({k[len(pre):]: v for k, v in P.items() if k.startswith(pre)})
    with torch.no_grad():
        y, L2 = m(g["x"].to(dev), g["lengths"].to(dev))
    assert rel_l2(y, g["y"]) < 2e-5
    assert torch.equal(L2.cpu(), g["out_lengths"])


@pytest.mark.parametrize("case", ["model_tiny", "model_cfg1_S"])
def test_full_model_vs_reference_golden(dev, case):
    meta, g = load_golden(case)
    P = cfg_params(meta)
    m = build_model(meta, P, dev)
    x, L = g["x"].to(dev), g["lengths"].to(dev)
    with torch.no_grad():
        enc, L2 = m.encoder(x, L)
        logits, L3 = m(x, L)
        enc_nm, _ = m.encoder(x, None)
    assert torch.equal(L2.cpu(), g["out_lengths"]) and torch.equal(L3.cpu(), g["out_lengths"])
    assert rel_l2(enc, g["enc"]) < 1e-4
    assert rel_l2(enc_nm, g["enc_nomask"]) < 1e-4
    assert rel_l2(logits, g["logits"]) < 1e-4
    am = logits.argmax(-1).cpu()
    if not torch.equal(am, g["argmax"]):                              # report the oracle's top-2 gap
        bad = (am != g["argmax"]).nonzero()
        top2 = g["logits"].topk(2, -1).values
        gaps = [float(top2[tuple(i)][0] - top2[tuple(i)][1]) for i in bad]
        pytest.fail(f"argmax mismatch at {bad.tolist()} with reference top-2 gaps {gaps}")
    loss = O.ctc_loss(logits.cpu(), g["targets"], L3.cpu(), g["target_lengths"])
    assert abs(float(loss) - float(g["ctc"])) < 1e-4 * abs(float(g["ctc"]))


def test_encoder_L_block_vs_oracle(dev):
    """One full-width Conformer-L block (d=512,H=8,K=31) at B=4,T'=249 with ragged lengths vs the fp64 oracle."""
    P = O.make_params(vocab=8, n_mel=80, n_blocks=1, d=512, n_heads=8, ksize=31, lstm_hidden=8, seed=5, with_decoder=False)
    from model.utils.block import ConformerBlock
    from model.utils.position import RelativePositionalEncoding
    blk = "encoder.layers.0."
    m = ConformerBlock(512, 8, 31).to(dev).eval()
    m.load_state_dict({k[len(blk):]: v for k, v in P.items() if k.startswith(blk)})
    g = torch.Generator().manual_seed(3)
    x = torch.randn(4, 249, 512, generator=g)
    L = torch.tensor([249, 200, 131, 17])
    rel = RelativePositionalEncoding(512).to(dev)
    with torch.no_grad():
        y = m.fused(x.to(dev), rel.table(249), L.to(dev))
    Pd = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    ref = O.conformer_block(x.double(), O.relpos_table(249, Pd["encoder.rel_pe.div_term"]), L, Pd, blk, 8)
    assert rel_l2(y, ref) < 2e-5


def test_encoder_cfg2_shapes_vs_oracle(dev):
    """BASELINE cfg-2 geometry (d=512, H=8, T=1000 -> T'=249) at reduced depth/batch so the CPU oracle
    finishes in seconds: 2 blocks, B=2, ragged lengths (sorted descending, max = T)."""
    meta = dict(vocab=8, n_mel=80, n_blocks=2, d=512, n_heads=8, ksize=31, lstm_hidden=8, seed=9)
    P = O.make_params(**meta, with_decoder=False)
    from model.modules.encoder import Encoder
    enc = Encoder(80, 2, 512, 8, 31, 0.0)
    enc.load_state_dict({k[len("encoder."):]: v for k, v in P.items()}, strict=True)
    enc = enc.to(dev).eval()
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 80, 1000, generator=g)
    L = torch.tensor([1000, 777])
    with torch.no_grad():
        y, L2 = enc(x.to(dev), L.to(dev))
        ref, R2 = O.encoder_forward(x, L, P, 2, 8)
    assert y.shape == (2, 249, 512) and torch.equal(L2.cpu(), R2)
    assert rel_l2(y, ref) < 1e-4


def test_encoder_cfg2_full_depth_vs_oracle(dev):
    """BASELINE cfg-2 model (16 blocks, d=512, H=8, T=1000) at B=2 vs the float64 oracle: the full-depth error budget."""
    meta = dict(vocab=8, n_mel=80, n_blocks=16, d=512, n_heads=8, ksize=31, lstm_hidden=8, seed=21)
    P = O.make_params(**meta, with_decoder=False)
    from model.modules.encoder import Encoder
    enc = Encoder(80, 16, 512, 8, 31, 0.0)
    enc.load_state_dict({k[len("encoder."):]: v for k, v in P.items()}, strict=True)
    enc = enc.to(dev).eval()
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 80, 1000, generator=g)
    L = torch.tensor([1000, 613])
    Pd = {k: (v.double() if v.is_floating_point() else v) for k, v in P.items()}
    with torch.no_grad():
        y, L2 = enc(x.to(dev), L.to(dev))
        ref, R2 = O.encoder_forward(x.double(), L, Pd, 16, 8)
    assert torch.equal(L2.cpu(), R2)
    assert rel_l2(y, ref) < 1e-4          # north_star: 1e-3 rel fp32


def test_encoder_cfg2_full_size_properties(dev):
    """The bench workload itself (B=32, T=1000, 16 blocks), too large for the CPU oracle: size-independent properties.
    Eval mode has no cross-utterance term (BatchNorm uses running statistics), so the encoder must be (a) deterministic,
    (b) equivariant under a permutation of the utterances and (c) consistent with running any sub-batch on its own;
    together with the B=2 full-depth oracle check above this pins the full-size result."""
    from model.modules.encoder import Encoder
    torch.manual_seed(0)
    enc = Encoder(80, 16, 512, 8, 31, 0.0).to(dev).eval()
    g = torch.Generator().manual_seed(8)
    x = torch.randn(32, 80, 1000, generator=g).to(dev)
    L = torch.full((32,), 1000, dtype=torch.int64)
    L[5], L[17], L[31] = 911, 640, 37
    L = L.to(dev)
    with torch.no_grad():
        y, L2 = enc(x, L)
        y_again, _ = enc(x, L)
        assert torch.equal(y, y_again)
        perm = torch.randperm(32, generator=g).to(dev)
        yp, Lp = enc(x[perm].contiguous(), L[perm].contiguous())
        assert torch.equal(Lp, L2[perm])
        assert rel_l2(yp, y[perm]) < 1e-6
        sub = torch.tensor([0, 5, 17], device=dev)          # keeps one full-length utterance: lengths.max() == T'
        ys, _ = enc(x[sub].contiguous(), L[sub].contiguous())
        assert rel_l2(ys, y[sub]) < 1e-6
    assert torch.isfinite(y).all() and y.shape == (32, 249, 512)
    # (d) utterances are independent: changing one leaves every other output bit-identical
    x2 = x.clone()
    x2[31, :, 200:] = 0.0
    with torch.no_grad():
        y2, _ = enc(x2, L)
    assert torch.equal(y2[:31], y[:31])


def test_encoder_long_utterance_vs_oracle(dev):
    """BASELINE cfg-5 input size (T = 20000 mel frames -> T' = 4999) as ONE non-streaming forward (the reference has no
    chunked/streaming code): a 1-block d=144 encoder, B=2 ragged, against the oracle -- the maximum-size edge of the
    stem, the relative-position table (9997 rows) and the attention ring."""
    meta = dict(vocab=8, n_mel=80, n_blocks=1, d=144, n_heads=4, ksize=31, lstm_hidden=8, seed=12)
    P = O.make_params(**meta, with_decoder=False)
    from model.modules.encoder import Encoder
    enc = Encoder(80, 1, 144, 4, 31, 0.0)
    enc.load_state_dict({k[len("encoder."):]: v for k, v in P.items()}, strict=True)
    enc = enc.to(dev).eval()
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 80, 20000, generator=g)
    L = torch.tensor([20000, 12345])
    with torch.no_grad(), torch.inference_mode():
        y, L2 = enc(x.to(dev), L.to(dev))
    with torch.no_grad():
        ref, R2 = O.encoder_forward(x, L, P, 1, 4)
    assert y.shape == (2, 4999, 144) and torch.equal(L2.cpu(), R2)
    assert rel_l2(y, ref) < 1e-4


def test_unbuilt_training_features_are_refused_loudly(dev):
    """No silent fallback: what has no kernels yet raises (train-mode dropout under no_grad; gradient w.r.t. the input)."""
    from model.modules.encoder import Encoder
    from model.utils.ffn import FeedForwardModule
    with pytest.raises(NotImplementedError), torch.no_grad():
        FeedForwardModule(32, dropout_rate=0.1).to(dev).train()(torch.zeros(2, 4, 32, device=dev))
    enc = Encoder(80, 1, 32, 4, 7).to(dev).eval()
    with pytest.raises(NotImplementedError):
        enc(torch.zeros(1, 80, 40, device=dev, requires_grad=True), None)


def test_graphed_encoder_matches_eager(dev):
    """hipGraph replay of the forward == eager launches, also after the input and the lengths change."""
    from conformer_amd.graph import GraphedEncoder
    from model.modules.encoder import Encoder
    meta, g = load_golden("model_tiny")
    P = cfg_params(meta)
    enc = Encoder(80, meta["n_blocks"], meta["d"], meta["n_heads"], meta["ksize"], 0.0)
    enc.load_state_dict({k[len("encoder."):]: v for k, v in P.items() if k.startswith("encoder.")}, strict=True)
    enc = enc.to(dev).eval()
    x, L = g["x"].to(dev), g["lengths"].to(dev)
    ge = GraphedEncoder(enc, x, L)
    y, L2 = ge(x, L)
    assert rel_l2(y, g["enc"]) < 1e-4 and torch.equal(L2.cpu(), g["out_lengths"])
    x2 = torch.flip(x, dims=[0]).contiguous()
    L3 = torch.tensor([103, 103, 60], device=dev)
    with torch.no_grad():
        ref, _ = enc(x2, L3)
    y2, _ = ge(x2, L3)
    assert torch.equal(y2, ref)


def test_graphed_encoder_recaptures_after_a_weight_update(dev):
    """The captured graph holds addresses of derived weight packs: after an in-place weight update (optimizer step,
    load_state_dict) a replay would compute with stale packs -- the wrapper must notice and capture again."""
    from conformer_amd.graph import GraphedEncoder
    from model.modules.encoder import Encoder
    meta, g = load_golden("model_tiny")
    P = cfg_params(meta)
    enc = Encoder(80, meta["n_blocks"], meta["d"], meta["n_heads"], meta["ksize"], 0.0)
    enc.load_state_dict({k[len("encoder."):]: v for k, v in P.items() if k.startswith("encoder.")}, strict=True)
    enc = enc.to(dev).eval()
    x, L = g["x"].to(dev), g["lengths"].to(dev)
    ge = GraphedEncoder(enc, x, L)
    y0 = ge(x, L)[0].clone()
    assert ge.captures == 1
    ge(x, L)
    assert ge.captures == 1                                   # unchanged weights: plain replay
    with torch.no_grad():
        enc.layers[0].attention.attention.query_proj.weight.mul_(1.5)      # goes through the fused-QKV pack
        enc.linear.weight.add_(0.01)                                       # goes through the packed input-linear weight
        ref, _ = enc(x, L)
    y1, _ = ge(x, L)
    assert ge.captures == 2
    assert torch.equal(y1, ref) and not torch.equal(y1, y0)


def test_inference_mode_with_cached_projected_positions(dev):
    """infer.py / test.py of the reference run under torch.inference_mode(): the cached packs and position tables are
    then inference tensors (no version counter) -- the pack cache must accept them as keys (round-1 advisor finding)."""
    from model.modules.encoder import Encoder
    meta, g = load_golden("model_tiny")
    P = cfg_params(meta)
    enc = Encoder(80, meta["n_blocks"], meta["d"], meta["n_heads"], meta["ksize"], 0.0)
    enc.load_state_dict({k[len("encoder."):]: v for k, v in P.items() if k.startswith("encoder.")}, strict=True)
    enc = enc.to(dev).eval()
    enc.cache_projected_positions = True
    x, L = g["x"].to(dev), g["lengths"].to(dev)
    with torch.inference_mode():
        y1, _ = enc(x, L)
        y2, _ = enc(x, L)
    assert rel_l2(y1, g["enc"]) < 1e-4 and torch.equal(y1, y2)
    with torch.no_grad():                                     # and the same module afterwards outside inference mode
        y3, _ = enc(x, L)
    assert torch.equal(y3, y1)


def test_position_table_of_an_inference_mode_module(dev):
    """A model BUILT under torch.inference_mode() holds inference tensors as parameters: `div_term._version` raises on them,
    so the table's cache key must not read it."""
    from conformer_amd import ops
    from model.utils.position import RelativePositionalEncoding
    with torch.inference_mode():
        rel = RelativePositionalEncoding(16).to(dev)
        assert rel.div_term.is_inference()
        t9 = rel.table(9)
        assert t9.shape == (17, 16) and torch.equal(t9, ops.relpos_table(rel.div_term, 9))
        assert rel.table(9) is t9
        t5 = rel.table(5)
        assert t5.shape == (9, 16) and torch.equal(t5, ops.relpos_table(rel.div_term, 5))
