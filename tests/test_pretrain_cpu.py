"""Self-supervised pretraining without a GPU: the float64 restatement against the reference's own Quantization (the golden of
tests/golden/make_golden_pretrain.py), the two samplers (device torch ops, so they run on the CPU too), the exported key set, the
header as the open table discovers it, and every refusal of conformer_hip3_pretrain.h through the built library (the argument
checks return before any HIP call, as in test_ctc_nbest_cpu.py)."""
import ctypes
import json
import math
import os
import re

import numpy as np
import pytest
import torch

from conformer_amd import _lib
from tests import pretrain_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "conformer_amd", "csrc")
HEADER = "conformer_hip3_pretrain.h"
ENTRIES = ("cfm3_quantize_workspace_floats", "cfm3_quantize_fwd_f32", "cfm3_quantize_bwd_f32",
           "cfm3_contrastive_workspace_floats", "cfm3_contrastive_fwd_f32", "cfm3_contrastive_bwd_f32")
GOLDEN = os.path.join(ROOT, "tests", "golden", "pretrain_quantizer.npz")


@pytest.fixture(scope="module")
def lib():
    from conformer_amd import build
    if not os.path.exists(_lib.LIB_PATH):
        build.build_library(verbose=False)
    return _lib.load()


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}, json.loads(str(z["meta"]))


def rel(got, ref):
    got, ref = torch.as_tensor(got).double(), torch.as_tensor(ref).double()
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30)


def golden_case(g, i):
    t = {k: torch.from_numpy(g[f"s{i}_{k}"]) for k in ("x", "mask", "gumbel", "weight", "bias", "codevectors")}
    t["logits"] = torch.nn.functional.linear(t["x"], t["weight"], t["bias"])      # fp32 on the CPU: the reference's own bits
    return t


@pytest.mark.parametrize("i", [0, 1])
def test_the_restatement_reproduces_the_reference(golden, i):
    g, meta = golden
    B, T, G, V, dg = meta["shapes"][i]
    c = golden_case(g, i)
    N = B * T
    logits = c["logits"].view(N, G, V)
    cv = c["codevectors"][0]
    x64, w64 = c["x"].double().view(N, -1), c["weight"].double()
    for name in meta["variants"]:
        train, mask = name.startswith("train"), (c["mask"].reshape(-1) if name.endswith("mask") else None)
        noise = c["gumbel"] if train else None
        assert R.top_gap(logits, noise) > meta["gap"]
        q = R.quantize(logits, noise, cv, meta["tau"], mask)
        v = f"s{i}_{name}_"
        assert np.array_equal(q["codes"].numpy(), g[v + "codes"]), name
        assert rel(q["out"].view(B, T, -1), g[v + "out"]) <= 2.0 ** -22, name            # the reference forms 1 - p + p
        assert rel(q["perplexity"], g[v + "perplexity"]) <= 1e-5, name
        if not train:
            assert q["surrogate"] is None
            continue
        dlogits, dcv = R.quantize_grads(logits, noise, cv, meta["tau"], mask, torch.full((N, G * dg), meta["a"]), meta["b"])
        dl = dlogits.view(N, G * V)
        assert rel(dcv, g[v + "dcodevectors"][0]) <= 1e-5, name
        assert rel(dl @ w64, g[v + "dx"].reshape(N, -1)) <= 1e-5, name
        assert rel(dl.t() @ x64, g[v + "dweight"]) <= 1e-5, name
        assert rel(dl.sum(0), g[v + "dbias"]) <= 1e-5, name


def test_the_golden_is_small_and_holds_only_arrays(golden):
    g, meta = golden
    assert os.path.getsize(GOLDEN) < 200 * 1024
    assert all(isinstance(v, np.ndarray) and v.dtype.kind in "fibU" for v in g.values())
    assert [tuple(s) for s in meta["shapes"]] == [(2, 5, 2, 7, 4), (2, 9, 2, 320, 8)]


# ---- span_mask ------------------------------------------------------------------------------------------------------------------

def test_span_mask_padding_minimum_and_seed():
    from conformer_amd.pretrain import span_mask
    lengths = torch.tensor([60, 10, 9, 0, 33, 11])
    for seed in range(20):
        g = torch.Generator().manual_seed(seed)
        m = span_mask(lengths, 60, 0.065, 10, g)
        assert m.dtype == torch.bool and m.shape == (6, 60)
        t = torch.arange(60)
        assert not (m & (t[None, :] >= lengths[:, None])).any()                       # never on padding
        counts = m.sum(1)
        assert all(int(counts[b]) >= 10 for b in (0, 1, 4, 5)), counts               # len >= span: at least one whole span
        assert int(counts[2]) == 0 and int(counts[3]) == 0                           # shorter than a span: nothing fits
        assert torch.equal(m, span_mask(lengths, 60, 0.065, 10, torch.Generator().manual_seed(seed)))
    # p = 0: the forced span alone, exactly `span` frames in one run
    m = span_mask(torch.tensor([40]), 40, 0.0, 7, torch.Generator().manual_seed(3))
    idx = m[0].nonzero().flatten()
    assert len(idx) == 7 and int(idx[-1] - idx[0]) == 6
    with pytest.raises(ValueError):
        span_mask(lengths, 60, 1.5, 10)


def test_span_mask_share():
    """10^4 frames in one row, p = 0.065, span = 10.  A frame s >= span - 1 away from the edges is masked unless none of the
    `span` frames that reach it started a span: q = 1 - (1 - p)^span.  The count C of masked frames sums n indicators of mean
    q, each correlated with at most 2 span - 1 of them (itself included), so Var C <= n (2 span - 1) q (1 - q): the binomial
    variance times the width of the dependence.  The forced start and the two edges move the mean by at most 2 span frames."""
    from conformer_amd.pretrain import span_mask
    n, p, span = 10000, 0.065, 10
    q = 1 - (1 - p) ** span
    sigma = math.sqrt(n * (2 * span - 1) * q * (1 - q))
    count = int(span_mask(torch.tensor([n]), n, p, span, torch.Generator().manual_seed(5)).sum())
    assert abs(count - n * q) <= 5 * sigma + 2 * span, (count, n * q, sigma)
    assert 5 * sigma / n < 0.12                                                      # the bound itself says something


# ---- sample_negatives -----------------------------------------------------------------------------------------------------------

def test_sample_negatives_rows_and_absence():
    from conformer_amd.pretrain import sample_negatives
    mask = torch.zeros(4, 30, dtype=torch.bool)
    mask[0, [2, 3, 4, 11, 29]] = True
    mask[1, 7] = True                                                                # m = 1: nothing to draw from
    mask[3, 5:25] = True
    neg = sample_negatives(mask, 50, torch.Generator().manual_seed(1))
    assert neg.dtype == torch.int32 and neg.shape == (4, 30, 50)
    assert (neg[1] == -1).all() and (neg[2] == -1).all()
    for b in (0, 3):
        assert (neg[b][~mask[b]] == -1).all()
        drawn = neg[b][mask[b]].long()                                               # (m, K)
        assert (drawn >= 0).all() and mask[b][drawn].all()                           # only masked frames of the same row
        own = mask[b].nonzero().flatten()[:, None]
        assert not (drawn == own).any()                                              # never the frame itself
    assert torch.equal(neg, sample_negatives(mask, 50, torch.Generator().manual_seed(1)))
    with pytest.raises(ValueError):
        sample_negatives(mask.float(), 5)


def test_sample_negatives_is_uniform():
    """m_b = 5, K = 4000: each masked frame draws over the 4 others, 1000 expected each.  Pearson's statistic has 3 degrees of
    freedom; P(chi2_3 > 30) is about 1.4e-6, so 30 is a bound a uniform sampler misses once in a million seeds, five frames
    included, while a sampler that never skips its own rank or favours one end misses it by hundreds."""
    from conformer_amd.pretrain import sample_negatives
    mask = torch.zeros(1, 40, dtype=torch.bool)
    pos = [1, 8, 9, 22, 39]
    mask[0, pos] = True
    neg = sample_negatives(mask, 4000, torch.Generator().manual_seed(9))
    for t in pos:
        others = [u for u in pos if u != t]
        counts = torch.tensor([(neg[0, t] == u).sum() for u in others], dtype=torch.float64)
        assert int(counts.sum()) == 4000
        assert float(((counts - 1000.0) ** 2 / 1000.0).sum()) <= 30.0, (t, counts)


# ---- modules --------------------------------------------------------------------------------------------------------------------

def test_exported_keys_are_the_encoders():
    from model.modules.encoder import Encoder
    from model.modules.quantization import Quantization
    from model.wav2vec2 import Wav2Vec2
    w = Wav2Vec2(2, 80, 32, 4, 7, 16, 2, 8)
    e = Encoder(80, 2, 32, 4, 7)
    sd = w.export_encoder_state_dict()
    assert set(sd) == set(e.state_dict())
    assert all(sd[k].shape == v.shape for k, v in e.state_dict().items())
    assert e.load_state_dict(sd, strict=True).missing_keys == []
    heads = {k.split(".", 1)[0] for k in w.state_dict()}
    assert heads == {"downsampling_conv", "linear", "rel_pe", "blocks", "quantization", "hidden_projector",
                     "quantization_projector"}
    q = Quantization(32, 80, 2, 8, 16)
    assert set(q.state_dict()) == {"codevectors", "weight_proj.weight", "weight_proj.bias"}
    assert q.codevectors.shape == (1, 16, 8) and 0 <= float(q.codevectors.detach().min()) and float(q.codevectors.detach().max()) <= 1
    assert q.temperature == 2
    with pytest.raises(ValueError):
        Quantization(32, 80, 3, 8, 16)


def test_host_tensors_are_refused():
    from conformer_amd import pretrain
    from conformer_amd.evaluation import ConformerCriterion
    x = torch.zeros(4, 2, 5)
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        pretrain.gumbel_quantize(x, torch.zeros(10, 3), 2.0)
    c = torch.zeros(1, 4, 8)
    with pytest.raises(_lib.ConformerHipError, match="no CPU fallback"):
        pretrain.contrastive_loss(c, c, torch.ones(1, 4, dtype=torch.bool), torch.zeros(1, 4, 2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ConformerCriterion(0).pretrain_loss(c, c, torch.tensor(1.0), torch.ones(1, 4, dtype=torch.bool))


# ---- the C entries --------------------------------------------------------------------------------------------------------------

def test_the_header_is_discovered():
    path = os.path.join(CSRC, HEADER)
    assert path in _lib.OPEN_HEADERS
    assert _lib.OPEN_CONSTANTS[HEADER] == {
        "CFM3_PRETRAIN_MAX_V": 1024, "CFM3_PRETRAIN_MAX_G": 8, "CFM3_PRETRAIN_MAX_DG": 512, "CFM3_PRETRAIN_MAX_D": 1024,
        "CFM3_PRETRAIN_MAX_K": 256, "CFM3_QUANT_ROWS": 32, "CFM3_QUANT_BWD_ROWS": 16, "CFM3_QUANT_FWD_LAUNCHES": 2,
        "CFM3_QUANT_BWD_LAUNCHES": 2, "CFM3_CONTRASTIVE_FWD_LAUNCHES": 3, "CFM3_CONTRASTIVE_BWD_LAUNCHES": 2}
    assert tuple(_lib.OPEN[path].signatures) == ENTRIES
    src = open(os.path.join(CSRC, "pretrain.hip")).read()
    found = dict(re.findall(r'extern\s+"C"[^;{()]*?\b(cfm3_\w+)\s*\(([^()]*)\)\s*\{', src))
    assert set(found) == set(ENTRIES)
    for name, args in found.items():
        assert len(args.split(",")) == len(_lib.OPEN_ENTRIES[name][1]) == len(_lib.OPEN_PARAMS[name]), name
    # the launches the header states are the ones the entries enqueue
    for entry, define in (("cfm3_quantize_fwd_f32", "CFM3_QUANT_FWD_LAUNCHES"), ("cfm3_quantize_bwd_f32", "CFM3_QUANT_BWD_LAUNCHES"),
                          ("cfm3_contrastive_fwd_f32", "CFM3_CONTRASTIVE_FWD_LAUNCHES"),
                          ("cfm3_contrastive_bwd_f32", "CFM3_CONTRASTIVE_BWD_LAUNCHES")):
        body = src[src.index(f"int {entry}("):]
        body = body[:body.index("return cfm_launch_status();")]
        paths = re.sub(r"(?s)switch.*?\n    \}", "hipLaunchKernelGGL;", body)           # a switch launches one of its cases
        paths = re.sub(r"(?m)^\s*else.*hipLaunchKernelGGL.*$", "", paths)                # ... and so does an if / else chain
        assert paths.count("hipLaunchKernelGGL") == _lib.OPEN_CONSTANTS[HEADER][define], entry
    assert _lib.OPEN_ENTRIES["cfm3_quantize_fwd_f32"][1][8] is ctypes.c_float
    assert _lib.OPEN_PARAMS["cfm3_contrastive_fwd_f32"][5:10] == ["B", "T", "D", "K", "temperature"]
    assert (len(_lib.ENTRIES), len(_lib.EXTRA_ENTRIES)) == (162, 4)                      # the closed tables did not move
    from conformer_amd import ops
    assert ops.PRETRAIN_LIMITS == {"V": 1024, "G": 8, "DG": 512, "D": 1024, "K": 256}


def test_workspace_floats(lib):
    qw, cw = lib.cfm3_quantize_workspace_floats, lib.cfm3_contrastive_workspace_floats
    for N, G, V in [(1, 1, 1), (45, 2, 320), (130, 3, 1024), (7968, 2, 320), (32, 8, 5), (33, 1, 64)]:
        nblk = (N + 31) // 32
        assert qw(N, G, V) == 2 * N * G + G * V + 4 + nblk * G * V + nblk, (N, G, V)
    for bad in ((0, 2, 7), (3, 0, 7), (3, 2, 0), (3, 9, 7), (3, 2, 1025), (1 << 30, 8, 4), (-1, 2, 7)):
        assert qw(*bad) == -1, bad
    for B, T, K in [(1, 2, 1), (3, 40, 100), (32, 249, 100), (2, 33, 256)]:
        assert cw(B, T, K) == 2 * B * T * (K + 2), (B, T, K)
    for bad in ((0, 4, 3), (2, 0, 3), (2, 4, 0), (2, 4, 257), (1 << 20, 1 << 10, 4), (2, -4, 3)):
        assert cw(*bad) == -1, bad
    # nothing of B T K D elements: at the benchmark's shape the workspace is under 1 % of the (M, K + 1, D) block
    assert cw(32, 249, 100) * 4 < 32 * 125 * 101 * 256 * 4 // 50


def test_refusals_before_any_hip_call(lib):
    buf = (ctypes.c_double * 4096)()
    a = (ctypes.addressof(buf) + 15) // 16 * 16
    NULL, SHAPE, UNSUPPORTED, ALIGN = (_lib.CONSTANTS[k] for k in ("CFM_ERR_NULL", "CFM_ERR_BAD_SHAPE", "CFM_ERR_UNSUPPORTED",
                                                                   "CFM_ERR_ALIGN"))

    def call(entry, base, **kw):
        args = list(base)
        for k, v in kw.items():
            args[int(k[1:])] = v
        assert args != list(base), "an accepted call would launch"
        return entry(*args)

    # logits, noise, codevectors, row_mask, N, G, V, dg, tau, workspace, codes, out, marginal, perplexity, stream
    fwd = (lib.cfm3_quantize_fwd_f32, [a, a, a, a, 3, 2, 7, 4, 2.0, a, a, a, a, a, None], (0, 2, 9, 10, 11, 12, 13), 4, 8, 9)
    # logits, noise, codevectors, row_mask, codes, dout, dperplexity, N, G, V, dg, tau, workspace, dlogits, dcodevectors, stream
    bwd = (lib.cfm3_quantize_bwd_f32, [a, a, a, a, a, a, a, 3, 2, 7, 4, 2.0, a, a, a, None], (0, 1, 2, 4, 5, 6, 12, 13, 14), 7, 11,
           12)
    for entry, good, pointers, n0, tau, ws in (fwd, bwd):
        for i in pointers:                                                   # bwd: a null noise is the eval path
            assert call(entry, good, **{f"a{i}": None}) == NULL, i
        for i in range(n0, n0 + 4):                                          # N, G, V, dg
            assert call(entry, good, **{f"a{i}": 0}) == SHAPE, i
            assert call(entry, good, **{f"a{i}": -1}) == SHAPE, i
        for bad in (0.0, -2.0, float("nan"), float("inf")):
            assert call(entry, good, **{f"a{tau}": bad}) == SHAPE, bad
        assert call(entry, good, **{f"a{n0 + 1}": 9}) == UNSUPPORTED          # G
        assert call(entry, good, **{f"a{n0 + 2}": 1025}) == UNSUPPORTED       # V
        assert call(entry, good, **{f"a{n0 + 3}": 513}) == UNSUPPORTED        # dg
        assert call(entry, good, **{f"a{n0}": 1 << 30, f"a{n0 + 1}": 8}) == UNSUPPORTED      # N G
        assert call(entry, good, **{f"a{ws}": a + 4}) == ALIGN
        # the order: NULL, shape, the limits, the alignment
        assert call(entry, good, a0=None, **{f"a{n0}": 0}) == NULL
        assert call(entry, good, **{f"a{n0}": 0, f"a{n0 + 2}": 1025}) == SHAPE
        assert call(entry, good, **{f"a{n0 + 2}": 1025, f"a{ws}": a + 4}) == UNSUPPORTED
    # context, targets, mask, negatives, ids, B, T, D, K, temperature, workspace, frame_loss, correct, loss, n_correct, stream
    cf = (lib.cfm3_contrastive_fwd_f32, [a, a, a, a, a, 2, 5, 8, 3, 0.1, a, a, a, a, a, None], (0, 1, 2, 3, 10, 11, 12, 13, 14), 5, 9,
          10)
    # context, targets, mask, negatives, order, start, gframe, B, T, D, K, temperature, workspace, dcontext, dtargets, stream
    cb = (lib.cfm3_contrastive_bwd_f32, [a, a, a, a, a, a, a, 2, 5, 8, 3, 0.1, a, a, a, None], (0, 1, 2, 3, 4, 5, 6, 12, 13, 14), 7,
          11, 12)
    for entry, good, pointers, n0, temp, ws in (cf, cb):
        for i in pointers:
            assert call(entry, good, **{f"a{i}": None}) == NULL, i
        for i in range(n0, n0 + 4):                                          # B, T, D, K
            assert call(entry, good, **{f"a{i}": 0}) == SHAPE, i
            assert call(entry, good, **{f"a{i}": -1}) == SHAPE, i
        for bad in (0.0, -0.1, float("nan"), float("inf")):
            assert call(entry, good, **{f"a{temp}": bad}) == SHAPE, bad
        assert call(entry, good, **{f"a{n0 + 2}": 1025}) == UNSUPPORTED       # D
        assert call(entry, good, **{f"a{n0 + 3}": 257}) == UNSUPPORTED        # K
        assert call(entry, good, **{f"a{n0}": 1 << 20, f"a{n0 + 1}": 1 << 10, f"a{n0 + 3}": 4}) == UNSUPPORTED       # B T K
        assert call(entry, good, **{f"a{ws}": a + 4}) == ALIGN
        assert call(entry, good, a0=a + 4) == ALIGN and call(entry, good, a1=a + 8) == ALIGN     # D % 4 == 0: 16-byte rows
        assert call(entry, good, a0=None, **{f"a{n0}": 0}) == NULL
        assert call(entry, good, **{f"a{n0}": 0, f"a{n0 + 2}": 1025}) == SHAPE
        assert call(entry, good, **{f"a{n0 + 2}": 1025, f"a{ws}": a + 4}) == UNSUPPORTED
    assert call(cb[0], cb[1], a4=a + 4) == ALIGN and call(cb[0], cb[1], a5=a + 4) == ALIGN      # order, start: int64
