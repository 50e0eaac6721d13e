"""Self-supervised pretraining on the MI355X (csrc/pretrain.hip; conformer_amd.pretrain, model.wav2vec2.Wav2Vec2,
ConformerCriterion.pretrain_loss) against the float64 restatement of tests/pretrain_restatement.py.

THE TOLERANCES are not tuned to what the kernels give.  Every comparison is |got - ref| <= f * scale, element by element, where
`scale` is the sum of the absolute values of the terms the element is a sum of (restatement *_scales; 0 where the definition
says exact zero), and f is the larger of
  (a) a rounding bound from the shape and the fp32 unit roundoff u = 2^-24, derived where it is computed below, and
  (b) 4 x the largest error / scale of the stock-PyTorch fp32 formulation of the same quantity (the restatement run in float32
      on the device) on the same inputs: summation order alone moves an fp32 result by a small multiple.
The figures are printed before they are asserted (pytest -s)."""
import json
import math
import os

import numpy as np
import pytest
import torch

from conformer_amd import _lib, ops, pretrain
from conformer_amd.evaluation import ConformerCriterion
from tests import pretrain_restatement as R
from tests.test_write_guard_gpu import guarded_allocations
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEFINES = _lib.OPEN_CONSTANTS["conformer_hip3_pretrain.h"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def held(name, got, ref, scale, f_a, stock=None):
    """assert |got - ref| <= max(f_a, 4 x the stock formulation's error / scale) * scale; prints the figures first"""
    got, ref, scale = got.detach().double().cpu(), ref.detach().double().cpu(), scale.double()
    live = scale > 0
    f_b = 0.0
    if stock is not None:
        es = (stock.detach().double().cpu() - ref).abs()
        f_b = 4 * float((es[live] / scale[live]).max()) if bool(live.any()) else 0.0
    err = (got - ref).abs()
    worst = float((err[live] / scale[live]).max()) if bool(live.any()) else 0.0
    print(f"{name}: error/scale {worst:.3e}  bound (a) {f_a:.3e}  bound (b) {f_b:.3e}")
    assert bool(torch.isfinite(got).all()), name
    assert bool((err <= max(f_a, f_b) * scale).all()), (name, worst, f_a, f_b)


# ---- the quantizer --------------------------------------------------------------------------------------------------------------

Q_SHAPES = [(1, 1, 1, 1), (3, 2, 7, 4), (10, 2, 65, 8), (45, 2, 320, 128), (130, 3, 1024, 5)]
TAU = 2.0
_Q = {}


def q_case(shape):
    """inputs at `shape` and their float64 restatement with a mixed mask, computed once and never changed"""
    if shape not in _Q:
        N, G, V, dg = shape
        g = torch.Generator().manual_seed(7 + N)
        logits = 2 * torch.randn(N, G, V, generator=g)
        noise = -torch.empty(N, G, V).exponential_(generator=g).log()
        cv = torch.rand(G * V, dg, generator=g)
        mask = torch.rand(N, generator=g) < 0.5
        mask[0] = True
        dout = torch.randn(N, G * dg, generator=g)
        dperp = 0.37
        assert R.top_gap(logits, noise) > 0 and R.top_gap(logits, None) > 0               # no fp32 tie: the codes are decided
        c = dict(logits=logits, noise=noise, cv=cv, mask=mask, dout=dout, dperp=dperp)
        c["ref"] = R.quantize(logits, noise, cv, TAU, mask)
        c["grads"] = R.quantize_grads(logits, noise, cv, TAU, mask, dout, dperp)
        c["scales"] = R.quantize_scales(logits, noise, cv, TAU, mask, dout, dperp)
        _Q[shape] = c
    return _Q[shape]


def q_bound(shape, c):
    """(a) for the quantizer.  gy is a dot of dg products and <gy, y>, <p, c> sums of V: (dg + 2 V) u.  y and p are exp of an
    argument of size `arg` whose own rounding is arg u, twice (the argument and the stored log-sum-exp): 8 arg u with the
    hardware's 2 ulp.  The marginal is a sum of N terms of V-term softmaxes, (N + V) u, and enters c through log m and exp H,
    H a V-term sum of m log m: (N + V) (ln V + 2) u.  64 u covers the fixed count of other roundings."""
    N, G, V, dg = shape
    arg = float(torch.maximum((c["logits"] + c["noise"]).abs() / TAU, c["logits"].abs()).max()) + math.log(V)
    marg = (N + V + 64 + 8 * arg) * U
    return (dg + 2 * V + 64 + 8 * arg + (N + V) * (math.log(V) + 2)) * U, marg


@pytest.mark.parametrize("shape", Q_SHAPES)
def test_quantizer_against_the_restatement(dev, shape):
    N, G, V, dg = shape
    c = q_case(shape)
    t = {k: c[k].to(dev) for k in ("logits", "noise", "cv", "mask", "dout")}
    out, codes, perp, marginal, ctx = ops.quantize_forward(t["logits"], t["cv"], TAU, t["noise"], t["mask"])
    ref = c["ref"]
    assert torch.equal(codes.cpu().long(), ref["codes"]) and codes.dtype == torch.int32
    rows = torch.stack([c["cv"].view(G, V, dg)[g][ref["codes"][:, g]] for g in range(G)], 1).reshape(N, -1)
    assert torch.equal(out.cpu(), rows)                                                  # a gather: the same bits
    f_a, f_m = q_bound(shape, c)
    stock = R.quantize(t["logits"], t["noise"], t["cv"], TAU, t["mask"], dtype=torch.float32)
    held("marginal", marginal, ref["marginal"], c["scales"]["marginal"], f_m, stock["marginal"])
    held("perplexity", perp, ref["perplexity"], c["scales"]["perplexity"] + ref["perplexity"].detach(), f_m + (V + 8) * U,
         stock["perplexity"])
    dperp = torch.tensor(c["dperp"], device=dev)
    dlogits, dcv = ops.quantize_backward(ctx, t["dout"], dperp)
    sl, sc = R.quantize_grads(t["logits"], t["noise"], t["cv"], TAU, t["mask"], t["dout"], c["dperp"], dtype=torch.float32)
    held("dlogits", dlogits, c["grads"][0], c["scales"]["dlogits"], f_a, sl)
    held("dcodevectors", dcv, c["grads"][1], c["scales"]["dcodevectors"], N * U, sc)
    # a code nobody chose has an exactly zero row
    chosen = torch.zeros(G * V, dtype=torch.bool)
    chosen[(ref["codes"] + V * torch.arange(G)[None, :]).reshape(-1)] = True
    assert float(dcv.cpu()[~chosen].abs().sum()) == 0.0
    assert V <= N or bool((~chosen).any())                                               # ... and the larger shapes have some
    # two runs, the same bits
    out2, codes2, perp2, marginal2, ctx2 = ops.quantize_forward(t["logits"], t["cv"], TAU, t["noise"], t["mask"])
    dl2, dc2 = ops.quantize_backward(ctx2, t["dout"], dperp)
    for a, b in ((out, out2), (codes, codes2), (perp, perp2), (marginal, marginal2), (dlogits, dl2), (dcv, dc2)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("which", ["all", "none", "null"])
def test_quantizer_row_masks(dev, which):
    shape = (45, 2, 320, 128)
    N, G, V, dg = shape
    c = q_case(shape)
    mask = {"all": torch.ones(N, dtype=torch.bool), "none": torch.zeros(N, dtype=torch.bool), "null": None}[which]
    t = {k: c[k].to(dev) for k in ("logits", "noise", "cv", "dout")}
    out, codes, perp, marginal, ctx = ops.quantize_forward(t["logits"], t["cv"], TAU, t["noise"], None if mask is None else mask.to(dev))
    ref = R.quantize(c["logits"], c["noise"], c["cv"], TAU, mask)
    sc = R.quantize_scales(c["logits"], c["noise"], c["cv"], TAU, mask, c["dout"], c["dperp"])
    f_a, f_m = q_bound(shape, c)
    held("marginal", marginal, ref["marginal"], sc["marginal"], f_m)
    held("perplexity", perp, ref["perplexity"], sc["perplexity"] + ref["perplexity"], f_m + (V + 8) * U)
    if which == "none":
        assert float(perp) == float(G) and float(marginal.abs().sum()) == 0.0            # defined: m = 0, exp(0) per group
    dlogits, dcv = ops.quantize_backward(ctx, t["dout"], torch.tensor(c["dperp"], device=dev))
    gl, gc = R.quantize_grads(c["logits"], c["noise"], c["cv"], TAU, mask, c["dout"], c["dperp"])
    held("dlogits", dlogits, gl, sc["dlogits"], f_a)
    held("dcodevectors", dcv, gc, sc["dcodevectors"], N * U)
    if which == "null":                                                                  # no mask = every row counts: the same bits
        every = ops.quantize_forward(t["logits"], t["cv"], TAU, t["noise"], torch.ones(N, dtype=torch.bool, device=dev))
        assert torch.equal(every[2], perp) and torch.equal(every[3], marginal)


@pytest.mark.parametrize("shape", [(3, 2, 7, 4), (130, 3, 1024, 5)])
def test_quantizer_eval_path(dev, shape):
    N, G, V, dg = shape
    c = q_case(shape)
    lg, cv, mask = c["logits"].to(dev), c["cv"].to(dev), c["mask"].to(dev)
    out, codes, perp, marginal, ctx = ops.quantize_forward(lg, cv, TAU, None, mask)
    ref = R.quantize(c["logits"], None, c["cv"], TAU, c["mask"])
    assert torch.equal(codes.cpu().long(), ref["codes"]) and torch.equal(out.cpu().double(), ref["out"])
    assert torch.equal(marginal.cpu().double(), ref["marginal"])                          # counts: exact
    held("perplexity", perp, ref["perplexity"], ref["perplexity"] * (math.log(V) + 2), (N + V + 64) * U)
    with pytest.raises(_lib.ConformerHipError, match="not differentiable"):
        ops.quantize_backward(ctx, c["dout"].to(dev), torch.ones((), device=dev))
    o2, c2, p2 = pretrain.gumbel_quantize(lg.requires_grad_(True), cv, TAU, row_mask=mask, hard_eval=True)
    assert torch.equal(o2, out) and torch.equal(c2, codes) and not o2.requires_grad
    # drawn noise: the public op draws Gumbel values itself and differs from run to run only through them
    o3, c3, p3 = pretrain.gumbel_quantize(lg, cv.requires_grad_(True), TAU, row_mask=mask)
    (o3.sum() + p3).backward()
    assert o3.requires_grad and bool(torch.isfinite(lg.grad).all()) and bool(torch.isfinite(cv.grad).all())


def test_quantizer_writes_stay_inside_their_buffers(dev):
    for shape in [(3, 2, 7, 4), (130, 3, 1024, 5), (45, 2, 320, 128)]:
        c = q_case(shape)
        t = {k: c[k].to(dev) for k in ("logits", "noise", "cv", "mask", "dout")}
        dperp = torch.ones((), device=dev)
        with guarded_allocations() as gt:
            out, codes, perp, marginal, ctx = ops.quantize_forward(t["logits"], t["cv"], TAU, t["noise"], t["mask"])
            dlogits, dcv = ops.quantize_backward(ctx, t["dout"], dperp)
            bad, n = gt.check(), len(gt.allocs)
        assert n >= 7 and not bad, (shape, bad)
        assert torch.equal(codes.cpu().long(), c["ref"]["codes"])


# ---- the contrastive loss -------------------------------------------------------------------------------------------------------

C_SHAPES = [(1, 2, 1, 1), (2, 7, 24, 3), (3, 40, 256, 100), (2, 33, 1024, 256)]
TEMP = 0.1
_C = {}


def c_case(shape):
    """A hand-built batch at `shape` (what it holds is listed in `facts`) with its float64 restatement, computed once."""
    if shape in _C:
        return _C[shape]
    B, T, D, K = shape
    g = torch.Generator().manual_seed(31 + T)
    context, targets = torch.randn(B, T, D, generator=g), torch.randn(B, T, D, generator=g)
    mask = torch.rand(B, T, generator=g) < 0.6
    negatives = torch.randint(0, T, (B, T, K), generator=g, dtype=torch.int32)           # any frame of the row, masked or not
    ids = torch.randint(0, 4, (B, T), generator=g)
    facts = {}
    if T == 2:
        mask[:] = True
        negatives[0, 0, 0], negatives[0, 1, 0] = 1, 0
        ids = None
    else:
        mask[0, :4] = True
        popular, nobody, zero, shut = 1, T - 1, 2, 3
        mask[0, nobody] = False
        negatives[0][negatives[0] == nobody] = 0                                         # a frame nobody draws, and unmasked
        negatives[0, :, 0] = popular                                                     # a frame everybody draws
        negatives[0, 0, K - 1], negatives[0, 1, K - 1] = -1, T                           # out of range: absent
        if K > 2:
            negatives[0, 2, 1], negatives[0, 3, 1] = T + 5, -7
        context[0, zero] = 0.0                                                           # the 1e-8 clamp
        ids[0, zero] = 7                                                                 # ... with an id of its own: negatives stay
        negatives[0, shut, :] = popular                                                  # ids shut every negative of this frame out
        ids[0, shut] = ids[0, popular]
        mask[1] = False
        mask[1, T // 2] = True                                                           # exactly one masked frame
        negatives[1, T // 2, :] = -1
        facts = dict(popular=(0, popular), nobody=(0, nobody), zero=(0, zero), shut=(0, shut), single=(1, T // 2))
        if B > 2:
            mask[2] = False                                                              # a row without a masked frame
            negatives[2, 0, 0] = 10 * T
    gframe = torch.rand(B, T, generator=g) + 0.5
    c = dict(context=context, targets=targets, mask=mask, negatives=negatives, ids=ids, gframe=gframe, facts=facts)
    c["ref"] = R.contrastive(context, targets, mask, negatives, ids, TEMP)
    c["grads"] = R.contrastive_grads(context, targets, mask, negatives, ids, TEMP, gframe)
    c["scales"] = R.contrastive_scales(context, targets, mask, negatives, ids, TEMP, gframe)
    _C[shape] = c
    return c


def c_bounds(shape):
    """(a) for the contrastive loss.  A cosine is a D-term dot over a product of two norms, each the root of a D-term sum: by
    Cauchy-Schwarz its absolute error is at most (2 D + 8) u, so z = cos / temperature moves by dz = (2 D + 8) u / temperature.
    frame_loss = logsumexp(z) - z_0 moves by 2 dz plus the (K + 16) u (1 + |z|max) of a (K + 1)-term log-sum-exp, |z| <= 1 /
    temperature.  A softmax weight moves by 2 dz + (K + 16) u relative to itself; a gradient row is a sum of up to K + 1 such
    weighted rows plus the own-row term, each with its own D-term dot: (K + D + 64) u more."""
    B, T, D, K = shape
    dz = (2 * D + 8) * U / TEMP
    loss = 2 * dz + (K + 16) * U * (1 + 1 / TEMP)
    return loss, 2 * dz + (K + 16) * U + (K + D + 64) * U


def c_run(c, dev):
    t = {k: (None if c[k] is None else c[k].to(dev)) for k in ("context", "targets", "mask", "negatives", "ids", "gframe")}
    loss, frame_loss, n_correct, correct, ctx = ops.contrastive_forward(t["context"], t["targets"], t["mask"], t["negatives"],
                                                                        t["ids"], TEMP)
    dcontext, dtargets = ops.contrastive_backward(ctx, t["gframe"])
    return t, (loss, frame_loss, n_correct, correct, dcontext, dtargets)


@pytest.mark.parametrize("shape", C_SHAPES)
def test_contrastive_loss_against_the_restatement(dev, shape):
    B, T, D, K = shape
    c = c_case(shape)
    t, (loss, frame_loss, n_correct, correct, dcontext, dtargets) = c_run(c, dev)
    ref, mask = c["ref"], c["mask"]
    f_loss, f_grad = c_bounds(shape)
    stock = R.contrastive(t["context"], t["targets"], t["mask"], t["negatives"], t["ids"], TEMP, dtype=torch.float32)
    ones = torch.ones(B, T, dtype=torch.float64)
    held("frame_loss", frame_loss, ref["frame_loss"], ones * mask, f_loss, stock["frame_loss"])
    held("loss", loss, ref["loss"], torch.tensor(float(mask.sum())) * (1 + ref["frame_loss"].max()), f_loss + B * T * U,
         stock["loss"])
    assert float(frame_loss.cpu()[~mask].abs().sum()) == 0.0 and int(correct.cpu()[~mask].sum()) == 0
    # correct: wherever the positive wins or loses by more than the bound on z decides it
    z = ref["z"]
    others = z[..., 1:].max(-1).values if K else None
    decided = mask & ((z[..., 0] - others).abs() > 2 * f_loss)
    assert torch.equal(correct.cpu().bool()[decided], ref["correct"][decided])
    assert abs(int(n_correct) - int(ref["correct"].sum())) <= int((mask & ~decided).sum())
    assert int(n_correct) == int(correct.sum())
    sd, st = R.contrastive_grads(t["context"], t["targets"], t["mask"], t["negatives"], t["ids"], TEMP, t["gframe"],
                                 dtype=torch.float32)
    held("dcontext", dcontext, c["grads"][0], c["scales"]["dcontext"], f_grad, sd)
    held("dtargets", dtargets, c["grads"][1], c["scales"]["dtargets"], f_grad, st)
    f = c["facts"]
    if f:
        fl, dc, dt = frame_loss.cpu(), dcontext.cpu(), dtargets.cpu()
        assert float(fl[f["shut"]]) == 0.0 and float(dc[f["shut"]].abs().sum()) == 0.0   # ids shut every negative out
        assert float(fl[f["single"]]) == 0.0 and float(dc[1].abs().sum()) == 0.0 and float(dt[1].abs().sum()) == 0.0
        assert float(dt[f["nobody"]].abs().sum()) == 0.0                                 # unmasked and never drawn: exact zeros
        assert float(dt[f["popular"]].abs().sum()) > 0.0
        assert float(dc[0][~mask[0]].abs().sum()) == 0.0                                 # unmasked frames
        assert bool(torch.isfinite(dc[f["zero"]]).all()) and float(dc[f["zero"]].abs().max()) > 1e3      # d cos / d a = c / 1e-8
        if B > 2:
            assert float(dc[2].abs().sum()) == 0.0 and float(dt[2].abs().sum()) == 0.0 and float(fl[2].abs().sum()) == 0.0
    # two runs, the same bits
    _, again = c_run(c, dev)
    for a, b in zip((loss, frame_loss, n_correct, correct, dcontext, dtargets), again):
        assert torch.equal(a, b)


def test_contrastive_without_ids_and_through_autograd(dev):
    shape = (2, 7, 24, 3)
    c = c_case(shape)
    ctx_, tgt_ = c["context"].to(dev).requires_grad_(True), c["targets"].to(dev).requires_grad_(True)
    loss, frame_loss, n_correct = pretrain.contrastive_loss(ctx_, tgt_, c["mask"].to(dev), c["negatives"].to(dev), None, TEMP)
    (2 * loss + (frame_loss * c["gframe"].to(dev)).sum()).backward()
    gd, gt = R.contrastive_grads(c["context"], c["targets"], c["mask"], c["negatives"], None, TEMP, c["gframe"] + 2)
    sc = R.contrastive_scales(c["context"], c["targets"], c["mask"], c["negatives"], None, TEMP, c["gframe"] + 2)
    f_loss, f_grad = c_bounds(shape)
    ref = R.contrastive(c["context"], c["targets"], c["mask"], c["negatives"], None, TEMP)
    held("frame_loss", frame_loss, ref["frame_loss"], torch.ones(2, 7, dtype=torch.float64) * c["mask"], f_loss)
    held("dcontext", ctx_.grad, gd, sc["dcontext"], f_grad)
    held("dtargets", tgt_.grad, gt, sc["dtargets"], f_grad)
    assert n_correct.dtype == torch.int32 and not n_correct.requires_grad


def test_contrastive_writes_stay_inside_their_buffers(dev):
    for shape in C_SHAPES:
        c = c_case(shape)
        t = {k: (None if c[k] is None else c[k].to(dev)) for k in ("context", "targets", "mask", "negatives", "ids", "gframe")}
        with guarded_allocations() as gt:
            loss, frame_loss, n_correct, correct, ctx = ops.contrastive_forward(t["context"], t["targets"], t["mask"],
                                                                                t["negatives"], t["ids"], TEMP)
            dcontext, dtargets = ops.contrastive_backward(ctx, t["gframe"])
            bad, n = gt.check(), len(gt.allocs)
        assert n >= 7 and not bad, (shape, bad)


def test_launch_counts(dev):
    """one C call per forward and per backward; the kernels each enqueues are the header's CFM3_*_LAUNCHES (held to the source
    in test_pretrain_cpu.py)"""
    q, c = q_case((10, 2, 65, 8)), c_case((2, 7, 24, 3))
    t = {k: q[k].to(dev) for k in ("logits", "noise", "cv", "mask", "dout")}
    one = torch.ones((), device=dev)
    n0 = _lib.CALLS[0]
    *_, ctx = ops.quantize_forward(t["logits"], t["cv"], TAU, t["noise"], t["mask"])
    n1 = _lib.CALLS[0]
    ops.quantize_backward(ctx, t["dout"], one)
    u = {k: (None if c[k] is None else c[k].to(dev)) for k in ("context", "targets", "mask", "negatives", "ids", "gframe")}
    n2 = _lib.CALLS[0]
    *_, cctx = ops.contrastive_forward(u["context"], u["targets"], u["mask"], u["negatives"], u["ids"], TEMP)
    n3 = _lib.CALLS[0]
    ops.contrastive_backward(cctx, u["gframe"])
    n4 = _lib.CALLS[0]
    assert (n1 - n0, n2 - n1, n3 - n2, n4 - n3) == (1, 1, 1, 1)
    assert [DEFINES[k] for k in ("CFM3_QUANT_FWD_LAUNCHES", "CFM3_QUANT_BWD_LAUNCHES", "CFM3_CONTRASTIVE_FWD_LAUNCHES",
                                 "CFM3_CONTRASTIVE_BWD_LAUNCHES")] == [2, 2, 3, 2]
    # a refused call has launched nothing and counts as one failed call
    with pytest.raises(_lib.ConformerHipError):
        ops.quantize_forward(t["logits"], t["cv"], 0.0, t["noise"], t["mask"])
    with pytest.raises(_lib.ConformerHipError):
        ops.contrastive_forward(u["context"], u["targets"], u["mask"], u["negatives"], u["ids"], -1.0)


# ---- the reference's Quantization, on the device --------------------------------------------------------------------------------

@pytest.mark.parametrize("i", [0, 1])
def test_golden_through_quantization(dev, i):
    from model.modules.quantization import Quantization
    z = np.load(os.path.join(ROOT, "tests", "golden", "pretrain_quantizer.npz"))
    meta = json.loads(str(z["meta"]))
    B, T, G, V, dg = meta["shapes"][i]
    q = Quantization(meta["d_model"], meta["n_mel"], G, V, G * dg)
    q.load_state_dict({"codevectors": torch.from_numpy(z[f"s{i}_codevectors"]), "weight_proj.weight": torch.from_numpy(z[f"s{i}_weight"]),
                       "weight_proj.bias": torch.from_numpy(z[f"s{i}_bias"])}, strict=True)
    q = q.to(dev)
    q.temperature = meta["tau"]
    mask, noise = torch.from_numpy(z[f"s{i}_mask"]).to(dev), torch.from_numpy(z[f"s{i}_gumbel"]).to(dev)
    for name in meta["variants"]:
        train = name.startswith("train")
        q.train(train)
        q.zero_grad()
        x = torch.from_numpy(z[f"s{i}_x"]).to(dev).requires_grad_(train)
        out, perp = q(x, mask if name.endswith("mask") else None, noise=noise if train else None)
        v = f"s{i}_{name}_"
        assert np.array_equal(q.last_codes.view(B * T, G).cpu().numpy(), z[v + "codes"]), name
        assert rel_l2(out, torch.from_numpy(z[v + "out"])) <= 2e-5 and rel_l2(perp, torch.from_numpy(z[v + "perplexity"])) <= 2e-5
        if train:
            (out.sum() * meta["a"] + perp * meta["b"]).backward()
            for got, key in ((x.grad, "dx"), (q.codevectors.grad, "dcodevectors"), (q.weight_proj.weight.grad, "dweight"),
                             (q.weight_proj.bias.grad, "dbias")):
                r = rel_l2(got, torch.from_numpy(z[v + key]))
                print(name, key, r)
                assert r <= 2e-5, (name, key, r)


# ---- end to end -----------------------------------------------------------------------------------------------------------------

def tiny(dev, seed=0):
    from model.wav2vec2 import Wav2Vec2
    torch.manual_seed(seed)
    m = Wav2Vec2(2, 80, 32, 4, 7, 16, 2, 8, time_augment=4, time_mask_ratio=0.2).to(dev)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 80, 120, generator=g).to(dev)
    return m, x, torch.tensor([120, 90], device=dev)


def test_wav2vec2_forward_loss_backward(dev):
    m, x, lengths = tiny(dev)
    crit = ConformerCriterion(0)

    def step(seed):
        m.zero_grad()
        g = torch.Generator(device=dev).manual_seed(seed)
        torch.manual_seed(seed)                                                          # the quantizer's own Gumbel draw
        context, target, perplexity, mask = m(x, lengths, generator=g)
        loss = crit.pretrain_loss(context, target, perplexity, mask, codes=m.quantization.last_codes, num_negatives=10,
                                  generator=g, num_codevectors=16)
        loss.backward()
        return loss, context, target, mask

    loss, context, target, mask = step(3)
    T2 = context.shape[1]
    assert context.shape == target.shape == (2, T2, 16) and mask.shape == (2, T2) and mask.dtype == torch.bool
    out_len = ((lengths - 1) // 2 - 1) // 2
    assert not bool((mask & (torch.arange(T2, device=dev)[None, :] >= out_len[:, None])).any())       # never on padding
    assert bool((mask.sum(1) >= 4).all())
    assert bool(torch.isfinite(loss))
    for name, p in m.named_parameters():
        if name.startswith("rel_pe."):                   # the sinusoid table's frequencies: a constant, as in the Encoder
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    for part in ("downsampling_conv", "linear", "blocks", "quantization", "hidden_projector", "quantization_projector"):
        assert any(float(p.grad.abs().max()) > 0 for n, p in m.named_parameters() if n.startswith(part + ".")), part
    acc = crit.last_pretrain["accuracy"]
    assert 0.0 <= float(acc) <= 1.0 and int(crit.last_pretrain["n_masked"]) == int(mask.sum())
    again, *_ = step(3)
    assert torch.equal(loss, again)                                                      # the same seed, the same bits
    m.eval()
    with torch.no_grad():
        c2, t2, p2, k2 = m(x, lengths, generator=torch.Generator(device=dev).manual_seed(3))
    assert torch.equal(k2, mask) and bool(torch.isfinite(c2).all()) and 2.0 <= float(p2) <= 16.0


def test_ten_adam_steps_lower_the_loss(dev):
    """a sanity check of the gradient's sign: one fixed batch, mask, negatives and noise"""
    m, x, lengths = tiny(dev, seed=1)
    crit = ConformerCriterion(0)
    g = torch.Generator(device=dev).manual_seed(5)
    with torch.no_grad():
        _, _, _, mask = m(x, lengths, generator=g)
    negatives = pretrain.sample_negatives(mask, 10, g)
    T2 = mask.shape[1]
    noise = -torch.empty(2 * T2, 2, 8, device=dev).exponential_(generator=g).log()
    opt = torch.optim.Adam(m.parameters(), lr=2e-3)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        context, target, perplexity, _ = m(x, lengths, mask_indexes=mask, noise=noise)
        loss = crit.pretrain_loss(context, target, perplexity, mask, negatives=negatives, num_codevectors=16)
        loss.backward()
        opt.step()
        losses.append(float(loss))
    print("losses", losses)
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]
