"""The transducer on the MI355X (csrc/rnnt.hip, ConformerCriterion.rnnt_loss, model/transducer.py, decode.rnnt_greedy_decode)
against the float64 restatement of tests/rnnt_restatement.py.

The bars are the project's own for a lattice likelihood and its gradient (tests/test_ctc_nbest_gpu.py):
    |nll - ref| <= 1e-5 max(1, |ref|)        and, per utterance,        ||dlogits - ref||_2 <= 1e-4 ||terms summed||_2
the second against gamma softmax + eb + el, the sizes of the terms the gradient sums (they cancel: every row of it sums to zero).
The joint and the model's logits meet the per-module bar, rel-L2 <= 2e-5 against float64."""
import math

import pytest
import torch

from conformer_amd import ops
from conformer_amd.autograd import RnntJointFn, RnntLossFn
from conformer_amd.decode import rnnt_greedy_decode
from conformer_amd.evaluation import ConformerCriterion
from tests import rnnt_restatement as R
from tests.test_write_guard_gpu import guarded_allocations
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
LL_TOL, GRAD_TOL, MODULE_TOL = 1e-5, 1e-4, 2e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


_CASES = {}


def case(B, T, U1, V, blank, in_len, tg_len, seed=0):
    """seeded logits and targets with their restatement, computed once and never changed"""
    key = (B, T, U1, V, blank, tuple(in_len), tuple(tg_len), seed)
    if key not in _CASES:
        g = torch.Generator().manual_seed(1000 * seed + 7 * V + T + U1)
        logits = torch.randn(B, T, U1, V, generator=g)
        targets = torch.randint(0, V, (B, U1 - 1), generator=g) if U1 > 1 else None
        if U1 > 2:
            targets[0, 1] = blank                                    # a label equal to blank
        nll, grad, terms = R.loss_and_grad(logits.double(), targets, in_len, tg_len, blank)
        _CASES[key] = dict(logits=logits, targets=targets, in_len=list(in_len), tg_len=list(tg_len), blank=blank, nll=nll,
                           grad=grad, terms=terms)
    return _CASES[key]


def on_device(c, dev):
    tg = None if c["targets"] is None else c["targets"].to(dev)
    return (c["logits"].to(dev), tg, torch.tensor(c["in_len"], dtype=torch.int64, device=dev),
            torch.tensor(c["tg_len"], dtype=torch.int64, device=dev))


def assert_nll(got, ref):
    got = got.cpu()
    assert got.dtype == torch.float64 and got.shape == ref.shape
    assert torch.equal(torch.isfinite(got), torch.isfinite(ref)), (got, ref)
    dead = ~torch.isfinite(ref)
    assert bool((got[dead] == math.inf).all())
    err = (got - ref)[~dead].abs()
    bar = LL_TOL * ref[~dead].abs().clamp_min(1.0)
    print("nll: max err", float(err.max()), "max err / bar", float((err / bar).max()))
    assert bool((err <= bar).all()), (err, bar)


def assert_grad(got, c, weight, what=""):
    """per utterance, against the size of the terms summed; exact zeros outside the live lattice"""
    got = got.double().cpu()
    T, U1 = got.shape[1:3]
    for b in range(got.shape[0]):
        w = float(weight[b])
        ref, size = w * c["grad"][b], abs(w) * float(c["terms"][b].norm())
        err = float((got[b] - ref).norm())
        print(f"grad {what} utterance {b}: err {err:.3e} terms {size:.3e} ratio {err / size if size else 0.0:.3e}")
        if size == 0.0:
            assert float(got[b].abs().max()) == 0.0
        else:
            assert err <= GRAD_TOL * size, (b, err, size)
        Tb, Ub = R.clamp(c["in_len"][b], 0, T), R.clamp(c["tg_len"][b], 0, U1 - 1)
        assert float(got[b, Tb:].abs().sum()) == 0.0 and float(got[b, :, Ub + 1:].abs().sum()) == 0.0


def run(c, dev, weight):
    x, tg, il, tl = on_device(c, dev)
    nll, ctx = ops.rnnt_loss_forward(x, tg, il, tl, c["blank"])
    d = ops.rnnt_loss_backward(ctx, weight.to(dev))
    assert d.dtype == torch.float32 and d.shape == x.shape
    return nll, d, ctx


@pytest.mark.parametrize("last_blank", [False, True])
@pytest.mark.parametrize("V", [29, 131])
def test_loss_and_gradient_against_the_restatement(dev, V, last_blank):
    c = case(3, 37, 12, V, V - 1 if last_blank else 0, (37, 20, 1), (11, 5, 3))
    w = torch.tensor([0.7, -1.3, 2.0])
    nll, d, ctx = run(c, dev, w)
    assert_nll(nll, c["nll"])
    assert_grad(d, c, w, f"V={V}")
    assert all(float(d[b].abs().max()) > 0 for b in range(3))
    w0 = torch.tensor([0.7, 0.0, 2.0])                              # a zero weight: an all-zero utterance, the others unchanged
    d0 = ops.rnnt_loss_backward(ctx, w0.to(dev))
    assert float(d0[1].abs().max()) == 0.0 and torch.equal(d0[0], d[0]) and torch.equal(d0[2], d[2])


def test_edges(dev):
    # in_len = 0 beside a live utterance
    c = case(2, 6, 4, 11, 0, (0, 6), (2, 3), seed=1)
    w = torch.tensor([5.0, 1.0])
    nll, d, _ = run(c, dev, w)
    assert float(nll[0]) == math.inf
    assert_nll(nll, c["nll"])
    assert_grad(d, c, w, "dead beside live")
    assert float(d[0].abs().max()) == 0.0
    x, tg, il, tl = on_device(c, dev)
    xg = x.clone().requires_grad_(True)
    crit = ConformerCriterion(0)
    loss = crit.rnnt_loss(xg, tg, il, tl)
    assert loss.dtype == torch.float64 and abs(float(loss.detach()) - float(c["nll"][1]) / 2) <= LL_TOL * max(1.0, float(c["nll"][1]) / 2)
    loss.backward()
    assert bool(torch.isfinite(xg.grad).all()) and float(xg.grad[0].abs().max()) == 0.0
    assert_grad(xg.grad, c, torch.tensor([0.0, 0.5]), "criterion mean")
    assert abs(float(crit.rnnt_loss(x, tg, il, tl, "sum")) - float(c["nll"][1])) <= LL_TOL * max(1.0, float(c["nll"][1]))
    assert torch.equal(crit.rnnt_loss(x, tg, il, tl, "none"), nll)
    assert crit.rnnt_loss(x.half(), tg, il, tl, "none").dtype == torch.float64          # any float dtype, computed in fp32
    # U1 = 1 with null targets: blanks only
    g = torch.Generator().manual_seed(5)
    x1 = torch.randn(2, 9, 1, 13, generator=g).to(dev)
    il1, tl1 = torch.tensor([9, 4], device=dev), torch.tensor([0, 0], device=dev)
    nll1, ctx1 = ops.rnnt_loss_forward(x1, None, il1, tl1, 3)
    lp = torch.log_softmax(x1.double(), -1)[:, :, 0, 3]
    ref1 = torch.stack([-lp[0].sum(), -lp[1, :4].sum()])
    assert bool(((nll1 - ref1).abs() <= LL_TOL * ref1.abs().clamp_min(1.0)).all()), (nll1, ref1)
    c1 = dict(in_len=[9, 4], tg_len=[0, 0])
    c1["nll"], c1["grad"], c1["terms"] = R.loss_and_grad(x1.double().cpu(), None, [9, 4], [0, 0], 3)
    assert_grad(ops.rnnt_loss_backward(ctx1, torch.ones(2, device=dev)), c1, torch.ones(2), "U1=1")
    # T = 1
    cT = case(2, 1, 4, 11, 2, (1, 1), (3, 0), seed=2)
    wT = torch.tensor([1.0, -1.0])
    nllT, dT, _ = run(cT, dev, wT)
    assert_nll(nllT, cT["nll"])
    assert_grad(dT, cT, wT, "T=1")


def test_logits_that_are_not_finite(dev):
    """a column of -inf is a column of probability 0; a live row without a finite log-sum-exp (a NaN, all -inf) makes its own
    utterance's nll not finite and its gradient zero, and changes no bit of the utterance beside it"""
    B, T, U1, V = 2, 6, 4, 12
    g = torch.Generator().manual_seed(17)
    x = torch.randn(B, T, U1, V, generator=g)
    x[..., 5] = -math.inf
    targets = torch.tensor([[1, 7, 3], [9, 2, 2]])
    c = dict(in_len=[6, 5], tg_len=[3, 2])
    c["nll"], c["grad"], c["terms"] = R.loss_and_grad(x.double(), targets, c["in_len"], c["tg_len"], 0)
    assert bool(torch.isfinite(c["nll"]).all()) and bool(torch.isfinite(c["grad"]).all())
    il, tl, w = torch.tensor(c["in_len"], device=dev), torch.tensor(c["tg_len"], device=dev), torch.tensor([1.0, -2.0])
    nll, ctx = ops.rnnt_loss_forward(x.to(dev), targets.to(dev), il, tl, 0)
    d = ops.rnnt_loss_backward(ctx, w.to(dev))
    assert_nll(nll, c["nll"])
    assert_grad(d, c, w, "-inf column")
    assert float(d[..., 5].abs().max()) == 0.0
    for bad in (math.nan, -math.inf):
        y = x.clone()
        if bad != bad:
            y[1, 2, 1, 3] = bad                                             # one NaN in a live row
        else:
            y[1, 2, 1] = bad                                                # a live row of -inf only
        nll2, ctx2 = ops.rnnt_loss_forward(y.to(dev), targets.to(dev), il, tl, 0)
        d2 = ops.rnnt_loss_backward(ctx2, w.to(dev))
        assert not math.isfinite(float(nll2[1])) and float(d2[1].abs().max()) == 0.0 and not bool(torch.isnan(d2).any())
        assert torch.equal(nll2[0], nll[0]) and torch.equal(d2[0], d[0])
        mean = ConformerCriterion(0).rnnt_loss(y.to(dev), targets.to(dev), il, tl)
        assert float(mean) == float(nll[0]) / 2


WIDTHS = ([(5, U1, 7) for U1 in (64, 65, 129)] + [(T, 3, 7) for T in (1, 2, 65)] + [(3, 3, V) for V in (2, 63, 132, 4099)])


@pytest.mark.parametrize("T,U1,V", WIDTHS)
def test_widths(dev, T, U1, V):
    """lattice workgroups of one, two and three waves; one, two and many anti-diagonals; rows narrower than a lane group, not a
    multiple of four (scalar loads), a multiple of four (16-byte loads) and wider than anything held at once"""
    c = case(2, T, U1, V, V // 2, (T, max(1, T - 1)), (U1 - 1, (U1 - 1) // 2), seed=3)
    w = torch.tensor([1.0, -0.6])
    nll, d, _ = run(c, dev, w)
    assert_nll(nll, c["nll"])
    assert_grad(d, c, w, f"T={T} U1={U1} V={V}")


def test_two_runs_give_the_same_bits(dev):
    c = case(3, 37, 12, 131, 0, (37, 20, 1), (11, 5, 3))
    w = torch.tensor([0.7, -1.3, 2.0])
    nll, d, _ = run(c, dev, w)
    nll2, d2, _ = run(c, dev, w)
    assert torch.equal(nll, nll2) and torch.equal(d, d2)
    c4 = case(2, 3, 3, 132, 66, (3, 2), (2, 1), seed=3)
    a, b = run(c4, dev, torch.ones(2)), run(c4, dev, torch.ones(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_writes_stay_inside_their_buffers(dev):
    c = case(3, 37, 12, 131, 0, (37, 20, 1), (11, 5, 3))
    x, tg, il, tl = on_device(c, dev)
    w = torch.tensor([0.7, -1.3, 2.0], device=dev)
    g = torch.Generator().manual_seed(9)
    e, p, dh = (torch.randn(*s, generator=g).to(dev) for s in ((2, 5, 36), (2, 4, 36), (2, 5, 4, 36)))
    z = torch.randn(3, 29, generator=g).to(dev)
    with guarded_allocations() as gt:
        nll, ctx = ops.rnnt_loss_forward(x, tg, il, tl, 0)                  # nll and the workspace
        d = ops.rnnt_loss_backward(ctx, w)                                  # dlogits
        h = ops.rnnt_joint_forward(e, p)
        de, dp = ops.rnnt_joint_backward(h, dh)
        h1 = ops.rnnt_joint_forward(e, p, torch.tensor([9, -1], device=dev))
        tokens, frames = gt.full((3, 46), -1, dtype=torch.int64, device=dev), gt.full((3, 46), -1, dtype=torch.int64, device=dev)
        count, last, t, nsym = (gt.zeros(3, dtype=torch.int64, device=dev) for _ in range(4))
        emit, active = gt.zeros(3, dtype=torch.int32, device=dev), gt.zeros(1, dtype=torch.int32, device=dev)
        new, cur = gt.full((4, 3, 16), 1.0, dtype=torch.float32, device=dev), gt.zeros(4, 3, 16, dtype=torch.float32, device=dev)
        t[2] = 23                                                           # a finished row
        ops.rnnt_greedy_decide(z, torch.tensor([23, 15, 23], device=dev), 23, 0, 2, tokens, frames, count, last, t, nsym, emit)
        ops.rnnt_greedy_commit(new, cur, emit, t, torch.tensor([23, 15, 23], device=dev), 23, active)
        bad, n = gt.check(), len(gt.allocs)
    assert n >= 17 and not bad, bad
    assert_nll(nll, c["nll"])
    assert int(active) == 2 and int(emit[2]) == 0 and int(t[2]) == 23 and float(cur[:, 2].abs().max()) == 0.0
    k = z.argmax(-1)
    for b in range(2):
        if int(k[b]) != 0:
            assert int(emit[b]) == 1 and int(tokens[b, 0]) == int(k[b]) and int(frames[b, 0]) == 0 and int(count[b]) == 1
            assert int(last[b]) == int(k[b]) and int(t[b]) == 0 and float(cur[:, b].min()) == 1.0
        else:
            assert int(emit[b]) == 0 and int(t[b]) == 1 and int(count[b]) == 0 and float(cur[:, b].abs().max()) == 0.0


@pytest.mark.parametrize("J", [7, 8, 36, 132, 640])
def test_joint_against_float64(dev, J):
    B, T, U1 = 2, 5, 4
    g = torch.Generator().manual_seed(J)
    e, p, dh = torch.randn(B, T, J, generator=g), torch.randn(B, U1, J, generator=g), torch.randn(B, T, U1, J, generator=g)
    e64, p64 = e.double().requires_grad_(True), p.double().requires_grad_(True)
    h64 = torch.tanh(e64[:, :, None] + p64[:, None])
    h64.backward(dh.double())
    eg, pg = e.to(dev).requires_grad_(True), p.to(dev).requires_grad_(True)
    h = RnntJointFn.apply(eg, pg)
    assert h.dtype == torch.float32 and h.shape == (B, T, U1, J)
    h.backward(dh.to(dev))
    errs = rel_l2(h, h64), rel_l2(eg.grad, e64.grad), rel_l2(pg.grad, p64.grad)
    print(f"joint J={J}: rel-L2 h {errs[0]:.2e} de {errs[1]:.2e} dp {errs[2]:.2e}")
    assert max(errs) <= MODULE_TOL
    de, dp = ops.rnnt_joint_backward(h.detach(), dh.to(dev))
    assert torch.equal(de, eg.grad) and torch.equal(dp, pg.grad)             # fixed summation orders
    frames = torch.tensor([3, 7], device=dev)                               # 7 clamps to the last frame
    hf = ops.rnnt_joint_forward(e.to(dev), p.to(dev), frames)
    assert hf.shape == (B, 1, U1, J)
    assert torch.equal(hf[0, 0], h[0, 3].detach()) and torch.equal(hf[1, 0], h[1, 4].detach())
    low = ops.rnnt_joint_forward(e.to(dev), p.to(dev), torch.tensor([-5, 0], device=dev))    # -5 clamps to the first
    assert torch.equal(low[0, 0], h[0, 0].detach()) and torch.equal(low[1, 0], h[1, 0].detach())


def tiny_model(dev):
    from model.conformer import Conformer
    from model.transducer import ConformerTransducer
    torch.manual_seed(21)
    m = ConformerTransducer(29, n_mel_channels=80, n_conformer_blocks=2, d_model=32, n_heads=4, kernel_size=31, pred_hidden_dim=24,
                            n_pred_layers=2, joint_dim=20, blank_id=0)
    ctc = Conformer(29, 80, 2, 32, 4, 31, 24, 1, 0.0)
    enc = {k: v for k, v in ctc.state_dict().items() if k.startswith("encoder.")}
    missing, unexpected = m.load_state_dict(enc, strict=False)
    assert not unexpected and not [k for k in missing if k.startswith("encoder.")]
    assert all(torch.equal(v, m.state_dict()[k]) for k, v in enc.items())
    g = torch.Generator().manual_seed(22)
    x = torch.randn(3, 80, 103, generator=g).to(dev)
    lengths = torch.tensor([103, 80, 31], device=dev)
    targets = torch.randint(1, 29, (3, 5), generator=g)
    return m.to(dev), x, lengths, targets, torch.tensor([5, 3, 0])


def test_model_against_the_restatement(dev):
    m, x, lengths, targets, tg_len = tiny_model(dev)
    m.train()
    seen = []
    hook = m.encoder.register_forward_hook(lambda mod, args, out: seen.append(out[0]))
    logits, out_len = m(x, lengths, targets.to(dev), tg_len.to(dev))
    hook.remove()
    (enc,) = seen                                                           # the encoder output this very forward used
    B, T, U1, V = logits.shape
    assert (B, U1, V) == (3, 6, 29) and logits.dtype == torch.float32 and int(out_len[0]) == T and int(out_len[2]) < T
    loss = ConformerCriterion(0).rnnt_loss(logits, targets.to(dev), out_len, tg_len.to(dev))
    loss.backward()
    # the restatement, fed the HIP encoder's own output, as leaves of a float64 autograd graph
    heads = {k: v.detach().double().cpu().requires_grad_(True) for k, v in m.state_dict().items()
             if k.startswith(("predictor.", "joiner."))}
    H = R.Heads(heads, 0, as_given=True)
    enc64, total = enc.detach().double().cpu(), 0.0
    for b in range(B):
        Tb, Ub = int(out_len[b]), int(tg_len[b])
        y = targets[b, :Ub].tolist()
        ref = H.logits(enc64[b], H.predictor(y, Ub))                        # (T, Ub + 1, V)
        r = rel_l2(logits[b, :, :Ub + 1], ref)
        print(f"model logits utterance {b}: rel-L2 {r:.2e}")
        assert r <= MODULE_TOL
        total = total + -R.ll_autograd(ref, y, Tb, Ub, 0)
    ref_loss = total / B
    print("model loss", float(loss.detach()), "ref", float(ref_loss.detach()))
    assert abs(float(loss.detach()) - float(ref_loss.detach())) <= LL_TOL * max(1.0, abs(float(ref_loss.detach())))
    ref_loss.backward()
    for k, ref in heads.items():
        p = dict(m.named_parameters())[k]
        r = rel_l2(p.grad, ref.grad)
        print(f"grad {k}: rel-L2 {r:.2e}")
        assert r <= 1e-4, k
    for k, p in m.encoder.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k


def test_greedy_against_the_restatement(dev):
    from model.modules.transducer import Joiner, Predictor
    s = R.GREEDY_SHAPE
    sd, enc = R.greedy_fixture()
    heads = torch.nn.Module()
    heads.predictor = Predictor(s["V"], s["H"], s["n_layers"], s["blank"])
    heads.joiner = Joiner(s["d"], s["H"], s["J"], s["V"])
    heads.load_state_dict(sd, strict=True)
    heads = heads.to(dev)
    ref = R.greedy_reference()
    in_len = torch.tensor(s["in_len"], device=dev)
    cap = s["T"] * s["max_symbols"]
    outs = [rnnt_greedy_decode(heads.predictor, heads.joiner, enc.to(dev), in_len, s["max_symbols"], sync_every=k) for k in (1, 7)]
    for tokens, counts, frames in outs:
        assert tokens.shape == frames.shape == (s["B"], cap) and tokens.dtype == frames.dtype == counts.dtype == torch.int64
        for b in range(s["B"]):
            n = len(ref[b][0])
            assert int(counts[b]) == n and tokens[b, :n].tolist() == ref[b][0] and frames[b, :n].tolist() == ref[b][1], b
            assert bool((tokens[b, n:] == -1).all()) and bool((frames[b, n:] == -1).all())
    assert all(torch.equal(a, b) for a, b in zip(*outs))


def test_model_greedy_is_the_decode_of_its_encoder_output(dev):
    m, x, lengths, _, _ = tiny_model(dev)
    m.eval()
    tokens, counts, frames = m.greedy(x, lengths, max_symbols=3)
    with torch.no_grad():
        enc, out_len = m.encoder(x, lengths)
    ref = rnnt_greedy_decode(m.predictor, m.joiner, enc, out_len, 3)
    assert tokens.shape == (3, enc.shape[1] * 3)
    assert torch.equal(tokens, ref[0]) and torch.equal(counts, ref[1]) and torch.equal(frames, ref[2])
    assert bool((counts <= out_len * 3).all())
    assert RnntLossFn.apply(torch.zeros(1, 2, 1, 4, device=dev), None, torch.tensor([2], device=dev), torch.tensor([0], device=dev),
                            0).dtype == torch.float64
