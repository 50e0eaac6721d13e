"""The n-best CTC scores, their gradient and the MWER loss on the MI355X (csrc/ctc_nbest.hip, ConformerCriterion.mwer_loss,
decode.ctc_nbest_scores / nbest_posterior) against the float64 restatement of tests/ctc_nbest_restatement.py.  The lists are
built by hand, so nothing depends on what a search happens to return.

The bars are the project's own for this lattice (an fp32 lattice re-centred into float64 offsets):
    |ll - ref| <= 1e-5 max(1, |ref|)        and        ||grad - ref||_2 <= 1e-4 || sum_n |w_n| |d ll_n / d logits| ||_2
the second against the size of the terms summed, not of the cancelled sum: MWER weights sum to zero and the rows of a list share
most of their alignment mass."""
import math

import pytest
import torch

from conformer_amd import ops
from conformer_amd.autograd import CtcNbestScoreFn
from conformer_amd.decode import BeamCTCDecoder, beam_ctc_decode, ctc_nbest_scores, nbest_posterior
from conformer_amd.error_rate import ErrorRateTables
from conformer_amd.evaluation import ConformerCriterion
from tests import ctc_nbest_restatement as R
from tests import error_rate_restatement as E
from tests.test_write_guard_gpu import guarded_allocations
from tests.util import rel_l2

pytestmark = pytest.mark.gpu
LL_TOL, GRAD_TOL = 1e-5, 1e-4


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def vocab_of(V):
    return ["<pad>"] + [chr(ord("a") + i) for i in range(V - 3)] + ["|", "<unk>"]


_CASES = {}


def case(V):
    """The hand-built list at vocabulary V with its restatement, computed once and never changed"""
    if V not in _CASES:
        g = torch.Generator().manual_seed(100 + V)
        logits = torch.randn(3, 37, V, generator=g)
        hyps, hyp_len, in_len = R.hand_built(V)
        ll, dll = R.scores(logits.double(), hyps, hyp_len, in_len, 0)
        _CASES[V] = dict(logits=logits, hyps=hyps, hyp_len=hyp_len, in_len=in_len, ll=ll, dll=dll)
    return _CASES[V]


def on_device(c, dev, width=None):
    tk, hl = R.padded(c["hyps"], c["hyp_len"], width)
    return c["logits"].to(dev), tk.to(dev), hl.to(dev), torch.tensor(c["in_len"], dtype=torch.int64, device=dev)


def assert_ll(got, ref):
    got = got.cpu()
    assert got.dtype == torch.float64 and got.shape == ref.shape
    assert torch.equal(torch.isfinite(got), torch.isfinite(ref)), (got, ref)
    dead = ~torch.isfinite(ref)
    assert bool((got[dead] == -math.inf).all())
    err = (got - ref)[~dead].abs()
    bar = LL_TOL * ref[~dead].abs().clamp_min(1.0)
    print("ll: max err", float(err.max()), "max err / bar", float((err / bar).max()))
    assert bool((err <= bar).all()), (err, bar)


def assert_grad(got, dll, weight, what=""):
    """per utterance, against the size of the terms summed"""
    ref, terms = R.weighted_grad(dll, weight.cpu())
    got = got.double().cpu()
    for b in range(ref.shape[0]):
        size = float(terms[b].norm())
        err = float((got[b] - ref[b]).norm())
        print(f"grad {what} utterance {b}: err {err:.3e} terms {size:.3e} ratio {err / size if size else 0.0:.3e}")
        if size == 0.0:
            assert float(got[b].abs().max()) == 0.0
        else:
            assert err <= GRAD_TOL * size, (b, err, size)


def weights_for(ll, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(ll.shape, generator=g)
    w[0, 2] = 0.0                                   # one zero weight
    return w


@pytest.mark.parametrize("V", [29, 131])
def test_scores_and_gradient_against_the_restatement(dev, V):
    c = case(V)
    x, tk, hl, il = on_device(c, dev)
    ll, ctx = ops.ctc_nbest_forward(x, tk, hl, il, 0)
    assert_ll(ll, c["ll"])
    w = weights_for(c["ll"], 5)
    w[2, 1] = 3.0                                   # the infeasible row: its weight must not count
    d = ops.ctc_nbest_backward(ctx, w.to(dev))
    assert d.dtype == torch.float32 and d.shape == x.shape
    assert_grad(d, c["dll"], w, f"V={V}")
    assert float(d[1, 20:].abs().max()) == 0.0 and float(d[2, 1:].abs().max()) == 0.0        # at or behind in_len
    assert float(d[0].abs().max()) > 0 and float(d[2, 0].abs().max()) > 0
    w0 = w.clone()
    w0[2, 1] = 0.0
    assert torch.equal(ops.ctc_nbest_backward(ctx, w0.to(dev)), d)                          # the infeasible row's contribution
    w1 = w.clone()
    w1[1] = 0.0                                     # an utterance with all weights zero
    w1[1, 3] = 2.0                                  # ... but for the unused row
    d1 = ops.ctc_nbest_backward(ctx, w1.to(dev))
    assert float(d1[1].abs().max()) == 0.0 and torch.equal(d1[0], d[0]) and torch.equal(d1[2], d[2])
    # weights that sum to zero per utterance, as MWER's do: the bar is against the terms, the sum cancels
    w0[1, 3] = 0.0                                  # the unused row
    wz = w0 - w0.sum(1, keepdim=True) * torch.tensor([[0, 1.0, 0, 0], [1.0, 0, 0, 0], [1.0, 0, 0, 0]])
    assert_grad(ops.ctc_nbest_backward(ctx, wz.to(dev)), c["dll"], wz, f"V={V} zero-sum")


def test_an_utterance_of_infeasible_rows_only(dev):
    c = case(29)
    hyps = [c["hyps"][0], c["hyps"][1], [[4, 5], [4, 4], [6, 7, 8], [9]]]
    hyp_len = [c["hyp_len"][0], c["hyp_len"][1], [2, 2, 3, -1]]
    tk, hl = R.padded(hyps, hyp_len)
    x, il = c["logits"].to(dev), torch.tensor(c["in_len"], device=dev)
    ll, ctx = ops.ctc_nbest_forward(x, tk.to(dev), hl.to(dev), il, 0)
    assert bool((ll[2] == -math.inf).all())
    assert_ll(ll[:2], c["ll"][:2])
    w = weights_for(c["ll"], 6)
    d = ops.ctc_nbest_backward(ctx, w.to(dev))
    assert float(d[2].abs().max()) == 0.0
    assert_grad(d[:2], c["dll"][:2], w[:2], "infeasible utterance beside")


def test_zero_frames_and_padding_beyond_the_lattice(dev):
    """in_len = 0: the empty row scores 0, every other -inf, no gradient; rows handed in wider than max_len are cut to it"""
    c = case(29)
    x, tk, hl, il = on_device(c, dev, width=11)
    zero = torch.tensor([37, 0, 1], device=dev)
    ll = ctc_nbest_scores(x, tk, hl.clamp_min(0), 0, zero, max_len=6)
    assert ll[1].tolist() == [-math.inf, -math.inf, -math.inf, 0.0]                        # hyp_len -1 clamped to the empty row
    ll, ctx = ops.ctc_nbest_forward(x, tk, hl, il, 0, max_len=6)
    assert ctx[1].shape[2] == 6
    assert_ll(ll, c["ll"])
    ll11, _ = ops.ctc_nbest_forward(x, tk, hl, il, 0)
    assert torch.equal(ll11, ll)                                                           # the lattice width changes no bit here


@pytest.mark.parametrize("Lmax", [63, 64, 128])
def test_lattice_widths(dev, Lmax):
    """pairs per lane 1, 2 and 4: T = 2 Lmax + 5 frames, one row of Lmax labels (with repeats) and a shorter one"""
    V, T = 17, 2 * Lmax + 5
    g = torch.Generator().manual_seed(Lmax)
    logits = torch.randn(1, T, V, generator=g)
    full = torch.randint(1, V, (Lmax,), generator=g).tolist()
    full[10] = full[9]
    full[-1] = full[-2]
    hyps, hyp_len = [[full, full[3:Lmax - 2]]], [[Lmax, Lmax - 5]]
    ll_ref, dll = R.scores(logits.double(), hyps, hyp_len, [T], 0)
    assert bool(torch.isfinite(ll_ref).all())
    tk, hl = R.padded(hyps, hyp_len)
    ll, ctx = ops.ctc_nbest_forward(logits.to(dev), tk.to(dev), hl.to(dev), torch.tensor([T], device=dev), 0)
    assert ctx[4] == Lmax
    assert_ll(ll, ll_ref)
    w = torch.tensor([[0.7, -0.4]])
    assert_grad(ops.ctc_nbest_backward(ctx, w.to(dev)), dll, w, f"Lmax={Lmax}")


def test_one_row_with_the_loss_weights_is_the_ctc_loss_gradient(dev):
    c = case(29)
    x, il = c["logits"].to(dev), torch.tensor(c["in_len"], device=dev)
    rows = [[2, 2, 2, 3], [5, 7, 9, 11, 4, 6], []]
    tk, hl = R.padded([[r] for r in rows], [[len(r)] for r in rows])
    lens = torch.tensor([len(r) for r in rows], device=dev)
    xg = x.clone().requires_grad_(True)
    ConformerCriterion(0).ctc_loss(xg, tk[:, 0].to(dev), il, lens).backward()
    ll, ctx = ops.ctc_nbest_forward(x, tk.to(dev), hl.to(dev), il, 0)
    w = (1.0 / (3 * lens.clamp_min(1).float()))[:, None]
    d = ops.ctc_nbest_backward(ctx, w)                       # d (sum_b ll_b / (B L_b)) / d logits = -d loss / d logits
    r = rel_l2(-d, xg.grad)
    print("N = 1 against ctc_loss: rel-L2", r)
    assert r < 1e-6


def test_determinism_and_the_repeat_interleave_route(dev):
    c = case(131)
    x, tk, hl, il = on_device(c, dev)
    w = weights_for(c["ll"], 7).to(dev)
    ll, ctx = ops.ctc_nbest_forward(x, tk, hl, il, 0)
    d = ops.ctc_nbest_backward(ctx, w)
    ll2, ctx2 = ops.ctc_nbest_forward(x, tk, hl, il, 0)
    d2 = ops.ctc_nbest_backward(ctx2, w)
    assert torch.equal(ll, ll2) and torch.equal(d, d2)
    # the parent's route: N copies of the logits through the loss entries, one utterance per row
    B, N = hl.shape
    xr = x.repeat_interleave(N, 0)
    _, state = ops.ctc_loss_forward(xr, tk.reshape(B * N, -1).clamp_min(0), il.repeat_interleave(N), hl.reshape(-1).clamp_min(0), 0)
    ll_r = -ops.ctc_nll(state).double().reshape(B, N).cpu()
    used = torch.tensor(c["hyp_len"]) >= 0
    ref = c["ll"]
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isfinite(ll_r) & used, fin)
    assert bool(((ll_r - ll.cpu())[fin].abs() <= 2 * LL_TOL * ref[fin].abs().clamp_min(1.0)).all())
    dr = ops.ctc_loss_backward(state, torch.ones((), device=dev))               # (softmax - occupancy) / (B N max(L, 1)) per row
    scale = -(B * N) * hl.reshape(-1).clamp_min(1).double()
    live = (used & fin).reshape(-1).to(dev)
    dll_r = (dr.double() * scale[:, None, None] * live[:, None, None]).reshape(B, N, *x.shape[1:]).cpu()
    assert_grad(d, dll_r, w, "repeat-interleave route")


def test_no_expanded_tensor(dev):
    B, N, T, V, L = 2, 8, 64, 4096, 20
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, T, V, generator=g).to(dev)
    tk = torch.randint(1, V, (B, N, L), generator=g).to(dev)
    hl = torch.randint(10, L + 1, (B, N), generator=g).to(dev)
    il = torch.tensor([T, T - 9], device=dev)
    w = torch.randn(B, N, generator=g).to(dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ll, ctx = ops.ctc_nbest_forward(x, tk, hl, il, 0)
    d = ops.ctc_nbest_backward(ctx, w)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print("rise", rise, "expanded", B * N * T * V * 4)
    assert rise < B * N * T * V * 4 // 2
    assert bool(torch.isfinite(ll).all()) and bool(torch.isfinite(d).all()) and float(d.abs().max()) > 0


def test_writes_stay_inside_their_buffers(dev):
    c = case(131)
    x, tk, hl, il = on_device(c, dev, width=9)
    w = weights_for(c["ll"], 8).to(dev)
    errors = torch.randint(0, 5, hl.shape, dtype=torch.int32).to(dev)
    with guarded_allocations() as gt:
        ll, ctx = ops.ctc_nbest_forward(x, tk, hl, il, 0, max_len=6)        # dlogits, ll, weight and the workspace are guarded
        d = ops.ctc_nbest_backward(ctx, w)
        loss, weight, risk = ops.mwer_risk(ll, errors, hl)
        bad, n = gt.check(), len(gt.allocs)
    assert n >= 7 and not bad, bad
    assert_ll(ll, c["ll"])


# ---- the loss ---------------------------------------------------------------------------------------------------------------------

def references(V):
    """targets (B, Lr) and their lengths for the hand-built list, chosen so that the rows of every list differ in their word
    and character errors; utterance 1's is row 0 of its list"""
    refs = [[2, 2, 2, 3, V - 2, 5, 7], [5, 7, 9, 11, 4, 6], [4, V - 2, 7]]
    lens = [len(r) for r in refs]
    t = torch.zeros(3, 7, dtype=torch.int64)
    for b, r in enumerate(refs):
        t[b, :len(r)] = torch.tensor(r)
    return refs, t, torch.tensor(lens)


def restated_errors(c, V, refs, unit):
    kinds, cps = E.tables(vocab_of(V), "|", (0, V - 1))
    return [[E.counts(h, max(n, 0), refs[b], len(refs[b]), kinds, cps, unit)[0] for h, n in zip(c["hyps"][b], c["hyp_len"][b])]
            for b in range(3)]


@pytest.mark.parametrize("unit", ["word", "char"])
def test_mwer_loss_on_the_hand_built_list(dev, unit):
    V = 29
    c = case(V)
    x, tk, hl, il = on_device(c, dev)
    refs, targets, tlen = references(V)
    tables = ErrorRateTables(vocab_of(V), "|", (0, V - 1))
    errors = restated_errors(c, V, refs, unit)
    assert all(len({e for e, n in zip(row, used) if n >= 0}) > 1 for row, used in zip(errors, c["hyp_len"])), errors
    loss_ref, w_ref, risk_ref, spread = R.risk_weights(c["ll"], errors, c["hyp_len"])
    assert float(w_ref.abs().max()) > 1e-3
    delta = LL_TOL * max(1.0, float(c["ll"][torch.isfinite(c["ll"])].abs().max()))
    xg = x.clone().requires_grad_(True)
    num = torch.tensor([4, 3, 4], device=dev)                          # utterance 1: row 3 unused
    loss = ConformerCriterion(0).mwer_loss(xg, targets.to(dev), il, tlen.to(dev), tables, unit=unit, hyp_tokens=tk,
                                           hyp_counts=hl.clamp_min(0), num_hyps=num)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    loss.backward()
    # the risk per utterance, from the entry itself on the device's own scores
    ll = ctc_nbest_scores(x, tk, hl.clamp_min(0), 0, il, num)
    err_dev = torch.tensor(errors, dtype=torch.int32, device=dev)
    _, weight, risk = ops.mwer_risk(ll, err_dev, hl)
    gap = (risk.double().cpu() - risk_ref).abs()
    print("risk", risk.tolist(), "ref", risk_ref.tolist(), "gap", gap.tolist(), "bound", (2 * delta * spread).tolist())
    assert bool((gap <= 2 * delta * spread).all())
    assert abs(float(loss.detach()) - float(loss_ref)) <= float((2 * delta * spread).mean())
    assert float(weight.sum(1).abs().max()) <= 1e-6 and float(weight[1, 3]) == 0.0 and float(weight[2, 1]) == 0.0
    assert_grad(xg.grad, c["dll"], w_ref, f"mwer {unit}")


def test_mwer_loss_variants(dev):
    """n_best = 1; add_reference with the reference in the list and not in it; the CTC interpolation"""
    V = 29
    c = case(V)
    x, tk, hl, il = on_device(c, dev)
    refs, targets, tlen = references(V)
    targets, tlen = targets.to(dev), tlen.to(dev)
    tables = ErrorRateTables(vocab_of(V), "|", (0, V - 1))
    crit = ConformerCriterion(0)
    num = torch.tensor([4, 3, 4], device=dev)
    given = dict(hyp_tokens=tk, hyp_counts=hl.clamp_min(0), num_hyps=num)

    def run(targets=targets, tlen=tlen, **kw):
        xg = x.clone().requires_grad_(True)
        loss = crit.mwer_loss(xg, targets, il, tlen, tables, **kw)
        loss.backward()
        return loss.detach(), xg.grad

    base, g_base = run(**given)
    assert float(g_base.abs().max()) > 0
    one, g_one = run(n_best=1)                                          # the search inside, one hypothesis: nothing to rank
    assert float(one) == 0.0 and float(g_one.abs().max()) == 0.0
    # the reference is in every list: utterance 0's is made its row 1, utterance 2's its row 0
    tin = torch.zeros(3, 6, dtype=torch.int64)
    for b, r in enumerate([c["hyps"][0][1], c["hyps"][1][0], c["hyps"][2][0]]):
        tin[b, :len(r)] = torch.tensor(r)
    lin = torch.tensor([6, 6, 1], device=dev)
    a, g_a = run(tin.to(dev), lin, **given)
    b_, g_b = run(tin.to(dev), lin, add_reference=True, **given)
    assert torch.equal(a, b_) and torch.equal(g_a, g_b)
    # not in the list: the row is appended and counts, as if it had been handed in
    with_ref, g_with = run(add_reference=True, **given)
    wide = torch.full((3, 5, 7), -1, dtype=torch.int64, device=dev)
    wide[:, :4, :tk.shape[2]] = tk
    wide[:, 4] = targets
    for b in range(3):
        wide[b, 4, int(tlen[b]):] = -1
    hl5 = torch.cat([hl, tlen[:, None]], 1)
    hl5[1, 4] = -1                                                     # utterance 1's reference is its row 0
    explicit, g_explicit = run(hyp_tokens=wide, hyp_counts=hl5.clamp_min(0), num_hyps=torch.tensor([5, 3, 5], device=dev))
    assert torch.equal(with_ref, explicit) and torch.equal(g_with, g_explicit)
    ll5 = ctc_nbest_scores(x, wide, hl5, 0, il)
    assert bool(torch.isfinite(ll5[0, 4])) and float(ll5[1, 4]) == -math.inf          # appended and live; unused
    assert float(ll5[2, 4]) == -math.inf                                             # three labels at one frame: appended, infeasible
    assert not torch.equal(with_ref, base) and not torch.equal(g_with, g_base)
    # interpolation
    xg = x.clone().requires_grad_(True)
    ctc = crit.ctc_loss(xg, targets, il, tlen)
    ctc.backward()
    mixed, g_mixed = run(ctc_weight=0.3, **given)
    assert abs(float(mixed) - (float(base) + 0.3 * float(ctc))) <= 1e-6 * max(1.0, abs(float(mixed)))
    assert rel_l2(g_mixed, g_base + 0.3 * xg.grad) < 1e-6


def test_mwer_loss_with_the_search_inside(dev):
    B, T, V = 2, 20, 12
    g = torch.Generator().manual_seed(9)
    x = torch.randn(B, T, V, generator=g).to(dev)
    il = torch.tensor([20, 16], device=dev)
    tables = ErrorRateTables(vocab_of(V), "|", (0, V - 1))
    crit = ConformerCriterion(0)
    tokens, counts, _, num = beam_ctc_decode(x, 0, il, 100, 4)
    assert bool((num >= 4).all()), num                                  # every log-probability is near -2.5, above token_min_logp
    # the reference is the second hypothesis: the rows of a list then differ in their errors (against a random reference
    # every row of a random list is wrong in every word, the risk is flat and there is nothing to compare)
    targets, tlen = tokens[:, 1].clamp_min(0), counts[:, 1]
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    la = crit.mwer_loss(xa, targets, il, tlen, tables, n_best=4)
    lb = crit.mwer_loss(xb, targets, il, tlen, tables, hyp_tokens=tokens, hyp_counts=counts, num_hyps=num)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(xa.grad, xb.grad) and float(xa.grad.abs().max()) > 0
    # a decoder's own search: the same list at the same beam settings
    dec = BeamCTCDecoder(vocab_of(V), 0, skip_ids=(V - 1,), beam_width=100, beam_prune_logp=-10.0, token_min_logp=-5.0)
    xc = x.clone().requires_grad_(True)
    lc = crit.mwer_loss(xc, targets, il, tlen, tables, n_best=4, decoder=dec)
    lc.backward()
    assert torch.equal(lc, la) and torch.equal(xc.grad, xa.grad)


def test_mwer_loss_through_a_tiny_conformer(dev):
    from model.conformer import Conformer
    from oracle import conformer_oracle as O
    V = 12
    P = O.make_params(vocab=V, n_mel=80, n_blocks=1, d=32, n_heads=4, ksize=31, lstm_hidden=24, seed=5)
    m = Conformer(V, 80, 1, 32, 4, 31, 24, 1, 0.0)
    m.load_state_dict(P, strict=True)
    m = m.to(dev).train()
    g = torch.Generator().manual_seed(6)
    feats = torch.randn(2, 80, 120, generator=g).to(dev)
    logits, out_len = m(feats, torch.tensor([120, 90], device=dev))
    logits.retain_grad()
    tables = ErrorRateTables(vocab_of(V), "|", (0, V - 1))
    crit = ConformerCriterion(0)
    # wide beam settings: the list does not depend on how peaked this random model is
    dec = BeamCTCDecoder(vocab_of(V), 0, skip_ids=(V - 1,), beam_width=50, beam_prune_logp=-1e9, token_min_logp=-1e9)
    from conformer_amd import decode
    out = decode._beam_search(logits.detach().float(), 0, out_len, 4, dec.beam_width, dec.token_min_logp, dec.beam_prune_logp,
                              dec.max_candidates, dec.vocab, None)
    assert bool((out[-1] >= 2).all()), out[-1]
    targets, tlen = out[0][:, 1].clamp_min(0), out[1][:, 1]             # the reference: the second hypothesis (see above)
    loss = crit.mwer_loss(logits, targets, out_len, tlen, tables, n_best=4, decoder=dec)
    loss.backward()
    trained = [(name, p) for name, p in m.named_parameters() if p.requires_grad]      # all but the positional frequency table
    assert len(trained) >= len(list(m.parameters())) - 1
    for name, p in trained:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert any(float(p.grad.abs().max()) > 0 for _, p in trained)
    # the restatement, fed the model's own logits and list
    tokens, counts, num = out[0].cpu(), out[1].cpu(), out[-1].cpu()
    hyp_len = [[int(counts[b, n]) if n < int(num[b]) else -1 for n in range(4)] for b in range(2)]
    hyps = [[tokens[b, n, :max(hyp_len[b][n], 0)].tolist() for n in range(4)] for b in range(2)]
    x64 = logits.detach().double().cpu()
    ll, dll = R.scores(x64, hyps, hyp_len, out_len.cpu().tolist(), 0)
    kinds, cps = E.tables(vocab_of(V), "|", (0, V - 1))
    refs = targets.cpu().tolist()
    errors = [[E.counts(hyps[b][n], max(hyp_len[b][n], 0), refs[b], int(tlen[b]), kinds, cps, "word")[0] for n in range(4)]
              for b in range(2)]
    loss_ref, w_ref, _, spread = R.risk_weights(ll, errors, hyp_len)
    delta = LL_TOL * max(1.0, float(ll[torch.isfinite(ll)].abs().max()))
    assert abs(float(loss) - float(loss_ref)) <= float((2 * delta * spread).mean())
    assert_grad(logits.grad, dll, w_ref, "conformer")


def test_nbest_posterior(dev):
    c = case(29)
    x, tk, hl, il = on_device(c, dev)
    num = torch.tensor([4, 3, 4], device=dev)
    p = nbest_posterior(x, tk, hl.clamp_min(0), 0, il, num)
    assert p.dtype == torch.float32 and p.shape == (3, 4)
    ref = R.posterior(c["ll"], c["hyp_len"])
    delta = LL_TOL * max(1.0, float(c["ll"][torch.isfinite(c["ll"])].abs().max()))
    assert float((p.double().cpu() - ref).abs().max()) <= 2 * delta
    assert float((p.sum(1) - 1).abs().max()) <= 1e-6
    assert float(p[1, 3]) == 0.0 and float(p[2, 1]) == 0.0               # the unused row, the infeasible row
    none = nbest_posterior(x, tk, hl.clamp_min(0), 0, il, torch.zeros(3, dtype=torch.int64, device=dev), max_len=6)
    assert float(none.abs().max()) == 0.0                                # a list without a live row
    xg = x.clone().requires_grad_(True)
    ctc_nbest_scores(xg, tk, hl.clamp_min(0), 0, il, num, max_len=6)[0, 1].backward()
    only = torch.zeros(3, 4)
    only[0, 1] = 1.0
    assert_grad(xg.grad, c["dll"], only, "ctc_nbest_scores autograd")
    assert CtcNbestScoreFn.apply(x, tk, hl, il, 0).dtype == torch.float64
