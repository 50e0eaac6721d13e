"""The scenarios that hold conformer_amd.optim.FusedAdam against torch.optim.Adam in float64 on the CPU, shared by
tests/test_fused_adam_gpu.py (the real entry on the device) and tests/test_fused_adam_host_cpu.py (the host logic alone, the
entry replaced by the fp32 restatement).  Both optimizers start from the same fp32 values and see the same gradients; at the
end every parameter, exp_avg and exp_avg_sq agrees to rel-L2 < 2e-6 and every parameter's `step` exactly."""
import torch

from tests.util import rel_l2

TOL = 2e-6                 # the bound tests/test_next_rows_gpu.py::test_fused_adam_matches_torch_adam uses


class Twin:
    """`shapes` parameters twice: fp32 on `dev` under `fused` (FusedAdam) and float64 on the CPU under torch.optim.Adam.
    groups: a list of (indices, options) (None: one group of all, `options` from **kw)."""

    def __init__(self, fused_cls, dev, shapes, groups=None, seed=0, **kw):
        self.gen = torch.Generator().manual_seed(seed)
        self.dev = dev
        init = [torch.randn(*s, generator=self.gen) for s in shapes]
        self.ps = [torch.nn.Parameter(t.to(dev)) for t in init]
        self.rs = [torch.nn.Parameter(t.double()) for t in init]
        groups = groups or [(list(range(len(shapes))), kw)]
        self.fused = fused_cls([dict(params=[self.ps[i] for i in idx], **opts) for idx, opts in groups])
        self.ref = torch.optim.Adam([dict(params=[self.rs[i] for i in idx], **opts) for idx, opts in groups])

    def grads(self, live=None, scale=1.0, bucket=False):
        """Fresh random gradients on the parameters in `live` (None: all), None on the others.  bucket: the device gradients
        are consecutive views of one flat buffer (the gradient_as_bucket_view layout: arbitrary element offsets)."""
        live = range(len(self.ps)) if live is None else live
        gs = {i: torch.randn(self.ps[i].shape, generator=self.gen) * scale for i in live}
        flat = torch.cat([g.flatten() for g in gs.values()]).to(self.dev) if bucket and gs else None
        off = 0
        for i, (p, r) in enumerate(zip(self.ps, self.rs)):
            if i not in gs:
                p.grad = r.grad = None
                continue
            r.grad = gs[i].double()
            if flat is None:
                p.grad = gs[i].to(self.dev)
            else:
                p.grad = flat[off:off + p.numel()].view(p.shape)
                off += p.numel()

    def step(self):
        self.fused.step()
        self.ref.step()

    def set_lr(self, lr, group=0):
        self.fused.param_groups[group]["lr"] = lr
        self.ref.param_groups[group]["lr"] = lr.clone().double() if torch.is_tensor(lr) else lr

    def check(self, what=""):
        assert_same(self.fused, self.ps, self.ref, self.rs, what)


def assert_same(fused, ps, ref, rs, what=""):
    fused.state_dict()                                           # (writes the host counts into state[p]['step'])
    for i, (p, r) in enumerate(zip(ps, rs)):
        tag = f"{what} parameter {i} {tuple(p.shape)}"
        assert rel_l2(p, r) < TOL, (tag, rel_l2(p, r))
        sf, sr = fused.state.get(p) or {}, ref.state.get(r) or {}
        assert bool(sf) == bool(sr), f"{tag}: state {sorted(sf)} vs {sorted(sr)}"
        if sr:
            assert float(sf["step"]) == float(sr["step"]), f"{tag}: step {float(sf['step'])} vs {float(sr['step'])}"
            for k in ("exp_avg", "exp_avg_sq"):
                assert rel_l2(sf[k], sr[k]) < TOL, (tag, k, rel_l2(sf[k], sr[k]))


SHAPES = [(33, 7), (17,), (4099,), (1,), (5, 3, 2)]


def late_join(fused_cls, dev):
    """Parameter 1 has no gradient on the first two of five steps: its count starts at 1 on the third."""
    tw = Twin(fused_cls, dev, SHAPES, lr=1e-2)
    for k in range(5):
        tw.grads([i for i in range(len(SHAPES)) if k >= 2 or i != 1])
        tw.step()
        tw.check(f"after step {k + 1}:")
    tw.fused.state_dict()
    assert [int(tw.fused.state[p]["step"]) for p in tw.ps] == [5, 3, 5, 5, 5]


def skip_and_resume(fused_cls, dev):
    """Parameter 2 has no gradient on step 3 of 5: nothing of it moves on that step, and it resumes at its own count."""
    tw = Twin(fused_cls, dev, SHAPES, lr=1e-2)
    for k in range(5):
        tw.grads([i for i in range(len(SHAPES)) if k != 2 or i != 2])
        before = None
        if k == 2:
            st = tw.fused.state[tw.ps[2]]
            before = [t.detach().clone() for t in (tw.ps[2], st["exp_avg"], st["exp_avg_sq"])]
        tw.step()
        if before is not None:
            st = tw.fused.state[tw.ps[2]]
            assert all(torch.equal(a, b) for a, b in zip(before, (tw.ps[2], st["exp_avg"], st["exp_avg_sq"])))
        tw.check(f"after step {k + 1}:")
    tw.fused.state_dict()
    assert [int(tw.fused.state[p]["step"]) for p in tw.ps] == [5, 5, 4, 5, 5]


def stock_state_with_unequal_counts(dev, seed=3):
    """A torch.optim.Adam (float64, CPU) whose parameters carry the counts 4, 2, 4, 1, 3, and its parameters."""
    g = torch.Generator().manual_seed(seed)
    rs = [torch.nn.Parameter(torch.randn(*s, generator=g).float().double()) for s in SHAPES]
    ref = torch.optim.Adam(rs, lr=1e-2)
    for k in range(4):
        for i, r in enumerate(rs):
            r.grad = torch.randn(r.shape, generator=g).float().double() if k < (4, 2, 4, 1, 3)[i] else None
        ref.step()
    for r in rs:
        r.grad = None
    return ref, rs, g


def loaded_stock_state(fused_cls, dev):
    """A stock state with unequal per-parameter counts goes into FusedAdam (its moments as fp32); both continue two steps."""
    ref, rs, g = stock_state_with_unequal_counts(dev)
    ps = [torch.nn.Parameter(r.detach().float().to(dev)) for r in rs]
    with torch.no_grad():
        for r, p in zip(rs, ps):
            r.copy_(p.double())                                  # the same fp32 starting values on both sides
    sd = ref.state_dict()
    for st in sd["state"].values():                              # ... and the same fp32 moments
        st["exp_avg"], st["exp_avg_sq"] = st["exp_avg"].float().double(), st["exp_avg_sq"].float().double()
    ref.load_state_dict(sd)
    fused = fused_cls(ps, lr=1e-2)
    fused.load_state_dict(sd)
    for p in ps:
        st = fused.state[p]
        assert st["exp_avg"].dtype == torch.float32 and st["exp_avg"].device == p.device
    assert_same(fused, ps, ref, rs, "as loaded:")
    for k in range(2):
        for p, r in zip(ps, rs):
            gr = torch.randn(r.shape, generator=g)
            p.grad, r.grad = gr.to(dev), gr.double()
        fused.step()
        ref.step()
        assert_same(fused, ps, ref, rs, f"after step {k + 1}:")
    assert [int(fused.state[p]["step"]) for p in ps] == [6, 4, 6, 3, 5]


def fused_state_into_stock(fused_cls, dev):
    """FusedAdam.state_dict() carries the per-parameter counts into torch.optim.Adam."""
    tw = Twin(fused_cls, dev, SHAPES, lr=1e-2)
    for k in range(3):
        tw.grads([i for i in range(len(SHAPES)) if k >= 1 or i != 3])
        tw.step()
    stock = torch.optim.Adam([torch.nn.Parameter(p.detach().clone()) for p in tw.ps], lr=1e-2)
    stock.load_state_dict(tw.fused.state_dict())
    assert [int(stock.state[p]["step"]) for p in stock.param_groups[0]["params"]] == [3, 3, 3, 2, 3]
    for p, q in zip(tw.ps, stock.param_groups[0]["params"]):
        assert torch.equal(stock.state[q]["exp_avg"], tw.fused.state[p]["exp_avg"])


def two_groups(fused_cls, dev):
    groups = [([0, 2, 4], dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)), ([1, 3], dict(lr=3e-4, betas=(0.5, 0.9), eps=1e-3))]
    tw = Twin(fused_cls, dev, SHAPES, groups)
    for k in range(4):
        tw.grads()
        tw.step()
    tw.check()


def changing_lr(fused_cls, dev):
    """lr changed between steps: as a float, then as a 0-d tensor (what schedulers leave in the group)."""
    tw = Twin(fused_cls, dev, SHAPES, lr=1e-2)
    for lr in (1e-2, 5e-3, torch.tensor(2.5e-3), torch.tensor(1e-4, dtype=torch.float64)):
        tw.set_lr(lr)
        tw.grads()
        tw.step()
    tw.check()


def many_parameters(fused_cls, dev):
    """120 parameters of mixed sizes in one group: three launches of the entry, one call."""
    sizes = (1, 5, 4096, 4097, 17, 1023, 33)
    shapes = [(sizes[i % len(sizes)],) for i in range(120)]
    tw = Twin(fused_cls, dev, shapes, lr=1e-3)
    for k in range(3):
        tw.grads(scale=0.1 + k)
        tw.step()
    tw.check()


def bucket_view_gradients(fused_cls, dev):
    """Gradients that are consecutive views of one flat buffer, odd sizes: every offset mod 4 occurs."""
    shapes = [(3,), (5, 7), (1,), (4099,), (2, 3), (17,), (1023,)]
    tw = Twin(fused_cls, dev, shapes, lr=1e-2)
    for k in range(3):
        tw.grads(bucket=True)
        assert {p.grad.data_ptr() % 16 for p in tw.ps} >= {0, 4, 8, 12} or dev.type == "cpu"
        tw.step()
    tw.check()


CASES = [late_join, skip_and_resume, loaded_stock_state, fused_state_into_stock, two_groups, changing_lr, many_parameters,
         bucket_view_gradients]
