"""Fused multi-tensor Adam on gfx950 (reference: torch.optim.Adam(model.parameters(), lr) at
train.py:188).  One kernel launch updates every parameter (param, grad, exp_avg, exp_avg_sq streamed once: 16 B read +
12 B written per element) instead of torch's per-dtype foreach chains.  The optimizer state keeps torch.optim.Adam's
layout ({'step', 'exp_avg', 'exp_avg_sq'} per parameter), so `manager.py`-style checkpoints interchange with the stock
optimizer.  Defaults only: no weight decay, no amsgrad, no maximize.

Step counts are PER PARAMETER, as in the stock optimizer: a parameter whose gradient is None does not advance, one that
joins later starts its bias correction at 1, and a loaded state keeps every parameter's own count.  The counts live on the
host (`step()` reads nothing back from the device; `load_state_dict` converts a loaded state's `step` tensors once) and
are written into `state[p]['step']` by `state_dict()`.  The parameters of a group that share a count go out in one
`cfm3_adam_step_f32` call: with all counts equal (the ordinary case) a step is one call per group, ceil(n / 48) launches;
otherwise one call per distinct count.  Every group is validated before the first launch, so a refused `step()` has
changed nothing.  The scalars cross the C boundary as doubles (csrc/conformer_hip3_adam.h): `1 - beta` formed from a beta
already rounded to fp32, as cfm_adam_step_f32 forms it, leaves exp_avg_sq 1.3e-5 off the stock optimizer's at beta2 = 0.999."""
from __future__ import annotations

import ctypes
import math
from typing import List

import torch

from . import _lib, ops

class _AdamTensor(ctypes.Structure):      # cfm_adam_tensor, include/conformer_hip.h
    _fields_ = [("param", ctypes.c_void_p), ("grad", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p),
                ("exp_avg_sq", ctypes.c_void_p), ("numel", ctypes.c_int64)]


def _fits(t: torch.Tensor) -> bool:
    """What the kernel takes through a raw pointer: a contiguous fp32 tensor on a HIP device."""
    return t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8) -> None:
        # the extra keys are torch.optim.Adam's own defaults, so a state_dict saved here loads into the stock optimizer
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=0, amsgrad=False, maximize=False,
                                      foreach=None, capturable=False, differentiable=False, fused=None,
                                      decoupled_weight_decay=False))
        self._tables = {}
        self._counts = {}           # parameter -> step count (mirrored into state[p]['step'] by state_dict())

    def _table(self, key, plist: List[torch.Tensor]):
        """Host descriptor array of one call (key: group index, call index within the step), rebuilt when the call's members
        change; otherwise the state pointers are stable and only the parameter / gradient pointers are refreshed."""
        hit = self._tables.get(key)
        ids = [id(p) for p in plist]
        if hit is None or hit[0] != ids:
            arr = (_AdamTensor * len(plist))()
            for i, p in enumerate(plist):
                st = self.state[p]
                arr[i] = _AdamTensor(p.data_ptr(), 0, st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel())
            hit = (ids, arr)
            self._tables[key] = hit
        arr = hit[1]
        for i, p in enumerate(plist):
            arr[i].grad = p.grad.data_ptr()
            arr[i].param = p.data_ptr()
        return arr

    def _count(self, p: torch.Tensor) -> int:
        """The host count of a parameter seen for the first time: its state's `step` (0 for a new state, created here)."""
        st = self.state[p]
        if not st:
            st["step"] = torch.tensor(0.0)
            st["exp_avg"] = torch.zeros(p.shape, device=p.device, dtype=torch.float32)
            st["exp_avg_sq"] = torch.zeros(p.shape, device=p.device, dtype=torch.float32)
        c = self._counts[p] = int(st["step"])
        return c

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        work = []
        for gi, group in enumerate(self.param_groups):          # every group is checked before the first launch
            plist = [p for p in group["params"] if p.grad is not None]
            if not plist:
                continue
            if group["weight_decay"] or group["amsgrad"] or group["maximize"]:
                raise _lib.ConformerHipError("FusedAdam: weight_decay / amsgrad / maximize are not built (train.py:188 uses none)")
            for p in plist:
                if not (_fits(p) and _fits(p.grad)):
                    raise _lib.ConformerHipError("FusedAdam: parameters and gradients must be contiguous fp32 HIP tensors")
            work.append((gi, group, plist))
        counts = self._counts
        for gi, group, plist in work:
            steps = [(counts[p] if p in counts else self._count(p)) + 1 for p in plist]
            first = steps[0]
            if steps.count(first) == len(steps):                 # all parameters of the group step together: one call
                calls = [(first, plist)]
            else:                                                # one call per distinct count
                by_step = {}
                for p, s in zip(plist, steps):
                    by_step.setdefault(s, []).append(p)
                calls = list(by_step.items())
            b1, b2 = group["betas"]
            lr, eps = float(group["lr"]), group["eps"]
            for k, (step, members) in enumerate(calls):
                arr = self._table((gi, k), members)
                _lib.call("cfm3_adam_step_f32", ctypes.addressof(arr), len(members), lr, b1, b2, eps,
                          1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step), ops._stream())
            for p, s in zip(plist, steps):
                counts[p] = s
            # the kernel wrote through raw pointers: tell autograd (and every cache keyed on `_version`: the packed / fused /
            # 16-bit weight copies of the modules and of ops.weight16) that the parameters changed in place
            torch.autograd.graph.increment_version(plist)
            ops.refresh_weight16(plist)                  # the cached 16-bit weight copies of the autocast path, in one batched launch
        return loss

    def _sync_steps(self) -> None:
        for p, c in self._counts.items():
            st = self.state.get(p)
            if st and float(st["step"]) != c:
                st["step"] = torch.tensor(float(c))

    def state_dict(self):
        self._sync_steps()
        return super().state_dict()

    def load_state_dict(self, state_dict) -> None:
        super().load_state_dict(state_dict)
        self._counts.clear()
        self._tables.clear()
        for p, st in self.state.items():                         # the one place a count may come back from the device
            if st and "step" in st:
                c = self._counts[p] = int(st["step"])
                if not (torch.is_tensor(st["step"]) and st["step"].device.type == "cpu"):
                    st["step"] = torch.tensor(float(c))
