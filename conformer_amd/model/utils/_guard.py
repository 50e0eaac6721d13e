"""Shared guards/caches for the module surface (not part of the reference API)."""
from __future__ import annotations

import os

import torch

# a module's pack cache and the documented invalidation call: the one rule of conformer_amd/_derived.py
from ..._derived import DerivedCache as PackCache, invalidate as invalidate_weight_caches  # noqa: F401

STRICT = os.environ.get("CONFORMER_AMD_STRICT", "0") == "1"


def active_dropout(drop: torch.nn.Dropout) -> float:
    """The probability an nn.Dropout sub-module applies right now (0 in eval mode) -- nn.Dropout semantics."""
    return float(drop.p) if drop.training else 0.0


def refuse_dropout(module: torch.nn.Module, what: str) -> None:
    """Dropout is only wired through the autograd Functions (training with gradients).  `.train()` under no_grad with
    p > 0 has no kernel path: refuse instead of silently skipping the masks."""
    if module.training and not torch.is_grad_enabled():
        for m in module.modules():
            if isinstance(m, torch.nn.Dropout) and m.p > 0:
                raise NotImplementedError(f"{what}: dropout p={m.p} in training mode under no_grad is not built "
                                          "(call .eval() for inference)")


def refuse_grad(module: torch.nn.Module, what: str, *tensors: torch.Tensor) -> None:
    """For pieces whose backward kernels do not exist yet (the conv-subsampling stem): refuse a call that would
    need gradients rather than return a silently non-differentiable result."""
    if torch.is_grad_enabled() and (any(t.requires_grad for t in tensors if isinstance(t, torch.Tensor))
                                    or any(p.requires_grad for p in module.parameters())):
        raise NotImplementedError(
            f"{what}: backward kernels for this piece are not built yet; freeze it (requires_grad_(False)) or call "
            "under torch.no_grad().  (No autograd fallback exists on purpose.)")
