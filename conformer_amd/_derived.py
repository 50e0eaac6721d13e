"""The one rule for what the forward derives from weights (fused q|k|v, packed conv / linear / FFN weights, folded LayerNorm, 16-bit
and split-plane copies, position tables, captured hipGraphs): valid while the sources are the same tensor objects, at the same
addresses, with the same in-place versions, in the same invalidation epoch.  Imports neither `ops` nor model code."""
import weakref
from collections import namedtuple
from typing import Callable, Hashable, Iterable, Sequence

import torch

_EPOCH = [0]


def version(t: torch.Tensor) -> int:
    """In-place version of a source tensor; inference tensors (made under torch.inference_mode(), as the reference's infer.py /
    test.py run) have no counter -- `_version` raises -- and cannot be modified in place outside that mode, so 0 identifies them."""
    return 0 if t.is_inference() else t._version


def invalidate() -> None:
    """Start a new epoch: no derived weight tensor (fused QKV, packed conv / linear weights, projected position tables, 16-bit and
    split-plane weight copies) made before hits again and every fingerprint taken before is stale.  Nothing is freed here: an old
    entry goes when its name is asked for again or a cache sweeps.  Needed only after writes that bypass PyTorch's version counter
    (`param.data.copy_(...)`; `param.data = ...` is seen through the identity check); optimizer steps, `load_state_dict` and
    ordinary in-place ops are detected automatically.  Public as conformer_amd.invalidate_weight_caches()."""
    _EPOCH[0] += 1


def fingerprint(tensors: Iterable[torch.Tensor]) -> tuple:
    """What a captured graph bakes in: the epoch and the (address, version) of every tensor."""
    return (_EPOCH[0],) + tuple((t.data_ptr(), version(t)) for t in tensors)


_Stamp = namedtuple("_Stamp", "ptr version device shape")               # what is recorded of one source
_Entry = namedtuple("_Entry", "epoch extra stamps owners value")        # owners: weak references


def _stamps(srcs: Sequence[torch.Tensor]) -> tuple:
    return tuple(_Stamp(s.data_ptr(), version(s), s.device, tuple(s.shape)) for s in srcs)


def _owner(t: torch.Tensor) -> torch.Tensor:
    """Views are re-created per call; the tensor that owns the storage identifies the weight."""
    return t if t._base is None else t._base


class DerivedCache:
    """name -> the value made from `srcs`; it hits while the epoch, `extra` (a hashable it also depends on: precision, plane
    count, table length) and every source's owner IDENTITY (weak reference: a freed tensor may hand its address to a new one),
    address, in-place version, device and shape are what they were.  One value per name: a miss replaces it, so eval pays for a
    re-layout once and training re-packs after every optimizer step."""

    def __init__(self) -> None:
        self._store = {}

    def _find(self, name: Hashable, srcs: Sequence[torch.Tensor]):
        """The entry of `name`, if it is of this epoch and of these sources' owners."""
        e = self._store.get(name)
        same = e is not None and e.epoch == _EPOCH[0] and [id(r()) for r in e.owners] == [id(_owner(s)) for s in srcs]
        return e if same else None

    def get(self, name: Hashable, srcs: Sequence[torch.Tensor], make: Callable[[], object], extra: Hashable = None):
        e, now = self._find(name, srcs), _stamps(srcs)
        if e is not None and e.extra == extra and e.stamps == now:
            return e.value
        val = make()
        if len(self._store) > 4096:           # the process-wide caches are named by addresses: drop what can never hit again
            self._store = {k: v for k, v in self._store.items() if v.epoch == _EPOCH[0] and all(r() is not None for r in v.owners)}
        self._store[name] = _Entry(_EPOCH[0], extra, now, tuple(weakref.ref(_owner(s)) for s in srcs), val)
        return val

    def refresh(self, name: Hashable, srcs: Sequence[torch.Tensor], rewrite: Callable[[Hashable, tuple, object], bool]) -> bool:
        """For a value that is rewritten IN PLACE when its sources change: an entry of these sources that is stale by version
        alone is handed to rewrite(extra, source shapes, value) and, when that returns True, stamped with the current versions.
        The shapes are handed over, not compared: the entry may come from a reshaped view of the parameter."""
        e, now = self._find(name, srcs), _stamps(srcs)
        if e is None or any((o.ptr, o.device) != (n.ptr, n.device) for o, n in zip(e.stamps, now)):
            return False                      # no entry of these sources where they are now: get() rebuilds
        if all(o.version == n.version for o, n in zip(e.stamps, now)):
            return False                      # current
        if not rewrite(e.extra, tuple(o.shape for o in e.stamps), e.value):
            return False                      # declined: stays stale
        self._store[name] = e._replace(stamps=tuple(o._replace(version=n.version) for o, n in zip(e.stamps, now)))
        return True

    def clear(self) -> None:
        self._store.clear()
