"""Kernel operands derived from parameters (packed MFMA weights, fp32 copies, concatenated projections, folded plans):
built once per parameter version and cached on the object that owns them.

``derived(owner, name, sources, build, extra)`` keeps ``build()``'s value in ``owner.__dict__["_sdetr_derived"][name]``
and rebuilds it when the key changes: ``data_ptr``, ``_version``, dtype, device and shape of every source tensor, plus
``extra``.  Optimizer steps, ``load_state_dict``, ``.to()`` and in-place ops change it; a write THROUGH ``p.data``
(``p.data.copy_()``, ``dist.broadcast(p.data)``, ``nn.init`` on ``.data``) does not -- call ``invalidate_caches(module)``
afterwards, or write ``with torch.no_grad(): p.copy_(..)``."""
from typing import Callable, Hashable, Optional, Sequence, TypeVar

from torch import Tensor, nn

T = TypeVar("T")
_ATTR = "_sdetr_derived"


def derived(owner, name: str, sources: Sequence[Optional[Tensor]], build: Callable[[], T], extra: Hashable = ()) -> T:
    """``build()``, cached on ``owner`` (a parameter or a module) under ``name`` and keyed on ``sources`` + ``extra``."""
    key = (tuple(None if t is None else (t.data_ptr(), t._version, t.dtype, t.device, t.shape) for t in sources), extra)
    cache = owner.__dict__.setdefault(_ATTR, {})
    hit = cache.get(name)
    if hit is None or hit[0] != key:
        hit = cache[name] = (key, build())
    return hit[1]


def invalidate_caches(module: nn.Module) -> None:
    """Drop every ``derived`` cache of ``module``, its submodules, their parameters and their buffers."""
    for m in module.modules():
        m.__dict__.pop(_ATTR, None)
        for t in list(m.parameters(recurse=False)) + list(m.buffers(recurse=False)):
            t.__dict__.pop(_ATTR, None)
