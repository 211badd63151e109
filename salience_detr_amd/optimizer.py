"""The last two lines of the reference's training step (util/engine.py:56-61) on this project's own kernels:
``clip_grad_norm_(model.parameters(), 0.1)`` + ``torch.optim.AdamW.step()`` as TWO launches (csrc/optimizer.hip), and the
parameter groups of the reference's ``optimizer/param_dict.py``.

``ClippedAdamW`` is a ``torch.optim.Optimizer``: ``param_groups``, ``zero_grad``, torch's LR schedulers and
``state_dict()`` / ``load_state_dict()`` in ``torch.optim.AdamW``'s own format work as they do there.  What differs:

* the clip is part of the step (``max_norm``; ``<= 0``: none) and ``last_grad_norm`` is the total norm as a device scalar,
  what ``clip_grad_norm_`` returns -- nothing in ``step()`` waits for the device;
* parameters stay where the model owns them; the two moments live in two flat buffers (``state[p]["exp_avg"]`` is a view);
* the kernels write through raw pointers, so ``step()`` bumps every updated parameter's ``_version`` itself
  (``torch.autograd.graph.increment_version``): the ``derived()`` operand caches key on it (derived.py);
* ``step_captured()`` issues the two launches only (no host-to-device copy, no memset: it replays as it ran), and
  ``after_replay()`` does the host's part after every replay of a graph that holds it; a graph that also holds the
  forward and backward is captured after ``prepare(whole_step=True)`` (the operands derived from the weights are then
  rebuilt inside the graph);
* ``from_reducer(reducer)`` reads the gradients from a ``StaticGradAllReducer``'s flat buffer and folds ``1 / world``
  into the step: ``reducer.all_reduce(average=False); optimizer.step()``.

Parameters on the CPU take ``_cpu_step``: the same statement in plain torch operations (the CPU tests and the gloo test
run there).  A HIP parameter always goes through the kernels; there is no fallback between the two.
"""
import math
from typing import Dict, List, Optional

import numpy as np
import torch
from torch import nn
from torch.optim import Optimizer

from . import _hip

__all__ = ["ClippedAdamW", "param_groups", "POLICIES"]

_RECORD = np.dtype([("param", "<u8"), ("grad", "<u8"), ("moment_offset", "<i8"), ("length", "<i8"), ("group", "<i4"),
                    ("lag", "<i4")])           # sdetr_adamw_record
_CHUNK = np.dtype([("record", "<i4"), ("start", "<i4"), ("count", "<i4"), ("reserved", "<i4")])    # sdetr_adamw_chunk
CHUNK_ELEMENTS = 1024      # SDETR_ADAMW_CHUNK (checked against the library when it is first used)
MAX_PARTIALS = 1024        # SDETR_ADAMW_MAX_PARTIALS
_TABLE_RING = 4            # pinned staging buffers of the per-group (lr, weight_decay) table


def build_tables(lengths, chunk=CHUNK_ELEMENTS):
    """The chunk table and the wave-item table for tensors of ``lengths`` elements (record i = tensor i), as numpy
    arrays: every tensor is cut into chunks of at most ``chunk`` elements; consecutive chunks are packed into one wave item
    while together they stay within ``chunk`` elements (a full chunk is an item of its own)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    assert lengths.ndim == 1 and lengths.size > 0 and (lengths > 0).all() and (lengths < 2 ** 31).all()
    per = (lengths + chunk - 1) // chunk
    record = np.repeat(np.arange(lengths.size, dtype=np.int64), per)
    first = np.repeat(np.cumsum(per) - per, per)
    start = (np.arange(record.size, dtype=np.int64) - first) * chunk
    count = np.minimum(lengths[record] - start, chunk)
    chunks = np.zeros(record.size, dtype=_CHUNK)
    chunks["record"], chunks["start"], chunks["count"] = record, start, count
    # every full chunk is an item of its own; only the tails (at most one per tensor) are packed, so the loop below takes
    # one Python step per TENSOR that has a tail, never one per chunk
    starts = np.ones(record.size, dtype=bool)            # chunk i opens a wave item
    tails = np.flatnonzero(count != chunk)
    filled, previous = 0, -2
    for i, c in zip(tails.tolist(), count[tails].tolist()):
        if previous == i - 1 and filled + c <= chunk:    # joins the item of the tail right before it
            starts[i] = False
            filled += c
        else:
            filled = c
        previous = i
    wave_first = np.append(np.flatnonzero(starts), record.size)
    return chunks, wave_first.astype(np.int32)


class ClippedAdamW(Optimizer):
    def __init__(self, params, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-4,
                 max_norm: float = 0.1, grad_scale: float = 1.0, amsgrad: bool = False, maximize: bool = False):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not 0.0 <= weight_decay:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if not (math.isfinite(grad_scale) and grad_scale > 0):
            raise ValueError(f"Invalid grad_scale: {grad_scale}")
        self.max_norm, self.grad_scale = float(max_norm), float(grad_scale)
        self._allocated = False
        self._grad_views: Optional[Dict[int, torch.Tensor]] = None      # from_reducer: id(p) -> slice of the flat buffer
        # the keys torch.optim.AdamW keeps in a group, so that a state dict moves between the two classes as it is
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        self._check_groups()

    # ---- construction ----------------------------------------------------------------------------------------------
    @classmethod
    def from_reducer(cls, reducer, params=None, **kwargs) -> "ClippedAdamW":
        """An optimizer over ``params`` (default: the reducer's parameters, one group) whose gradients are the slices of
        ``reducer.flat`` (``StaticGradAllReducer``).  ``grad_scale`` defaults to ``1 / world``: with
        ``reducer.all_reduce(average=False)`` the step reads the SUM and averages, clips and updates in one pass."""
        import torch.distributed as dist
        if "grad_scale" not in kwargs:
            world = 1
            if dist.is_available() and dist.is_initialized():
                world = dist.get_world_size(reducer.group)
            kwargs["grad_scale"] = 1.0 / world
        opt = cls(list(reducer.params) if params is None else params, **kwargs)
        views = {id(p): v for p, v in zip(reducer.params, reducer.views)}
        for group in opt.param_groups:
            for p in group["params"]:
                if id(p) not in views:
                    raise ValueError("from_reducer: a parameter of the optimizer is not one of the reducer's")
        opt._grad_views = views
        return opt

    def _check_groups(self) -> None:
        for group in self.param_groups:
            if group.get("amsgrad", False):
                raise ValueError("ClippedAdamW: amsgrad=True is not supported")
            if group.get("maximize", False):
                raise ValueError("ClippedAdamW: maximize=True is not supported")
            if not group.get("decoupled_weight_decay", True):
                raise ValueError("ClippedAdamW: only decoupled weight decay (AdamW) is supported")
            if len(group["betas"]) != 2 or tuple(group["betas"]) != tuple(self.param_groups[0]["betas"]) or \
                    group["eps"] != self.param_groups[0]["eps"]:
                raise ValueError("ClippedAdamW: betas and eps are shared by all parameter groups")
            for p in group["params"]:
                if p.dtype != torch.float32:
                    raise ValueError(f"ClippedAdamW: parameters must be float32, got {p.dtype}")
                if p.is_sparse or not p.is_contiguous():
                    raise ValueError("ClippedAdamW: parameters must be dense and contiguous")

    def add_param_group(self, param_group) -> None:
        if getattr(self, "_allocated", False):
            raise RuntimeError("ClippedAdamW: parameter groups can only be added before the first step (the moments of "
                               "all parameters share two flat buffers)")
        super().add_param_group(param_group)
        self._check_groups()

    # ---- state -----------------------------------------------------------------------------------------------------
    def _allocate(self) -> None:
        """Flat moment buffers; a tensor's moments start at its parameter's misalignment (in elements, mod 4), so that they
        are 16-byte aligned wherever the parameter is."""
        self._params: List[nn.Parameter] = [p for g in self.param_groups for p in g["params"]]
        if not self._params:
            raise ValueError("ClippedAdamW: no parameters")
        self._group_of = [gi for gi, g in enumerate(self.param_groups) for _ in g["params"]]
        self.device = self._params[0].device
        if any(p.device != self.device for p in self._params):
            raise ValueError("ClippedAdamW: all parameters must live on one device")
        self._offsets, cursor = [], 0
        for p in self._params:
            cursor = (cursor + 3) // 4 * 4 + (p.data_ptr() // 4) % 4
            self._offsets.append(cursor)
            cursor += p.numel()
        self._exp_avg = torch.zeros(cursor + 4, dtype=torch.float32, device=self.device)
        self._exp_avg_sq = torch.zeros_like(self._exp_avg)
        self._views = [(self._exp_avg[o:o + p.numel()].view_as(p), self._exp_avg_sq[o:o + p.numel()].view_as(p))
                       for o, p in zip(self._offsets, self._params)]
        self._steps = [0] * len(self._params)       # steps each parameter has taken (torch counts them per parameter)
        self._global_step = 0                       # the device counter's value
        self._norm = torch.zeros((), dtype=torch.float32, device=self.device)
        self._key = None
        self._replay_active: List[int] = []
        if self.device.type == "cuda":
            lib = _hip.lib()
            if lib.sdetr_adamw_chunk_elements() != CHUNK_ELEMENTS or lib.sdetr_adamw_max_partials() != MAX_PARTIALS:
                raise _hip.HipExtensionError("ClippedAdamW: the library's chunk geometry is not this module's")
            self._counter = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._partials = torch.zeros(MAX_PARTIALS, dtype=torch.float64, device=self.device)
            self._group_table = torch.zeros(len(self.param_groups), 2, dtype=torch.float64, device=self.device)
            self._ring = [torch.zeros(len(self.param_groups), 2, dtype=torch.float64).pin_memory()
                          for _ in range(_TABLE_RING)]
            self._ring_events = [None] * _TABLE_RING
            self._ring_at = 0
            self._group_values = None
        self._allocated = True

    @property
    def last_grad_norm(self) -> torch.Tensor:
        """Total gradient norm of the last step (before clipping), a scalar tensor on the parameters' device."""
        if not self._allocated:
            self._allocate()
        return self._norm

    def _sync_state(self) -> None:
        """``self.state`` in torch.optim.AdamW's layout for every parameter that has taken a step."""
        if not self._allocated:
            return
        for p, n, (m, v) in zip(self._params, self._steps, self._views):
            if n > 0:
                self.state[p] = {"step": torch.tensor(float(n), dtype=torch.float32), "exp_avg": m, "exp_avg_sq": v}

    def state_dict(self):
        self._sync_state()
        return super().state_dict()

    def load_state_dict(self, state_dict) -> None:
        if self._allocated:
            for p in self._params:
                self.state.pop(p, None)
        super().load_state_dict(state_dict)
        self._check_groups()
        loaded = dict(self.state)
        steps = {float(s["step"]) for s in loaded.values()}
        if len(steps) > 1:
            raise ValueError(f"ClippedAdamW: the loaded per-parameter steps differ ({sorted(steps)}); the step counter is "
                             "shared by all parameters")
        step = int(steps.pop()) if steps else 0
        self._allocated = False
        self._allocate()
        for i, p in enumerate(self._params):
            s = loaded.get(p)
            if s is None:
                continue
            if s["exp_avg"].shape != p.shape or s["exp_avg_sq"].shape != p.shape:
                raise ValueError("ClippedAdamW: a loaded moment does not have its parameter's shape")
            self._views[i][0].copy_(s["exp_avg"])
            self._views[i][1].copy_(s["exp_avg_sq"])
            self._steps[i] = step
        self._global_step = step
        if self.device.type == "cuda":
            self._counter.fill_(step)
        self._sync_state()

    # ---- the step --------------------------------------------------------------------------------------------------
    def _gradient(self, p) -> Optional[torch.Tensor]:
        if self._grad_views is not None:
            return self._grad_views[id(p)]
        return p.grad

    def _collect(self):
        """(indices of the parameters that take this step, their gradients)."""
        active, grads = [], []
        for i, p in enumerate(self._params):
            g = self._gradient(p)
            if g is None:
                continue
            if g.is_sparse:
                raise RuntimeError("ClippedAdamW does not support sparse gradients")
            if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape or not g.is_contiguous():
                raise RuntimeError("ClippedAdamW: a gradient must be a contiguous float32 tensor of its parameter's shape "
                                   "on its parameter's device")
            active.append(i)
            grads.append(g)
        return active, grads

    def _refresh_records(self, capturing: bool = False):
        active, grads = self._collect()
        key = tuple((i, self._params[i].data_ptr(), g.data_ptr(), self._global_step - self._steps[i])
                    for i, g in zip(active, grads))
        if key != self._key:
            if capturing:
                raise RuntimeError("ClippedAdamW.step_captured: the parameter / gradient addresses are not the ones of "
                                   "the last prepare() / step(); inside a captured region the tables cannot be copied to "
                                   "the device.  Keep the gradients where they are (zero_grad(set_to_none=False) or "
                                   "from_reducer) and call prepare() before the capture")
            if not active:
                self._key, self._active, self._tables = key, [], None
                return
            records = np.zeros(len(active), dtype=_RECORD)
            records["param"] = [k[1] for k in key]
            records["grad"] = [k[2] for k in key]
            records["moment_offset"] = [self._offsets[i] for i in active]
            records["length"] = [self._params[i].numel() for i in active]
            records["group"] = [self._group_of[i] for i in active]
            records["lag"] = [k[3] for k in key]
            chunks, wave_first = build_tables(records["length"])
            # one host-to-device copy for the three tables (each starts on a 16-byte boundary of the one buffer)
            parts = [a.view(np.uint8).reshape(-1) for a in (records, chunks, wave_first)]
            starts = np.cumsum([0] + [(a.size + 15) // 16 * 16 for a in parts])
            host = np.zeros(int(starts[-1]), dtype=np.uint8)
            for a, o in zip(parts, starts):
                host[o:o + a.size] = a
            dev = torch.from_numpy(host).to(self.device)
            d_records, d_chunks, d_wave_first = (dev[o:o + a.size] for a, o in zip(parts, starts))
            num_waves = wave_first.size - 1
            self._tables = dict(records=d_records, chunks=d_chunks, wave_first=d_wave_first,
                                num_records=len(active), num_chunks=int(chunks.size), num_waves=int(num_waves),
                                num_partials=int(min(MAX_PARTIALS, num_waves)))
            self._key, self._active = key, active
        return

    def _refresh_group_table(self) -> None:
        values = tuple((float(g["lr"]), float(g["weight_decay"])) for g in self.param_groups)
        if values == self._group_values:
            return
        slot = self._ring_at
        self._ring_at = (slot + 1) % _TABLE_RING
        if self._ring_events[slot] is not None:
            self._ring_events[slot].synchronize()      # the copy that last read this staging buffer (long done)
        self._ring[slot].copy_(torch.tensor(values, dtype=torch.float64))
        self._group_table.copy_(self._ring[slot], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._ring_events[slot] = ev
        self._group_values = values

    def prepare(self, whole_step: bool = False) -> None:
        """The host's part in front of a step: the record / chunk tables (rebuilt when a parameter or gradient address
        changed) and the per-group ``lr`` / ``weight_decay`` table.  ``step()`` calls it; call it yourself before
        capturing ``step_captured()``.

        ``whole_step=True`` when the captured region also holds the forward and backward: the parameters' versions are
        bumped once more, so every ``derived()`` operand built from them (derived.py) is stale and is rebuilt INSIDE the
        captured region.  The rebuild is then part of the graph and every replay derives its operands from the weights
        the replay before it wrote; an operand cached before the capture would be read by every replay as it was."""
        if not self._allocated:
            self._allocate()
        if self.device.type != "cuda":
            return
        self._refresh_records()
        self._refresh_group_table()
        if whole_step:
            torch.autograd.graph.increment_version(self._params)

    def _launch(self) -> None:
        t = self._tables
        dev = t["records"].device
        g0 = self.param_groups[0]
        _hip.launch("sdetr_adamw_grad_sumsq", None, dev, t["records"].data_ptr(), t["num_records"],
                    t["chunks"].data_ptr(), t["num_chunks"], t["wave_first"].data_ptr(), t["num_waves"],
                    t["num_partials"], self._partials.data_ptr(), self._counter.data_ptr())
        _hip.launch("sdetr_adamw_clip_step", None, dev, t["records"].data_ptr(), t["num_records"],
                    t["chunks"].data_ptr(), t["num_chunks"], t["wave_first"].data_ptr(), t["num_waves"],
                    t["num_partials"], self._partials.data_ptr(), self._counter.data_ptr(),
                    self._group_table.data_ptr(), len(self.param_groups), self._exp_avg.data_ptr(),
                    self._exp_avg_sq.data_ptr(), float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"]),
                    self.max_norm, self.grad_scale, self._norm.data_ptr())

    def _account(self, active: List[int]) -> None:
        """Host bookkeeping of a step that ran: step counts, and the version bump the raw-pointer write did not make."""
        self._global_step += 1
        for i in active:
            self._steps[i] += 1
        torch.autograd.graph.increment_version([self._params[i] for i in active])

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not self._allocated:
            self._allocate()
        if self.device.type != "cuda":
            self._cpu_step()
            return loss
        self.prepare()
        if self._active:
            self._launch()
            self._account(self._active)
        return loss

    def step_captured(self) -> None:
        """The two launches and nothing else, for a region captured by ``torch.cuda.graph``.  The tables are the ones of
        the last ``prepare()`` / ``step()`` / ``after_replay()``; call ``after_replay()`` after every replay."""
        if not self._allocated or self.device.type != "cuda":
            raise RuntimeError("ClippedAdamW.step_captured: HIP parameters and a prepare() or step() before the capture")
        capturing = torch.cuda.is_current_stream_capturing()
        self._refresh_records(capturing=capturing)
        if not self._active:
            raise RuntimeError("ClippedAdamW.step_captured: no parameter has a gradient")
        self._launch()
        if capturing:
            self._replay_active = list(self._active)
        else:
            self._account(self._active)

    def after_replay(self) -> None:
        """After each replay of a graph that holds ``step_captured()``: counts the step, bumps the parameters' versions
        and refreshes the per-group table (a scheduler's new ``lr``) for the next replay."""
        if not self._replay_active:
            raise RuntimeError("ClippedAdamW.after_replay: no captured step")
        self._account(self._replay_active)
        self._refresh_group_table()

    # ---- the same statement in plain torch operations (CPU parameters) ------------------------------------------------
    def _cpu_step(self) -> None:
        active, grads = self._collect()
        if not active:
            return
        g0 = self.param_groups[0]
        beta1, beta2, eps = float(g0["betas"][0]), float(g0["betas"][1]), float(g0["eps"])
        sumsq = torch.zeros((), dtype=torch.float64)
        for g in grads:
            sumsq += g.detach().double().pow(2).sum()
        total_norm = (self.grad_scale * sumsq.sqrt()).float()
        coef = torch.ones((), dtype=torch.float32)
        if self.max_norm > 0:
            coef = self.max_norm / (total_norm + 1e-6)
            coef = torch.where(coef > 1.0, torch.ones_like(coef), coef)        # a NaN stays
        clip = coef * torch.tensor(self.grad_scale, dtype=torch.float32)
        self._norm.copy_(total_norm)
        for i, g in zip(active, grads):
            p, (m, v) = self._params[i].data, self._views[i]
            group = self.param_groups[self._group_of[i]]
            lr, wd = float(group["lr"]), float(group["weight_decay"])
            step = self._steps[i] + 1
            g = g.detach() * clip
            p.mul_(1 - lr * wd)
            m.lerp_(g, 1 - beta1)
            v.mul_(beta2).addcmul_(g, g, value=1 - beta2)
            step_size = lr / (1 - beta1 ** step)
            denom = (v.sqrt() / (1 - beta2 ** step) ** 0.5).add_(eps)
            p.addcdiv_(m, denom, value=-step_size)
        self._account(active)


# ---- parameter groups (reference optimizer/param_dict.py) --------------------------------------------------------------
_NORM_CLASSES = (nn.modules.batchnorm._BatchNorm, nn.LayerNorm, nn.GroupNorm, nn.modules.instancenorm._InstanceNorm,
                 nn.LocalResponseNorm)


def _has(name: str, *words: str) -> bool:
    return any(w in name for w in words)


def _groups_backbone(model: nn.Module, lr: float):
    """Two groups: everything else at ``lr``; names containing ``backbone`` at ``lr / 10``."""
    rest, backbone = [], []
    for name, p in model.named_parameters():
        if p.requires_grad:
            (backbone if "backbone" in name else rest).append(p)
    return [{"params": rest}, {"params": backbone, "lr": lr * 0.1}]


def _groups_backbone_no_norm_decay(model: nn.Module, lr: float):
    """Four groups by MODULE: other | backbone norms (lr / 10, no decay) | other norms (no decay) | backbone (lr / 10).
    A module with children contributes its own direct parameters to the plain groups; a leaf contributes all of its
    parameters, to a norm group when it is one of torch's normalisation layers."""
    other, backbone_norm, other_norm, backbone = [], [], [], []
    seen = set()
    for name, module in model.named_modules():
        in_backbone = "backbone" in name
        leaf = next(module.children(), None) is None
        if leaf and isinstance(module, _NORM_CLASSES):
            dest = backbone_norm if in_backbone else other_norm
        else:
            dest = backbone if in_backbone else other
        for p in module.parameters(recurse=False):
            if p.requires_grad and id(p) not in seen:
                seen.add(id(p))
                dest.append(p)
    return [{"params": other}, {"params": backbone_norm, "lr": lr * 0.1, "weight_decay": 0},
            {"params": other_norm, "weight_decay": 0}, {"params": backbone, "lr": lr * 0.1}]


def _groups_backbone_and_linear_projection(model: nn.Module, lr: float):
    """Six groups by NAME.  A name is ``backbone`` when it contains that word, a ``linear projection`` when it contains
    ``reference_points`` or ``sampling_offsets``, and free of weight decay when it contains ``norm`` or ``bias``.
    Backbone-only and projection-only names train at ``lr / 10``; a name that is both or neither trains at ``lr``:
    0 other | 1 backbone | 2 backbone, no decay | 3 projection | 4 projection, no decay | 5 other, no decay."""
    groups = [[] for _ in range(6)]
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        is_backbone, is_projection = _has(name, "backbone"), _has(name, "reference_points", "sampling_offsets")
        no_decay = _has(name, "norm", "bias")
        if is_backbone and not is_projection:
            base = 1
        elif is_projection and not is_backbone:
            base = 3
        else:
            base = None
        groups[(5 if no_decay else 0) if base is None else base + int(no_decay)].append(p)
    tenth = lr * 0.1
    return [{"params": groups[0]}, {"params": groups[1], "lr": tenth},
            {"params": groups[2], "lr": tenth, "weight_decay": 0}, {"params": groups[3], "lr": tenth},
            {"params": groups[4], "lr": tenth, "weight_decay": 0}, {"params": groups[5], "weight_decay": 0}]


POLICIES = {"backbone_and_linear_projection": _groups_backbone_and_linear_projection,      # the reference's default
            "backbone": _groups_backbone,
            "backbone_no_norm_weight_decay": _groups_backbone_no_norm_decay}


def param_groups(model: nn.Module, lr: float, policy: str = "backbone_and_linear_projection"):
    """The parameter-group list of the reference's ``optimizer/param_dict.py`` for ``model``: a list of dicts for
    ``ClippedAdamW`` / ``torch.optim.AdamW``; a group states ``lr`` / ``weight_decay`` only where it departs from the
    optimizer's defaults.  Every trainable parameter lands in exactly one group; a tensor registered under two names
    (``encoder_class_head`` and ``encoder.enhance_mcsp`` share theirs) is listed once, under its first name."""
    if policy not in POLICIES:
        raise ValueError(f"param_groups: unknown policy {policy!r} (one of {sorted(POLICIES)})")
    return POLICIES[policy](model, lr)
