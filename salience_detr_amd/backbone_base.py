"""What the four HIP backbones (``backbone.py``, ``convnext.py``, ``focalnet.py``, ``swin.py``) share on top of
``hip_module.HipModule``: ``HipBackbone``, with the torch / HIP dispatch, checkpoint loading, the operand packers, the
opening checks of a ``forward_hip`` and a backbone's side of the training interface (``hip_train_reason``,
``forward_hip_train`` and the autograd node's hooks: a backbone with a HIP backward adds its forward's stored state and a
``_backward_ops``, which the default ``_run_backward`` runs); and the two parameter-free holder modules ``Permute`` and
``StochasticDepth``."""
import os
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor, nn

from . import _hip
from .derived import derived
from .hip_module import HipModule, _TrainFunction


class Permute(nn.Module):
    def __init__(self, dims: Sequence[int]):
        super().__init__()
        self.dims = list(dims)

    def forward(self, x: Tensor) -> Tensor:
        return torch.permute(x, self.dims)


class StochasticDepth(nn.Module):
    """torchvision's ``StochasticDepth``: in training one Bernoulli(1 - p) per sample (``"row"``) or per batch
    (``"batch"``), survivors divided by 1 - p; the identity with ``p == 0`` or in ``eval()``."""

    def __init__(self, p: float, mode: str):
        super().__init__()
        if p < 0.0 or p > 1.0:
            raise ValueError(f"drop probability has to be between 0 and 1, but got {p}")
        if mode not in ("batch", "row"):
            raise ValueError(f"mode has to be either 'batch' or 'row', but got {mode}")
        self.p, self.mode = p, mode

    def forward(self, x: Tensor) -> Tensor:
        if not self.training or self.p == 0.0:
            return x
        survival = 1.0 - self.p
        size = [x.shape[0]] + [1] * (x.ndim - 1) if self.mode == "row" else [1] * x.ndim
        noise = torch.empty(size, dtype=x.dtype, device=x.device).bernoulli_(survival)
        if survival > 0.0:
            noise.div_(survival)
        return x * noise

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}(p={self.p}, mode={self.mode})"


class HipBackbone(HipModule):
    """A backbone with a HIP inference form (``forward_hip``, one plan per forward) and a plain-torch composite
    (``forward_torch``, the autograd path); a subclass gives both, ``hip_form()`` and ``compute_dtype``.

    One with a HIP backward also gives ``train_reasons`` and ``_stem_modules()`` (what ``hip_train_reason`` says in its
    own words), ``_output_name(i)``, ``forward_hip(x, splits, state)`` (``state``, a dict, receives what the backward
    reads) and ``_backward_ops(acts, factors, shape, cotangents, splits)`` (``(ops, names, grads, keep)``, filled through
    a ``PlanBuilder``), run as ``backward_struct`` ops by ``<backward_prefix>_run``.  The rest has a default here:
    ``_trainable()`` (``[(name, tensor)]``: the autograd node's inputs), the test hooks, ``_run_backward(state, shape,
    cotangents, splits)`` (``{name: fp32 gradient}``) and, for a backbone whose backward walks ``_sequence()`` (``[(kind,
    name, module)]`` in forward order), ``_first_trainable()``."""

    # of a backbone with a HIP backward: why hip_form() is False, why a trainable stem is not served
    train_reasons: Optional[Tuple[str, str]] = None
    # of the default _run_backward: the backward op struct and the C prefix of its entry points
    backward_struct = None
    backward_prefix: Optional[str] = None

    @staticmethod
    def _freeze(module: nn.Module):
        module.eval()
        for p in module.parameters():
            p.requires_grad = False

    def _remap_checkpoint_keys(self, weights: Dict[str, Tensor]) -> Dict[str, Tensor]:
        """The checkpoint's entries under this module's own state-dict keys."""
        return weights

    def load_weights(self, weights: Union[str, Dict[str, Tensor]]):
        """A local checkpoint path or a state dict (possibly under ``"model"``); non-strict, entries whose shape does not
        match are skipped (``util.utils.load_state_dict`` of the reference).  Never downloads."""
        if isinstance(weights, str):
            if not os.path.exists(weights):
                raise FileNotFoundError(f"{type(self).__name__}: no weight file at {weights} (nothing is downloaded)")
            weights = torch.load(weights, map_location="cpu")
        if "model" in weights and isinstance(weights["model"], dict):
            weights = weights["model"]
        own = self.state_dict()
        weights = self._remap_checkpoint_keys(weights)
        matched = {k: v for k, v in weights.items() if k not in own or own[k].shape == v.shape}
        return self.load_state_dict(matched, strict=False)

    def forward(self, x: Tensor) -> Dict[str, Tensor]:
        if self.train_form == "hip" and self._needs_autograd(x):
            return self.forward_hip_train(x)
        if self._needs_autograd(x) or not self.hip_form():
            return self.forward_torch(x)
        return self.forward_hip(x)

    # ------------------------------------------------------------------------------------------ training in HIP
    def _stem_modules(self) -> Sequence[nn.Module]:
        """The modules below the first stage, whose backward is out of scope."""
        return ()

    def _extra_train_reason(self) -> Optional[str]:
        """A backbone's own eligibility rule on top of the shared ones (``hip_train_reason`` asks it); ``None``: eligible."""
        return None

    def hip_train_reason(self, x: Optional[Tensor] = None) -> Optional[str]:
        """Why the ``"hip"`` training form cannot serve this module (and input ``x``); ``None`` when it can."""
        if self.train_reasons is None:
            return "this backbone has no HIP backward"
        if not self.hip_form():
            return self.train_reasons[0]
        if any(p.requires_grad for m in self._stem_modules() for p in m.parameters()):
            return self.train_reasons[1]
        extra = self._extra_train_reason()
        if extra is not None:
            return extra
        if self.compute_dtype not in (torch.float32, torch.bfloat16):
            return f"compute dtype {self.compute_dtype} is not float32 / bfloat16 (float16 has no loss scaling here)"
        if x is not None and x.requires_grad:
            return "the input requires a gradient: the gradient to the image is out of scope"
        return None

    def forward_hip_train(self, x: Tensor, splits: int = 0) -> Dict[str, Tensor]:
        """The ``"hip"`` training form: the HIP forward plan as one autograd node.  The node keeps what the backward
        reads (the plan's own activations, no copy); its backward is one ``_run_backward`` call and returns the fp32
        parameter gradients to autograd, which accumulates them into ``.grad``."""
        self._check_train_form(x)
        named = self._trainable()
        maps = _TrainFunction.apply(self, 1, splits, tuple(n for n, _ in named), x, *[t for _, t in named])
        return dict(zip([self._output_name(i) for i in sorted(self.return_indices)], maps))

    def _train_forward(self, inputs: Sequence[Tensor], splits: int, state: dict) -> Tuple[Tensor, ...]:
        outputs = self.forward_hip(inputs[0], splits, state)
        state["shape"], state["keys"] = tuple(inputs[0].shape), sorted(outputs)
        return tuple(outputs[k] for k in state["keys"])

    def _train_backward(self, state: dict, cotangents: Sequence[Optional[Tensor]], wanted: Sequence[bool], splits: int):
        """(No gradient for the image: ``hip_train_reason`` refuses one that requires it.)"""
        return self._run_backward(state, state["shape"], dict(zip(state["keys"], cotangents)), splits), (None,)

    def _trainable(self) -> List[Tuple[str, Tensor]]:
        return [(n, p) for n, p in self.named_parameters() if p.requires_grad]

    def _first_trainable(self) -> Optional[int]:
        """The index in ``_sequence()`` of the lowest module with a trainable parameter: where the backward stops."""
        for idx, (_, _, m) in enumerate(self._sequence()):
            if any(p.requires_grad for p in m.parameters()):
                return idx
        return None

    def stochastic_depth_factors(self) -> Dict[str, Tensor]:
        """Test hook (read-only): ``{branch name: factors [B]}`` (0 or 1 / (1 - p)) the last ``"hip"`` training forward
        drew, in forward order; blocks with ``p == 0`` or in ``eval()`` draw nothing.  Valid as ``saved_activations``."""
        return dict(self._train_state()["factors"])

    def _run_backward(self, state: dict, shape, cotangents: Dict[str, Optional[Tensor]], splits: int = 0
                      ) -> Dict[str, Tensor]:
        """Runs the backward plan on the stored activations; returns ``{parameter name: fp32 gradient}``."""
        acts = state["acts"]
        if not acts:
            return {}
        ops, _, grads, keep = self._backward_ops(acts, state.get("factors"), shape, cotangents, splits)
        if ops:
            self._run_plan(self.backward_struct, self.backward_prefix, ops, next(iter(acts.values())).device)
        return grads

    def _check_image(self, x: Tensor) -> Tensor:
        """The opening checks of every ``forward_hip``: ``x`` as fp32, on the device like every parameter, ``[B, 3, H, W]``."""
        who = type(self).__name__
        if x.dtype != torch.float32:
            x = x.float()
        _hip.require_device(who, x=x)
        for t in self.parameters():
            _hip.require_device(who, parameter=t.detach())
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError(f"{who}: expected [B, 3, H, W], got {tuple(x.shape)}")
        return x

    def _packed(self, layer: nn.Module, layout: int = 0, scale: Union[None, float, Tensor] = None, scale_bias: bool = True,
                pad_to: int = 1) -> Tuple[Tensor, Tensor]:
        """``(packed weight, bias)`` of a conv or Linear for the implicit GEMM (``sdetr_backbone_pack`` with a unit norm):
        ``scale`` (a layer scale, or a constant) folded into the weight and, with ``scale_bias``, the bias; a layer
        without a bias gets zeros; the output width zero-padded to a multiple of ``pad_to``.  Built once per parameter
        version, precision and compute dtype."""
        w = layer.weight
        co, ci, k = w.shape[0], w.shape[1], (w.shape[2] if w.dim() == 4 else 1)
        cop = -(-co // pad_to) * pad_to

        def build():
            dev = w.device
            w32 = torch.zeros((cop, ci, k, k), dtype=torch.float32, device=dev)
            w32[:co] = w.detach().to(torch.float32).reshape(co, ci, k, k)
            b32 = torch.zeros(cop, dtype=torch.float32, device=dev)
            if layer.bias is not None:
                b32[:co] = layer.bias.detach().to(torch.float32)
            gamma = torch.ones(cop, device=dev)
            if isinstance(scale, Tensor):
                gamma[:co] = scale.detach().to(torch.float32).reshape(co)
            elif scale is not None:
                gamma *= float(scale)
            beta = (b32 * gamma if scale_bias else b32).contiguous()
            return self._pack(w32, (gamma, beta, torch.zeros(cop, device=dev), torch.ones(cop, device=dev)), 0.0, layout)
        sources = (w, layer.bias) + ((scale,) if isinstance(scale, Tensor) else ())
        fixed = None if isinstance(scale, Tensor) else scale
        return derived(layer, "rows_packed", sources, build,
                       extra=(self._precision(), self.compute_dtype, layout, fixed, scale_bias, pad_to))

    def _affine(self, norm: nn.LayerNorm, scale: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """The LayerNorm's affine in fp32, a layer scale folded in: ``g * (w n + b) = (g w) n + g b``."""
        def build():
            w, b = norm.weight.detach().to(torch.float32), norm.bias.detach().to(torch.float32)
            if scale is not None:
                g = scale.detach().to(torch.float32)
                w, b = w * g, b * g
            return w.contiguous(), b.contiguous()
        return derived(norm, "rows_affine", (norm.weight, norm.bias, scale), build)

    def _packed_rows_dgrad(self, layer: nn.Module, scale: Optional[Tensor] = None) -> Tensor:
        """The backward-data planes (``sdetr_backbone_pack_dgrad``, kernel 1) of a Linear's ``[out, in]`` weight, ``scale``
        (the layer scale) folded per output; of the 2x2 down-sampler conv, its weight as ``[out, (ky, kx, in)]`` rows."""
        w = layer.weight

        def build():
            w32 = w.detach().to(torch.float32)
            if w32.dim() == 4:
                w32 = w32.permute(0, 2, 3, 1)
            w32 = w32.reshape(w.shape[0], -1).contiguous()
            co = w32.shape[0]
            gamma = torch.ones(co, device=w.device) if scale is None else scale.detach().to(torch.float32).reshape(co).contiguous()
            return self._pack_dgrad(w32, gamma, torch.ones(co, device=w.device), 0.0)[0]
        return derived(layer, "rows_packed_dgrad", (w, scale), build, extra=(self._precision(), self.compute_dtype))

    def _f32(self, owner, name: str, t: Tensor) -> Tensor:
        """A parameter as a contiguous fp32 tensor, cached per version."""
        return derived(owner, "rows_f32_" + name, (t,), lambda: t.detach().to(torch.float32).contiguous().clone())
