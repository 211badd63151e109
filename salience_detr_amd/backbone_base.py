"""What the four HIP backbones (``backbone.py``, ``convnext.py``, ``focalnet.py``, ``swin.py``) share: ``HipBackbone``,
the module base with the precision switch, the torch / HIP dispatch, checkpoint loading, the operand packers, the
launch of a plan, the opening checks of a ``forward_hip`` and the training interface (``set_train_form``,
``hip_train_reason``, ``forward_hip_train`` and the one autograd node behind it: a backbone with a HIP backward adds its
forward's stored state and either ``_sequence`` and ``_backward_ops``, which the default ``_run_backward`` runs, or a
``_run_backward`` of its own); ``PlanBuilder``, the op list a ``build_plan`` fills, with the stochastic-depth draw;
``BackwardPlanBuilder``, the op list, gradients, scratch buffers and shared emitters a ``_backward_ops`` fills; and the
two parameter-free holder modules ``Permute`` and ``StochasticDepth``."""
import os
import weakref
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor, nn

from . import _hip
from .derived import derived


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


class PlanBuilder:
    """The op list of one forward: ``ops`` (structs of ``struct_type``), ``names`` (one label per op), ``keep`` (every
    tensor the ops point into) and ``outputs`` (the returned maps).  ``defaults`` are the fields every op of the plan
    starts from (the batch, the splits ..); the struct's remaining fields start at zero / null.  An op's kind goes into
    the struct's first field, whatever the header calls it (``kind``, or ``op`` in ``sdetr_backbone_op``)."""

    def __init__(self, struct_type, x: Tensor, **defaults):
        self.struct_type, self.device, self.defaults = struct_type, x.device, defaults
        self.kind_field = struct_type._fields_[0][0]
        self.ops: list = []
        self.names: List[str] = []
        self.keep: List[Tensor] = [x]
        self.outputs: Dict[str, Tensor] = {}

    def new(self, shape, dtype) -> Tensor:
        t = torch.empty(shape, device=self.device, dtype=dtype)
        self.keep.append(t)
        return t

    def op(self, name: str, kind: int, **fields):
        self.ops.append(self.struct_type(**{self.kind_field: kind, **self.defaults, **fields}))
        self.names.append(name)

    def layer_norm(self, name: str, kind: int, affine: Tuple[Tensor, Tensor], eps: float, src: Tensor, out: Tensor, h: int,
                   w: int, c: int, out_f32: bool = False, **fields):
        """LayerNorm over the ``c`` channels of the fp32 rows ``src`` ``[batch, h, w, c]`` into ``out``."""
        gamma, beta = affine
        self.keep.extend((gamma, beta))
        self.op(name, kind, x=src.data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(), out=out.data_ptr(), in_channels=c,
                height=h, width=w, out_channels=c, out_f32=1 if out_f32 else 0, eps=float(eps), **fields)

    def draw(self, sd: StochasticDepth, batch: int, training_forward: bool) -> Optional[Tensor]:
        """``StochasticDepth.forward``'s own draw, in its order: the factors ``[batch, 1, 1, 1]`` (0 or 1 / (1 - p)) of
        one residual branch; ``None`` when nothing is drawn (inference, ``eval()`` or ``p == 0``)."""
        if not training_forward or not sd.training or sd.p == 0.0:
            return None
        factor = torch.empty((batch, 1, 1, 1), dtype=torch.float32, device=self.device).bernoulli_(1.0 - sd.p)
        if sd.p < 1.0:
            factor.div_(1.0 - sd.p)
        self.keep.append(factor)
        return factor


class BackwardPlanBuilder(PlanBuilder):
    """The op list of one backward over rows ``[batch, h, w, c]``: ``grads`` (``{parameter name: fp32 tensor}``, as views
    of what the ops write), the scratch buffers and one emitter per kind that ``sdetr_convnext_bwd_op`` and
    ``sdetr_swin_bwd_op`` number alike (0 dgrad, 1 wgrad, 2 rows, 3 gelu, 4 layer norm); the NCHW ingest has the caller's
    number.  An op's name is its label in the op-timing tools."""

    def __init__(self, struct_type, x: Tensor, **defaults):
        super().__init__(struct_type, x, **defaults)
        self.grads: Dict[str, Tensor] = {}
        self.scratch: Dict[tuple, Tensor] = {}
        self.flip = 0

    def tmp(self, tag: str, shape, dtype) -> Tensor:
        """A buffer the next block may overwrite: the plan runs in order on one stream."""
        key = (tag, tuple(shape), dtype)
        if key not in self.scratch:
            self.scratch[key] = self.new(shape, dtype)
        return self.scratch[key]

    def ones(self, n: int) -> Tensor:
        key = ("ones", n)
        if key not in self.scratch:
            self.scratch[key] = torch.ones(n, device=self.device)
            self.keep.append(self.scratch[key])
        return self.scratch[key]

    @staticmethod
    def want(*params) -> bool:
        return any(p is not None and p.requires_grad for p in params)

    def grad(self, name: str, shape, *params) -> Optional[Tensor]:
        """The fp32 gradient buffer of parameter ``name`` when one of ``params`` requires it, else ``None``."""
        if not self.want(*params):
            return None
        self.grads[name] = self.new(shape, torch.float32)
        return self.grads[name]

    def next_dy(self, shape) -> Tensor:
        """The stream's gradient below the current module: two fp32 buffers in turns."""
        dy = self.tmp(f"dy{self.flip}", shape, torch.float32)
        self.flip ^= 1
        return dy

    def wgrad(self, name: str, dz: Tensor, x: Tensor, ci: int, co: int, h: int, w: int) -> Tensor:
        """``dW [co, ci] = dz^T x`` of a Linear, registered as ``<name>.weight``."""
        dw = self.grads[name + ".weight"] = self.new((co, ci), torch.float32)
        self.op(name + " (wgrad)", 1, dz=dz.data_ptr(), x=x.data_ptr(), scale=self.ones(co).data_ptr(), out=dw.data_ptr(),
                channels=ci, height=h, width=w, out_channels=co)
        return dw

    def dgrad(self, name: str, packed: Tensor, dz: Tensor, out: Tensor, ci: int, co: int, h: int, w: int):
        """``out = dz W`` over the ``_packed_rows_dgrad`` planes of a Linear's weight."""
        self.keep.append(packed)
        self.op(name + " (dgrad)", 0, dz=dz.data_ptr(), weight=packed.data_ptr(), out=out.data_ptr(), channels=ci, height=h,
                width=w, out_channels=co)

    def rows(self, name: str, dz: Tensor, factor: Optional[Tensor], out: Tensor, dbias: Optional[Tensor], c: int, h: int,
             w: int):
        """``out = factor[n] * dz`` in ``out``'s type and the column sums of it (a bias gradient) into ``dbias``."""
        self.op(name + " (rows)", 2, dz=dz.data_ptr(), scale=_hip.ptr(factor), out=out.data_ptr(), dbias=_hip.ptr(dbias),
                channels=c, height=h, width=w)

    def gelu(self, name: str, dz: Tensor, pre: Tensor, dbias: Optional[Tensor], c: int, h: int, w: int):
        """``dz *= gelu'(pre)`` in place and the column sums of it (the bias gradient of the Linear in front)."""
        self.op(name + " (gelu)", 3, dz=dz.data_ptr(), x=pre.data_ptr(), out=dz.data_ptr(), dbias=_hip.ptr(dbias), channels=c,
                height=h, width=w)

    def layer_norm_bwd(self, name: str, norm: nn.LayerNorm, gamma32: Tensor, kind: int = 4, label: str = " (layer norm)",
                       **fields):
        """A LayerNorm backward (kind 4, or a backbone's own variant of it); ``fields`` are the op's remaining ones,
        tensors for its pointers.  Registers ``<name>.weight`` / ``<name>.bias``."""
        self.keep.append(gamma32)
        n = norm.weight.numel()
        affine = self.want(norm.weight, norm.bias)
        dgam = self.new((n,), torch.float32) if affine else None
        dbet = self.new((n,), torch.float32) if affine else None
        fields = {k: v.data_ptr() if isinstance(v, Tensor) else v for k, v in fields.items()}
        self.op(name + label, kind, gamma=gamma32.data_ptr(), dgamma=_hip.ptr(dgam), dbeta=_hip.ptr(dbet), eps=float(norm.eps),
                **fields)
        if self.want(norm.weight):
            self.grads[name + ".weight"] = dgam
        if self.want(norm.bias):
            self.grads[name + ".bias"] = dbet

    def ingest(self, name: str, kind: int, cotangent: Optional[Tensor], add: Optional[Tensor], c: int, h: int, w: int) -> Tensor:
        """A returned map's NCHW cotangent plus ``add`` (what arrives from above) as fp32 rows; ``add`` itself when the
        map has no cotangent."""
        if cotangent is None and add is not None:
            return add
        batch = self.defaults["batch"]
        g = torch.zeros((batch, c, h, w), device=self.device) if cotangent is None else cotangent.to(torch.float32).contiguous()
        self.keep.append(g)
        out = self.new((batch, h, w, c), torch.float32)
        self.op(name + " (ingest)", kind, dz=g.data_ptr(), add=_hip.ptr(add), out=out.data_ptr(), channels=c, height=h, width=w)
        return out


class _TrainState(dict):
    """What one ``"hip"`` training forward stored for its backward; a dict that can be weakly referenced."""


class _TrainFunction(torch.autograd.Function):
    """``HipBackbone.forward_hip_train``: inputs are the trainable parameters, outputs the returned fp32 maps."""

    @staticmethod
    def forward(ctx, backbone: "HipBackbone", x: Tensor, splits: int, names: Tuple[str, ...], *params: Tensor):
        state = _TrainState()
        outputs = backbone.forward_hip(x, splits, state)
        ctx.backbone, ctx.state, ctx.names, ctx.splits = backbone, state, names, splits
        ctx.shape = tuple(x.shape)
        ctx.keys = sorted(outputs)
        backbone.__dict__["_train_state_ref"] = weakref.ref(state)
        return tuple(outputs[k] for k in ctx.keys)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *grads):
        got = ctx.backbone._run_backward(ctx.state, ctx.shape, dict(zip(ctx.keys, grads)), ctx.splits)
        return (None, None, None, None) + tuple(None if n not in got else got[n].contiguous() for n in ctx.names)


class HipBackbone(nn.Module):
    """A backbone with a HIP inference form (``forward_hip``, one plan per forward) and a plain-torch composite
    (``forward_torch``, the autograd path); a subclass gives both, ``hip_form()`` and ``compute_dtype``.

    One with a HIP backward also gives ``train_reasons`` and ``_stem_modules()`` (what ``hip_train_reason`` says in its
    own words), ``_output_name(i)`` and ``forward_hip(x, splits, state)`` (``state``, a dict, receives what the backward
    reads).  The rest has a default here for a backbone whose backward walks ``_sequence()`` (``[(kind, name, module)]``
    in forward order) in ``_backward_ops`` (a ``BackwardPlanBuilder``'s ``(ops, names, grads, keep)``), run as
    ``backward_struct`` ops by ``<backward_prefix>_run``: ``_trainable()`` (``[(name, tensor)]``: the autograd node's
    inputs), ``_first_trainable()``, the test hooks and ``_run_backward(state, shape, cotangents, splits)`` (``{name:
    fp32 gradient}``).  The ResNet, whose backward plan goes by tensor names, overrides them."""

    train_form = "torch"
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

    def set_dtype(self, dtype: torch.dtype):
        """Precision of the products: ``torch.float32`` (fp32 accuracy), ``torch.bfloat16`` or ``torch.float16`` (one
        16-bit product, fp32 accumulation, 16-bit GEMM operands between launches).  Outputs are fp32."""
        if dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError(f"{type(self).__name__}.set_dtype: {dtype} is not float32 / bfloat16 / float16")
        self.compute_dtype = dtype
        return self

    def _needs_autograd(self, x: Tensor) -> bool:
        if not torch.is_grad_enabled():
            return False
        return x.requires_grad or any(p.requires_grad for p in self.parameters())

    def forward(self, x: Tensor) -> Dict[str, Tensor]:
        if self.train_form == "hip" and self._needs_autograd(x):
            return self.forward_hip_train(x)
        if self._needs_autograd(x) or not self.hip_form():
            return self.forward_torch(x)
        return self.forward_hip(x)

    # ------------------------------------------------------------------------------------------ training in HIP
    def set_train_form(self, form: str):
        """How a forward that needs autograd runs: ``"torch"`` (default: the composite ``forward_torch``) or ``"hip"``
        (the HIP forward plan inside an autograd node whose backward is one plan too, see ``forward_hip_train``).
        ``"hip"`` on a module or input that is not eligible (``hip_train_reason``) raises at forward: it never falls
        back."""
        if form not in ("torch", "hip"):
            raise ValueError(f"{type(self).__name__}.set_train_form: {form!r} is not 'torch' / 'hip'")
        self.train_form = form
        return self

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

    def hip_train_form(self, x: Optional[Tensor] = None) -> bool:
        """True when ``set_train_form("hip")`` can train this module (on input ``x``): ``hip_form()``, a frozen stem, an
        input without gradient and a float32 / bfloat16 compute dtype."""
        return self.hip_train_reason(x) is None

    def forward_hip_train(self, x: Tensor, splits: int = 0) -> Dict[str, Tensor]:
        """The ``"hip"`` training form: the HIP forward plan as one autograd node.  The node keeps what the backward
        reads (the plan's own activations, no copy); its backward is one ``_run_backward`` call and returns the fp32
        parameter gradients to autograd, which accumulates them into ``.grad``."""
        reason = self.hip_train_reason(x)
        if reason is not None:
            raise RuntimeError(f"{type(self).__name__}: the 'hip' training form cannot run: {reason}")
        named = self._trainable()
        maps = _TrainFunction.apply(self, x, splits, tuple(n for n, _ in named), *[t for _, t in named])
        return dict(zip([self._output_name(i) for i in sorted(self.return_indices)], maps))

    def _train_state(self) -> dict:
        """What the last ``"hip"`` training forward stored; valid while that forward's autograd graph is alive."""
        state = self.__dict__.get("_train_state_ref")
        state = state() if state is not None else None
        if state is None:
            raise RuntimeError(f"{type(self).__name__}: no 'hip' training forward is alive")
        return state

    def _trainable(self) -> List[Tuple[str, Tensor]]:
        return [(n, p) for n, p in self.named_parameters() if p.requires_grad]

    def _first_trainable(self) -> Optional[int]:
        """The index in ``_sequence()`` of the lowest module with a trainable parameter: where the backward stops."""
        for idx, (_, _, m) in enumerate(self._sequence()):
            if any(p.requires_grad for p in m.parameters()):
                return idx
        return None

    def saved_activations(self) -> Dict[str, Tensor]:
        """Test hook (read-only): what the last ``"hip"`` training forward stored, by name (the backbone's module lists
        the names next to its ``_sequence``).  Valid while that forward's autograd graph is alive."""
        return dict(self._train_state()["acts"])

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
        ops, _, grads, keep = self._backward_ops(acts, state["factors"], shape, cotangents, splits)
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

    def _precision(self) -> int:
        return 0 if self.compute_dtype == torch.float32 else 1

    def _lib(self):
        return _hip.lib(self.compute_dtype if self.compute_dtype == torch.float16 else None)

    def _packed(self, layer: nn.Module, layout: int = 0, scale: Union[None, float, Tensor] = None, scale_bias: bool = True,
                pad_to: int = 1) -> Tuple[Tensor, Tensor]:
        """``(packed weight, bias)`` of a conv or Linear for the implicit GEMM (``sdetr_backbone_pack`` with a unit norm):
        ``scale`` (a layer scale, or a constant) folded into the weight and, with ``scale_bias``, the bias; a layer
        without a bias gets zeros; the output width zero-padded to a multiple of ``pad_to``.  Built once per parameter
        version, precision and compute dtype."""
        precision, lib = self._precision(), self._lib()
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
            zeros, ones = torch.zeros(cop, device=dev), torch.ones(cop, device=dev)
            nbytes = lib.sdetr_backbone_packed_bytes(cop, ci, k, precision)
            packed = torch.empty(nbytes // 2, dtype=torch.int16, device=dev)
            bias = torch.empty(cop, dtype=torch.float32, device=dev)
            _hip.launch("sdetr_backbone_pack", lib, dev, w32.data_ptr(), gamma.data_ptr(), beta.data_ptr(), zeros.data_ptr(),
                        ones.data_ptr(), 0.0, cop, ci, k, layout, precision, packed.data_ptr(), bias.data_ptr(),
                        what=f"{type(self).__name__} (pack)")
            return packed, bias
        sources = (w, layer.bias) + ((scale,) if isinstance(scale, Tensor) else ())
        fixed = None if isinstance(scale, Tensor) else scale
        return derived(layer, "rows_packed", sources, build,
                       extra=(precision, self.compute_dtype, layout, fixed, scale_bias, pad_to))

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
        precision, lib = self._precision(), self._lib()
        w = layer.weight

        def build():
            w32 = w.detach().to(torch.float32)
            if w32.dim() == 4:
                w32 = w32.permute(0, 2, 3, 1)
            w32 = w32.reshape(w.shape[0], -1).contiguous()
            co, ci = w32.shape
            gamma = torch.ones(co, device=w.device) if scale is None else scale.detach().to(torch.float32).reshape(co).contiguous()
            ones = torch.ones(co, device=w.device)
            packed = torch.empty(lib.sdetr_backbone_dgrad_packed_bytes(co, ci, 1, precision) // 2, dtype=torch.int16,
                                 device=w.device)
            unused = torch.empty(co, dtype=torch.float32, device=w.device)
            _hip.launch("sdetr_backbone_pack_dgrad", lib, w.device, w32.data_ptr(), gamma.data_ptr(), ones.data_ptr(), 0.0, co,
                        ci, 1, precision, packed.data_ptr(), unused.data_ptr(), what=f"{type(self).__name__} (pack dgrad)")
            return packed
        return derived(layer, "rows_packed_dgrad", (w, scale), build, extra=(precision, self.compute_dtype))

    def _f32(self, owner, name: str, t: Tensor) -> Tensor:
        """A parameter as a contiguous fp32 tensor, cached per version."""
        return derived(owner, "rows_f32_" + name, (t,), lambda: t.detach().to(torch.float32).contiguous().clone())

    def _run_plan(self, struct_type, c_prefix: str, ops: list, device) -> None:
        """Launch ``ops`` in order: ``<c_prefix>_run`` over a workspace of ``<c_prefix>_workspace_bytes``."""
        lib, precision, who = self._lib(), self._precision(), type(self).__name__
        arr = (struct_type * len(ops))(*ops)
        ws_bytes = getattr(lib, c_prefix + "_workspace_bytes")(arr, len(ops), precision)
        if ws_bytes < 0:
            _hip.check(-1, f"{who} (workspace)", lib)
        ws = torch.empty(max(int(ws_bytes), 16), dtype=torch.uint8, device=device)
        _hip.launch(c_prefix + "_run", lib, device, arr, len(ops), precision, ws.data_ptr(), ws_bytes, what=f"{who} (run)")
