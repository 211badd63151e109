"""What every module with a HIP form shares, backbone or not: ``HipModule``, the module base with the precision switch,
the training-form switch (``set_train_form``, ``hip_train_form``), the launch of a plan (``_run_plan``), the two
``sdetr_backbone_pack*`` launches and the stored state of a ``"hip"`` training forward; the one autograd node behind every
``forward_hip_train``; ``PlanBuilder``, the op list a ``build_plan`` fills, with the stochastic-depth draw; and
``BackwardPlanBuilder``, the op list, gradients, scratch buffers and shared emitters a backward plan fills.

A module with a ``"hip"`` training form gives ``hip_train_reason(inputs)`` (the reasons are its own), a
``forward_hip_train`` that opens with ``_check_train_form`` and applies ``_TrainFunction``, and the node's two hooks:
``_train_forward(inputs, splits, state)`` (the tuple of outputs; ``state`` receives what the backward reads, as detached
aliases where that is a returned map) and ``_train_backward(state, cotangents, wanted, splits)`` (``({parameter name: fp32
gradient}, input gradients)``)."""
import weakref
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import Tensor, nn

from . import _hip


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

    def draw(self, sd: nn.Module, batch: int, training_forward: bool) -> Optional[Tensor]:
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
    """Every ``forward_hip_train``: the first ``n_inputs`` of ``tensors`` are the differentiable inputs, the rest the
    trainable parameters ``names``; outputs are the returned fp32 maps."""

    @staticmethod
    def forward(ctx, module: "HipModule", n_inputs: int, splits: int, names: Tuple[str, ...], *tensors: Tensor):
        state = _TrainState()
        outputs = module._train_forward(tensors[:n_inputs], splits, state)
        ctx.module, ctx.state, ctx.names, ctx.splits, ctx.n_inputs = module, state, names, splits, n_inputs
        module.__dict__["_train_state_ref"] = weakref.ref(state)
        return outputs

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *cotangents):
        wanted = ctx.needs_input_grad[4:4 + ctx.n_inputs]
        grads, dxs = ctx.module._train_backward(ctx.state, cotangents, wanted, ctx.splits)
        return (None, None, None, None) + tuple(dxs) + tuple(None if n not in grads else grads[n].contiguous() for n in ctx.names)


class HipModule(nn.Module):
    """A module with a HIP inference form and, opt-in, a HIP training form (see the module docstring); a subclass sets
    ``compute_dtype`` and gives ``hip_form()``."""

    train_form = "torch"

    def set_dtype(self, dtype: torch.dtype):
        """Precision of the products: ``torch.float32`` (fp32 accuracy), ``torch.bfloat16`` or ``torch.float16`` (one
        16-bit product, fp32 accumulation, 16-bit GEMM operands between launches).  Outputs are fp32."""
        if dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError(f"{type(self).__name__}.set_dtype: {dtype} is not float32 / bfloat16 / float16")
        self.compute_dtype = dtype
        return self

    def _precision(self) -> int:
        return 0 if self.compute_dtype == torch.float32 else 1

    def _lib(self):
        return _hip.lib(self.compute_dtype if self.compute_dtype == torch.float16 else None)

    def _needs_autograd(self, *tensors: Tensor) -> bool:
        if not torch.is_grad_enabled():
            return False
        return any(t.requires_grad for t in tensors) or any(p.requires_grad for p in self.parameters())

    # ------------------------------------------------------------------------------------------ training in HIP
    def set_train_form(self, form: str):
        """How a forward that needs autograd runs: ``"torch"`` (default: the composite ``forward_torch``) or ``"hip"``
        (the HIP forward inside an autograd node whose backward is one plan, see ``forward_hip_train``).  ``"hip"`` on a
        module or input that is not eligible (``hip_train_reason``) raises at forward: it never falls back."""
        if form not in ("torch", "hip"):
            raise ValueError(f"{type(self).__name__}.set_train_form: {form!r} is not 'torch' / 'hip'")
        self.train_form = form
        return self

    def hip_train_form(self, inputs=None) -> bool:
        """True when ``set_train_form("hip")`` can train this module (on ``inputs``): ``hip_train_reason`` has nothing to say."""
        return self.hip_train_reason(inputs) is None

    def _check_train_form(self, inputs) -> None:
        reason = self.hip_train_reason(inputs)
        if reason is not None:
            raise RuntimeError(f"{type(self).__name__}: the 'hip' training form cannot run: {reason}")

    def _train_state(self) -> dict:
        """What the last ``"hip"`` training forward stored; valid while that forward's autograd graph is alive."""
        state = self.__dict__.get("_train_state_ref")
        state = state() if state is not None else None
        if state is None:
            raise RuntimeError(f"{type(self).__name__}: no 'hip' training forward is alive")
        return state

    def saved_activations(self) -> Dict[str, Tensor]:
        """Test hook (read-only): what the last ``"hip"`` training forward stored, by name (the module lists the names
        where it stores them).  Valid while that forward's autograd graph is alive."""
        return dict(self._train_state()["acts"])

    # ------------------------------------------------------------------------------------------ launches
    def _run_plan(self, struct_type, c_prefix: str, ops: list, device) -> None:
        """Launch ``ops`` in order: ``<c_prefix>_run`` over a workspace of ``<c_prefix>_workspace_bytes``."""
        lib, precision, who = self._lib(), self._precision(), type(self).__name__
        arr = (struct_type * len(ops))(*ops)
        ws_bytes = getattr(lib, c_prefix + "_workspace_bytes")(arr, len(ops), precision)
        if ws_bytes < 0:
            _hip.check(-1, f"{who} (workspace)", lib)
        ws = torch.empty(max(int(ws_bytes), 16), dtype=torch.uint8, device=device)
        _hip.launch(c_prefix + "_run", lib, device, arr, len(ops), precision, ws.data_ptr(), ws_bytes, what=f"{who} (run)")

    def _pack(self, w32: Tensor, norm: Sequence[Tensor], eps: float, layout: int, precision: Optional[int] = None
              ) -> Tuple[Tensor, Tensor]:
        """``sdetr_backbone_pack`` of the fp32 conv weight ``w32`` ``[out, in, k, k]`` and the fp32 batch-norm vectors
        ``norm`` (weight, bias, running mean, running variance): ``(packed weight, folded bias [out])``.  ``precision``:
        the module's own unless given (0: the three exact planes whatever the compute dtype)."""
        lib, (co, ci, k) = self._lib(), w32.shape[:3]
        precision = self._precision() if precision is None else precision
        packed = torch.empty(lib.sdetr_backbone_packed_bytes(co, ci, k, precision) // 2, dtype=torch.int16, device=w32.device)
        bias = torch.empty(co, dtype=torch.float32, device=w32.device)
        _hip.launch("sdetr_backbone_pack", lib, w32.device, w32.data_ptr(), *[t.data_ptr() for t in norm], eps, co, ci, k,
                    layout, precision, packed.data_ptr(), bias.data_ptr(), what=f"{type(self).__name__} (pack)")
        return packed, bias

    def _pack_dgrad(self, w32: Tensor, gamma: Tensor, var: Tensor, eps: float, with_weight: bool = True
                    ) -> Tuple[Optional[Tensor], Tensor]:
        """``sdetr_backbone_pack_dgrad`` of the fp32 weight ``w32`` ``[out, in, k, k]`` (a Linear's: ``k == 1``) and the
        fp32 vectors ``gamma`` / ``var``: ``(backward-data planes, s[out] = gamma / sqrt(var + eps))``; without
        ``with_weight`` only the scale."""
        lib, precision, co, ci = self._lib(), self._precision(), w32.shape[0], w32.shape[1]
        k = w32.shape[2] if w32.dim() == 4 else 1
        packed = None
        if with_weight:
            packed = torch.empty(lib.sdetr_backbone_dgrad_packed_bytes(co, ci, k, precision) // 2, dtype=torch.int16,
                                 device=w32.device)
        scale = torch.empty(co, dtype=torch.float32, device=w32.device)
        _hip.launch("sdetr_backbone_pack_dgrad", lib, w32.device, w32.data_ptr(), gamma.data_ptr(), var.data_ptr(), eps, co,
                    ci, k, precision, _hip.ptr(packed), scale.data_ptr(), what=f"{type(self).__name__} (pack dgrad)")
        return packed, scale
