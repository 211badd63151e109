"""Row N7 of DESIGN.md section 1b: the ChannelMapper neck between the backbone and the transformer
(reference ``models/necks/channel_mapper.py``).

Same constructor, ``num_channels``, ``init_weights`` (xavier) and state-dict keys as the reference, so its checkpoints
load unchanged: ``convs.{i}.0.weight`` (the convolution), ``convs.{i}.1.weight`` / ``convs.{i}.1.bias`` (the norm).  The
``nn.Conv2d`` / ``nn.GroupNorm`` objects below only HOLD those parameters.

How it runs (inference: grad disabled, or nothing that requires grad):
  * every backbone level (bias-free 1x1 conv + ``GroupNorm``) and the first extra level (bias-free 3x3 stride-2 pad-1
    conv of the last backbone map + ``GroupNorm``) are TWO launches (``csrc/frontend.hip``): one convolution launch for
    all levels, whose 1x1 epilogue writes NCHW and the GroupNorm partials and whose 3x3 level is split over the
    reduction; one GroupNorm launch that merges the partials in a fixed order and normalises every level in place;
  * a further extra level reads the previous NORMALISED level: two more launches per level;
  * ``set_dtype``: fp32 (default) multiplies at fp32 accuracy (exact three-way bf16 split); bf16 / fp16 take one
    16-bit product with fp32 accumulation, statistics and output (the reference's autocast numerics, where GroupNorm
    runs in fp32).  The output is fp32 NCHW in every mode: it goes straight into ``SalienceTransformer.forward``.
The HIP path serves the form every reference config uses: ``kernel_size=1, stride=1, groups=1, dilation=1``,
``GroupNorm`` with ``out_channels % num_groups == 0``, no activation, no conv bias, every input width a multiple of 32
(``out_channels`` too when a second extra level reads it), on HIP tensors, parameters of any float dtype (the kernels
read fp32 / packed copies of them).  Anything else, and by default every call with grad enabled on something that requires
grad (training), takes the differentiable plain-torch composite on the device (``F.conv2d`` + ``F.group_norm``), the default
autograd path of this row.  A CPU tensor on the HIP form raises: the hot path has no CPU fallback.

Training in HIP (``set_train_form("hip")``, ``csrc/frontend_backward.hip``; the interface, its autograd node and the plan
runner are ``hip_module.HipModule``'s, as the backbones' are): a forward that needs autograd runs the same convolution launches and ``sdetr_frontend_groupnorm_train`` -- the inference GroupNorm, bit for
bit, which also keeps the raw convolution ``z`` and every group's (mean, rstd) -- inside ONE autograd node over the backbone
maps and the trainable parameters.  Its backward is one ``sdetr_frontend_bwd_run`` plan (``build_backward_plan``), levels
from the last to the first: the GroupNorm backward (from ``z`` and the statistics, never from the output: gamma may be
zero), the backbone's backward-weight and backward-data kernels on its channels-last result, and one egest per input that
requires grad, back to fp32 NCHW.  Stored: ``z``, the statistics and the inputs themselves (no copy; an input that is not
dense fp32 NCHW -- a torch-form ConvNeXt hands out channels-last maps -- is copied once, in the inference form too, and the
copy is what is stored and read; its gradient comes back dense, in the input's shape).  Served:
``hip_form()``, ``out_channels % 8 == 0``, float32 or bfloat16, HIP tensors; anything else raises at forward with the reason
(``hip_train_reason``), it never falls back.
"""
import ctypes
from functools import partial
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor, nn

from . import _hip
from .derived import derived
from .hip_module import BackwardPlanBuilder, HipModule, _TrainFunction


class _ConvNormActivation(nn.Sequential):
    """Parameter holder with the reference's layout (``models/bricks/misc.py:61-158``): ``0`` = convolution, ``1`` =
    norm, then the activation.  ``bias=None`` means a conv bias only when there is no norm, as the reference."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int, stride: int, padding: int, groups: int,
                 norm_layer, activation_layer, dilation: int, inplace: Optional[bool], bias: Optional[bool]):
        if bias is None:
            bias = norm_layer is None
        layers: List[nn.Module] = [nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, dilation=dilation,
                                             groups=groups, bias=bias)]
        if norm_layer is not None:
            layers.append(norm_layer(out_channels))
        if activation_layer is not None:
            layers.append(activation_layer(**({} if inplace is None else {"inplace": inplace})))
        super().__init__(*layers)
        self.out_channels = out_channels


class ChannelMapper(HipModule):
    def __init__(self, in_channels: List[int], out_channels: int, num_outs: int, kernel_size: int = 1, stride: int = 1,
                 groups: int = 1, norm_layer=partial(nn.GroupNorm, 32), activation_layer: nn.Module = None,
                 dilation: int = 1, inplace: bool = True, bias: bool = None):
        self.in_channels = in_channels
        super().__init__()
        self.convs = nn.ModuleList()
        self.num_channels = [out_channels] * num_outs
        common = dict(groups=groups, norm_layer=norm_layer, activation_layer=activation_layer, dilation=dilation,
                      inplace=inplace, bias=bias)
        in_channel = None
        for in_channel in in_channels:
            self.convs.append(_ConvNormActivation(in_channel, out_channels, kernel_size, stride, (kernel_size - 1) // 2,
                                                  **common))
        for _ in range(num_outs - len(in_channels)):
            self.convs.append(_ConvNormActivation(in_channel, out_channels, 3, 2, 1, **common))
            in_channel = out_channels
        self.out_channels = out_channels
        self.kernel_size, self.stride, self.groups, self.dilation = kernel_size, stride, groups, dilation
        self.compute_dtype = torch.float32
        self.init_weights()

    def init_weights(self):
        for layer in self.modules():
            if isinstance(layer, nn.Conv2d):
                nn.init.xavier_uniform_(layer.weight, gain=1)
                if layer.bias is not None:
                    nn.init.constant_(layer.bias, 0)

    # ------------------------------------------------------------------------------------------ form checks
    def hip_form(self) -> bool:
        """True when the configuration is the one the HIP kernels serve (see the module docstring)."""
        if self.kernel_size != 1 or self.stride != 1 or self.groups != 1 or self.dilation != 1:
            return False
        if any(c % 32 for c in self.in_channels):
            return False
        groups = None
        for block in self.convs:
            if len(block) != 2 or block[0].bias is not None or not isinstance(block[1], nn.GroupNorm):
                return False
            gn = block[1]
            if not gn.affine or gn.num_channels != self.out_channels or self.out_channels % gn.num_groups:
                return False
            if groups is not None and (gn.num_groups, gn.eps) != groups:
                return False
            groups = (gn.num_groups, gn.eps)
        if len(self.convs) > len(self.in_channels) + 1 and self.out_channels % 32:
            return False   # a second extra level reads out_channels channels
        return len(self.convs) >= len(self.in_channels) and len(self.in_channels) < 8   # <= 8 levels per launch

    # ------------------------------------------------------------------------------------------ forward
    def forward(self, inputs: Union[Dict[str, Tensor], Sequence[Tensor]]) -> List[Tensor]:
        inputs = list(inputs.values()) if isinstance(inputs, dict) else list(inputs)
        assert len(inputs) == len(self.in_channels)
        if self.train_form == "hip" and self._needs_autograd(*inputs):
            return self.forward_hip_train(inputs)
        if self._needs_autograd(*inputs) or not self.hip_form():
            return self.forward_torch(inputs)
        return self.forward_hip(inputs)

    def forward_torch(self, inputs: Sequence[Tensor]) -> List[Tensor]:
        """The differentiable composite (training and every configuration outside the HIP form), on the inputs' device."""
        outs = [self.convs[i](inputs[i]) for i in range(len(inputs))]
        for i in range(len(inputs), len(self.convs)):
            outs.append(self.convs[i](inputs[-1] if i == len(inputs) else outs[-1]))
        return outs

    def _packed_weight(self, i: int) -> Tensor:
        """Conv weight of level ``i`` packed for the kernel (``sdetr_frontend_pack_weight``: three bf16 planes of the exact
        split in fp32 mode, one 16-bit plane otherwise), built once per parameter version and precision."""
        conv = self.convs[i][0]
        w = conv.weight
        precision, lib = self._precision(), self._lib()

        def build():
            src = w.detach().to(torch.float32).contiguous()
            nbytes = lib.sdetr_frontend_packed_bytes(src.numel(), precision)
            out = torch.empty(nbytes // 2, dtype=torch.int16, device=src.device)
            _hip.launch("sdetr_frontend_pack_weight", lib, src.device, src.data_ptr(), src.numel(), precision,
                        out.data_ptr(), what="ChannelMapper (pack weight)")
            return out
        return derived(conv, "frontend_packed_weight", (w,), build, extra=(precision, self.compute_dtype))

    def _affine(self, i: int) -> Tuple[Tensor, Tensor]:
        """GroupNorm's gamma / beta as the fp32 vectors the kernel reads, whatever the parameters' dtype."""
        gn = self.convs[i][1]
        return derived(gn, "frontend_affine", (gn.weight, gn.bias),
                       lambda: (gn.weight.detach().to(torch.float32).contiguous(),
                                gn.bias.detach().to(torch.float32).contiguous()))

    def _level(self, i: int, x: Tensor, out: Tensor) -> "_hip.FrontendLevelStruct":
        gamma, beta = self._affine(i)
        return _hip.FrontendLevelStruct(x.data_ptr(), self._packed_weight(i).data_ptr(), x.shape[1], x.shape[2],
                                        x.shape[3], self.convs[i][0].kernel_size[0], out.data_ptr(), gamma.data_ptr(),
                                        beta.data_ptr())

    def _run(self, levels: List["_hip.FrontendLevelStruct"], batch: int, device, kept: Sequence[Tensor] = ()) -> None:
        """One convolution launch and one GroupNorm launch over ``levels``; ``kept`` (``z`` and ``stats`` of every level,
        in level order) makes it the training forward's GroupNorm."""
        n = len(levels)
        arr = (_hip.FrontendLevelStruct * n)(*levels)
        gn = self.convs[0][1]
        lib = self._lib()
        ws_bytes = lib.sdetr_frontend_workspace_bytes(arr, n, batch, self.out_channels)
        if ws_bytes < 0:
            _hip.check(-1, "ChannelMapper (workspace)", lib)
        ws = torch.empty(max(int(ws_bytes), 1), dtype=torch.uint8, device=device)
        precision = self._precision()
        _hip.launch("sdetr_frontend_conv", lib, device, arr, n, batch, self.out_channels, precision, ws.data_ptr(),
                    ws_bytes, what="ChannelMapper (conv)")
        if kept:
            z = (ctypes.c_void_p * n)(*[t.data_ptr() for t in kept[0::2]])
            stats = (ctypes.c_void_p * n)(*[t.data_ptr() for t in kept[1::2]])
            _hip.launch("sdetr_frontend_groupnorm_train", lib, device, arr, n, batch, self.out_channels, gn.num_groups,
                        gn.eps, ws.data_ptr(), ws_bytes, z, stats, what="ChannelMapper (groupnorm, training)")
        else:
            _hip.launch("sdetr_frontend_groupnorm", lib, device, arr, n, batch, self.out_channels, gn.num_groups,
                        gn.eps, ws.data_ptr(), ws_bytes, what="ChannelMapper (groupnorm)")

    def _check_inputs(self, inputs: Sequence[Tensor]) -> List[Tensor]:
        """The inputs as the kernels read them: fp32, dense NCHW, on the device.  A map of another dtype or in other
        strides (a torch-form backbone hands out channels-last maps) is copied; a contiguous fp32 one is taken as it is."""
        xs = []
        for x in inputs:
            if x.dtype != torch.float32:
                x = x.float()
            if not x.is_contiguous():
                x = x.contiguous()
            _hip.require_device("ChannelMapper", x=x)
            xs.append(x)
        for p in self.parameters():
            _hip.require_device("ChannelMapper", parameter=p.detach())
        if any(x.shape[0] != xs[0].shape[0] for x in xs):
            raise RuntimeError("ChannelMapper: inputs of different batch sizes")
        for x, c in zip(xs, self.in_channels):
            if x.dim() != 4 or x.shape[1] != c:
                raise RuntimeError(f"ChannelMapper: expected [B, {c}, H, W], got {tuple(x.shape)}")
        return xs

    def build_plan(self, xs: Sequence[Tensor], state: Optional[dict] = None):
        """The forward over the checked fp32 inputs ``xs`` as host data: ``(calls, outs, keep)``.  A call is ``(levels,
        kept)``: the levels of one convolution + GroupNorm launch pair (a further extra level reads the previous
        NORMALISED level: a call of its own) and, with ``state`` (the training forward), their ``z`` / ``stats`` buffers in
        level order; ``state["acts"]`` receives what the backward reads, by name: ``input.<i>`` (the inputs themselves, no
        copy), ``convs.<i>.z``, ``convs.<i>.stats`` and, of an extra level that a further one reads, ``convs.<i>.out`` (the
        normalised map, the next level's input)."""
        batch, dev, co, nin = xs[0].shape[0], xs[0].device, self.out_channels, len(xs)
        groups = self.convs[0][1].num_groups
        acts = None if state is None else state.setdefault("acts", {})
        outs: List[Tensor] = []
        calls: List[Tuple[list, List[Tensor]]] = [([], [])]
        keep: List[Tensor] = list(xs)
        for i in range(len(self.convs)):
            src = xs[i] if i < nin else (xs[-1] if i == nin else outs[-1])
            h, w = (src.shape[2], src.shape[3]) if i < nin else ((src.shape[2] - 1) // 2 + 1, (src.shape[3] - 1) // 2 + 1)
            out = torch.empty(batch, co, h, w, device=dev, dtype=torch.float32)
            if i > nin:
                calls.append(([], []))
            calls[-1][0].append(self._level(i, src, out))
            keep.extend((out, self._packed_weight(i)) + self._affine(i))
            if acts is not None:
                z = torch.empty_like(out)
                stats = torch.empty(batch, groups, 2, device=dev, dtype=torch.float32)
                calls[-1][1].extend((z, stats))
                keep.extend((z, stats))
                acts[f"convs.{i}.z"], acts[f"convs.{i}.stats"] = z, stats
                if i < nin:
                    acts[f"input.{i}"] = src
                elif i < len(self.convs) - 1:
                    # (an alias without autograd history: the returned map itself would tie the autograd node, which
                    # owns this state, into a reference cycle with its own output)
                    acts[f"convs.{i}.out"] = out.detach()
            outs.append(out)
        return calls, outs, keep

    def forward_hip(self, inputs: Sequence[Tensor], state: Optional[dict] = None) -> List[Tensor]:
        xs = self._check_inputs(inputs)
        calls, outs, _ = self.build_plan(xs, state)
        for levels, kept in calls:
            self._run(levels, xs[0].shape[0], xs[0].device, kept)
        return outs

    # ------------------------------------------------------------------------------------------ training in HIP
    # (the interface is HipModule's; the backward of the node is one ``sdetr_frontend_bwd_run`` plan)
    def hip_train_reason(self, inputs: Optional[Sequence[Tensor]] = None) -> Optional[str]:
        """Why the ``"hip"`` training form cannot serve this module (and ``inputs``); ``None`` when it can."""
        if not self.hip_form():
            return ("the configuration is not one the HIP kernels serve (a 1x1 stride-1 ungrouped bias-free conv + affine "
                    "GroupNorm per level, every input width a multiple of 32)")
        if self.out_channels % 8:
            return f"out_channels {self.out_channels} is not a multiple of 8 (the backward-data and backward-weight kernels)"
        if self.compute_dtype not in (torch.float32, torch.bfloat16):
            return f"compute dtype {self.compute_dtype} is not float32 / bfloat16 (float16 has no loss scaling here)"
        if inputs is not None and any(not x.is_cuda for x in inputs):
            return "an input is a CPU tensor: the hot path has no CPU fallback"
        return None

    def forward_hip_train(self, inputs: Sequence[Tensor], splits: int = 0) -> List[Tensor]:
        """The ``"hip"`` training form: ``forward_hip`` with the training GroupNorm as one autograd node over the inputs
        and the trainable parameters.  The node keeps the raw convolutions ``z``, the (mean, rstd) of every group and the
        inputs (no copy); its backward is one plan and returns fp32 gradients, which autograd accumulates."""
        inputs = list(inputs.values()) if isinstance(inputs, dict) else list(inputs)
        self._check_train_form(inputs)
        named = [(n, p) for n, p in self.named_parameters() if p.requires_grad]
        return list(_TrainFunction.apply(self, len(inputs), splits, tuple(n for n, _ in named), *inputs, *[p for _, p in named]))

    def _train_forward(self, inputs: Sequence[Tensor], splits: int, state: dict) -> Tuple[Tensor, ...]:
        """(The stored names are ``build_plan``'s.)"""
        return tuple(self.forward_hip(inputs, state))

    def _packed_dgrad(self, i: int) -> Tensor:
        """The backward-data planes of level ``i``'s conv weight (``sdetr_backbone_pack_dgrad`` with a unit scale), built
        once per parameter version and precision."""
        conv = self.convs[i][0]
        w = conv.weight

        def build():
            w32 = w.detach().to(torch.float32).contiguous()
            ones = torch.ones(w.shape[0], device=w.device)
            return self._pack_dgrad(w32, ones, ones, 0.0)[0]
        return derived(conv, "frontend_packed_dgrad", (w,), build, extra=(self._precision(), self.compute_dtype))

    def build_backward_plan(self, acts: Dict[str, Tensor], cotangents: Sequence[Optional[Tensor]],
                            input_grads: Sequence[bool], splits: int = 0):
        """The backward of one training forward as ``sdetr_frontend_bwd_op`` ops (kinds: 0 dgrad, 1 wgrad, 2 rows, 3
        GroupNorm backward, 4 egest): ``(ops, names, grads, input_grads, keep)``.  Levels run from the last to the first,
        so that an extra level's backward-data result reaches the level below (``add``) before that level's GroupNorm
        backward.  Per level: the GroupNorm backward; for a trainable conv weight the input as channels-last rows (once per
        input: the last backbone map feeds two levels) and the backward-weight; the backward-data where something below
        wants a gradient.  An input that requires grad gets one egest, which adds its two backward-data results where it
        has two.  ``grads``: ``{parameter name: fp32 tensor}``; ``input_grads``: fp32 NCHW tensors, ``None`` where not asked."""
        nin, n_levels = len(self.in_channels), len(self.convs)
        xs = [acts[f"input.{i}"] for i in range(nin)]
        batch, co, act = xs[0].shape[0], self.out_channels, self.compute_dtype
        b = BackwardPlanBuilder(_hip.FrontendBwdOpStruct, xs[0], batch=batch, splits=splits)
        b.keep.extend(xs[1:])
        rows: Dict[int, Tensor] = {}                    # the channels-last copy of a level's input, by level of the source
        parts: List[List[Tensor]] = [[] for _ in xs]    # the backward-data results an input's gradient is the sum of
        add: Optional[Tensor] = None                    # what the level above hands to this level's normalised output
        trainable_below = [any(p.requires_grad for blk in self.convs[nin:i] for p in blk.parameters()) or input_grads[-1]
                           for i in range(n_levels)]
        for i in reversed(range(n_levels)):
            conv, gn = self.convs[i]
            name, k = f"convs.{i}", conv.kernel_size[0]
            src = xs[i] if i < nin else (xs[-1] if i == nin else acts[f"convs.{i - 1}.out"])
            src_key = min(i, nin - 1) if i <= nin else -i
            ci, h, w = src.shape[1], src.shape[2], src.shape[3]
            z, stats = acts[name + ".z"], acts[name + ".stats"]
            ho, wo = z.shape[2], z.shape[3]
            want_dx = trainable_below[i] if i > nin else input_grads[min(i, nin - 1)]
            above, add = add, None
            if not (want_dx or b.want(conv.weight, gn.weight, gn.bias)):
                continue
            cot = cotangents[i]
            cot = torch.zeros_like(z) if cot is None else cot.to(torch.float32).contiguous()
            gamma = self._affine(i)[0]
            b.keep.extend((cot, z, stats, gamma, src))
            affine = b.want(gn.weight, gn.bias)
            dgamma = b.new((co,), torch.float32) if affine else None
            dbeta = b.new((co,), torch.float32) if affine else None
            dz = b.new((batch, ho, wo, co), act)
            b.op(name + " (group norm)", 3, dz=cot.data_ptr(), add=_hip.ptr(above), z=z.data_ptr(), stats=stats.data_ptr(),
                 gamma=gamma.data_ptr(), out=dz.data_ptr(), dgamma=_hip.ptr(dgamma), dbeta=_hip.ptr(dbeta), height=ho, width=wo,
                 out_channels=co, groups=gn.num_groups, eps=float(gn.eps))
            if b.want(gn.weight):
                b.grads[name + ".1.weight"] = dgamma
            if b.want(gn.bias):
                b.grads[name + ".1.bias"] = dbeta
            shape = dict(in_channels=ci, height=h, width=w, out_channels=co, kernel_size=k)
            if b.want(conv.weight):
                if src_key not in rows:
                    rows[src_key] = b.new((batch, h, w, ci), act)
                    b.op(name + " (rows)", 2, x=src.data_ptr(), out=rows[src_key].data_ptr(), in_channels=ci, height=h, width=w)
                dw = b.grad(name + ".0.weight", tuple(conv.weight.shape), conv.weight)
                b.op(name + " (wgrad)", 1, dz=dz.data_ptr(), x=rows[src_key].data_ptr(), scale=b.ones(co).data_ptr(),
                     out=dw.data_ptr(), **shape)
            if want_dx:
                packed = self._packed_dgrad(i)
                b.keep.append(packed)
                dx = b.new((batch, h, w, ci), act)
                b.op(name + " (dgrad)", 0, dz=dz.data_ptr(), weight=packed.data_ptr(), out=dx.data_ptr(), **shape)
                if i > nin:
                    add = dx
                else:
                    parts[min(i, nin - 1)].append(dx)
        dxs: List[Optional[Tensor]] = []
        for j, x in enumerate(xs):
            if not parts[j]:
                dxs.append(None)
                continue
            dxs.append(b.new(tuple(x.shape), torch.float32))
            b.op(f"input.{j} (egest)", 4, dz=parts[j][0].data_ptr(), add=_hip.ptr(parts[j][1] if len(parts[j]) > 1 else None),
                 out=dxs[-1].data_ptr(), in_channels=x.shape[1], height=x.shape[2], width=x.shape[3])
        return b.ops, b.names, b.grads, dxs, b.keep

    def _run_backward(self, state: dict, cotangents: Sequence[Optional[Tensor]], input_grads: Sequence[bool], splits: int = 0):
        """Runs the backward plan on what the forward stored: ``({parameter name: fp32 gradient}, input gradients)``."""
        ops, _, grads, dxs, keep = self.build_backward_plan(state["acts"], cotangents, input_grads, splits)
        if ops:
            self._run_plan(_hip.FrontendBwdOpStruct, "sdetr_frontend_bwd", ops, keep[0].device)
        return grads, dxs

    _train_backward = _run_backward   # the autograd node's hook takes exactly these
