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
read fp32 / packed copies of them).  Anything else, and every call with grad enabled on something that requires grad (training), takes
the differentiable plain-torch composite on the device (``F.conv2d`` + ``F.group_norm``): it is the autograd path of this
row (there is no HIP backward of the mapper).  A CPU tensor on the HIP form raises: the hot path has no CPU fallback.
"""
from functools import partial
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor, nn

from . import _hip
from .derived import derived


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


class ChannelMapper(nn.Module):
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

    def set_dtype(self, dtype: torch.dtype):
        """Precision of the convolutions' products: ``torch.float32`` (fp32 accuracy), ``torch.bfloat16`` or
        ``torch.float16`` (one 16-bit product, fp32 accumulation).  Parameters, statistics and output stay fp32."""
        if dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise ValueError(f"ChannelMapper.set_dtype: {dtype} is not float32 / bfloat16 / float16")
        self.compute_dtype = dtype
        return self

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

    def _needs_autograd(self, inputs: Sequence[Tensor]) -> bool:
        if not torch.is_grad_enabled():
            return False
        return any(p.requires_grad for p in self.parameters()) or any(x.requires_grad for x in inputs)

    # ------------------------------------------------------------------------------------------ forward
    def forward(self, inputs: Union[Dict[str, Tensor], Sequence[Tensor]]) -> List[Tensor]:
        inputs = list(inputs.values()) if isinstance(inputs, dict) else list(inputs)
        assert len(inputs) == len(self.in_channels)
        if self._needs_autograd(inputs) or not self.hip_form():
            return self.forward_torch(inputs)
        return self.forward_hip(inputs)

    def forward_torch(self, inputs: Sequence[Tensor]) -> List[Tensor]:
        """The differentiable composite (training and every configuration outside the HIP form), on the inputs' device."""
        outs = [self.convs[i](inputs[i]) for i in range(len(inputs))]
        for i in range(len(inputs), len(self.convs)):
            outs.append(self.convs[i](inputs[-1] if i == len(inputs) else outs[-1]))
        return outs

    def _precision(self) -> int:
        return 0 if self.compute_dtype == torch.float32 else 1

    def _lib(self):
        return _hip.lib(self.compute_dtype if self.compute_dtype == torch.float16 else None)

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

    def _run(self, levels: List["_hip.FrontendLevelStruct"], batch: int, device) -> None:
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
        _hip.launch("sdetr_frontend_groupnorm", lib, device, arr, n, batch, self.out_channels, gn.num_groups,
                    gn.eps, ws.data_ptr(), ws_bytes, what="ChannelMapper (groupnorm)")

    def forward_hip(self, inputs: Sequence[Tensor]) -> List[Tensor]:
        xs = []
        for x in inputs:
            if x.dtype != torch.float32:
                x = x.float()
            _hip.require_device("ChannelMapper", x=x)
            xs.append(x)
        for p in self.parameters():
            _hip.require_device("ChannelMapper", parameter=p.detach())
        batch, dev = xs[0].shape[0], xs[0].device
        if any(x.shape[0] != batch for x in xs):
            raise RuntimeError("ChannelMapper: inputs of different batch sizes")
        for x, c in zip(xs, self.in_channels):
            if x.dim() != 4 or x.shape[1] != c:
                raise RuntimeError(f"ChannelMapper: expected [B, {c}, H, W], got {tuple(x.shape)}")
        co, nin = self.out_channels, len(xs)
        outs = [torch.empty(batch, co, x.shape[2], x.shape[3], device=dev, dtype=torch.float32) for x in xs]
        levels = [self._level(i, x, o) for i, (x, o) in enumerate(zip(xs, outs))]
        src = xs[-1]
        for i in range(nin, len(self.convs)):
            h, w = (src.shape[2] - 1) // 2 + 1, (src.shape[3] - 1) // 2 + 1
            out = torch.empty(batch, co, h, w, device=dev, dtype=torch.float32)
            levels.append(self._level(i, src, out))
            outs.append(out)
            if i > nin:   # reads the previous extra level after its GroupNorm: a call of its own
                self._run(levels[:-1], batch, dev)
                levels = levels[-1:]
            src = out
        self._run(levels, batch, dev)
        return outs
