"""Row N0 (DESIGN.md §4 "Backbone"): the ResNet backbone in front of ``ChannelMapper`` (reference
``models/backbones/resnet.py``, ``models/bricks/misc.py:9-57``), eval mode with ``FrozenBatchNorm2d``.

``ResNetBackbone(arch, weights=None, return_indices=(0, 1, 2, 3), freeze_indices=(), **kwargs)`` has the reference's
constructor, ``num_channels`` and state-dict keys: the reference's feature extractor keeps ``conv1``, ``bn1`` and
``layer1`` .. ``layer{max(return_indices) + 1}`` under their own names (no ``avgpool`` / ``fc``).  ``forward(x)`` returns ``{"layer{i + 1}": map}`` for
``i in return_indices``, fp32 NCHW.  ``weights`` is a state dict (optionally under ``"model"``) or a local file path:
nothing is ever downloaded (``weights=None`` keeps the random initialisation).  Loading is non-strict with shape
filtering, as the reference's ``util.utils.load_state_dict``; ``num_batches_tracked`` entries are dropped by
``FrozenBatchNorm2d``.

How it runs (inference: grad disabled, or nothing that requires grad) -- ``csrc/backbone.hip``:
  * every conv + its ``FrozenBatchNorm2d`` is ONE implicit-GEMM launch whose epilogue adds the folded bias, the residual
    and the ReLU; the weight is folded and packed once per parameter version (``derived``);
  * activations between layers are channels-last in the compute dtype; the last block of each returned stage also
    writes the stage's fp32 NCHW map; the stem reads the fp32 NCHW canvas; the max pool is a launch of its own;
  * the whole network is one precomputed plan (``build_plan``, filled through ``hip_module.PlanBuilder`` as the other
    backbones' are) handed to ``sdetr_backbone_run`` (one ctypes call per forward);
  * ``set_dtype``: fp32 (default) multiplies at fp32 accuracy (exact three-way bf16 split of both operands); bf16 /
    fp16 take one 16-bit product with fp32 accumulation and keep the activations in that type between layers.
The HIP path serves every ``groups == 1`` arch without dilation: resnet18/34/50/101/152 and wide_resnet50_2 / 101_2,
with or without deformable stages.  A DCN stage (``stage_with_dcn``, ``deform_conv.DeformConv2dPack`` as ``conv2``) is
two ops per block: the offset and mask convs as ONE exact conv (27 channels padded to 32, fp32 out, the three-way split
whatever ``set_dtype`` says: an offset is a coordinate), then the deformable product, whose A tile is the masked bilinear
gather and whose weight, epilogue and tiles are the plain conv's.  Grouped ResNeXt (with or without DCN), and by default every call with grad enabled on something that requires grad, take the
plain-torch composite (``F.conv2d`` + the frozen affine), which is also the default autograd path.  A CPU tensor on the
HIP form raises: the hot path has no CPU fallback.

Training in HIP (``set_train_form("hip")``, ``csrc/backbone_backward.hip``; the interface, its autograd node and
``_run_backward`` are ``backbone_base.HipBackbone``'s, this module gives ``_trainable``, the stored activations and
``_backward_ops``): a forward that needs autograd runs the same forward plan inside one autograd node; its backward is one
``sdetr_backbone_bwd_run`` call over ``build_backward_plan``:
one backward-data launch per conv whose input has a trainable conv upstream, one backward-weight launch per trainable
conv (plus the fixed-order reduction where a reduction is split), one ingest launch per returned map.  The stored
activations are the ReLU masks and the weight-gradient operands; no activation is copied.  Served: ``hip_form()``
archs with a frozen stem (``freeze_indices`` non-empty), an input without gradient, float32 or bfloat16; anything else
raises at forward.  Stem / max-pool backward, float16 training and the deformable backward are out of scope: a DCN conv
that is trainable, or that a gradient has to pass through (something trainable upstream of it), raises with that reason;
frozen DCN stages below the lowest trainable conv do not stand in the way.
"""
import ctypes
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Type, Union

import torch
from torch import Tensor, nn

from . import _hip
from .backbone_base import HipBackbone
from .deform_conv import DeformConv2dPack
from .derived import derived
from .hip_module import PlanBuilder


class FrozenBatchNorm2d(nn.Module):
    """BatchNorm2d with fixed statistics and affine (reference ``models/bricks/misc.py:9-57``)."""

    def __init__(self, num_features: int, eps: float = 1e-5):
        super().__init__()
        self.eps = eps
        self.register_buffer("weight", torch.ones(num_features))
        self.register_buffer("bias", torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        state_dict.pop(prefix + "num_batches_tracked", None)
        super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs)

    def forward(self, x: Tensor) -> Tensor:
        w = self.weight.reshape(1, -1, 1, 1)
        b = self.bias.reshape(1, -1, 1, 1)
        rv = self.running_var.reshape(1, -1, 1, 1)
        rm = self.running_mean.reshape(1, -1, 1, 1)
        scale = w * (rv + self.eps).rsqrt()
        bias = b - rm * scale
        return x * scale + bias

    def __repr__(self) -> str:
        return f"{self.__class__.__name__}({self.weight.shape[0]}, eps={self.eps})"


def conv3x3(in_planes: int, out_planes: int, stride: int = 1, groups: int = 1, dilation: int = 1) -> nn.Conv2d:
    return nn.Conv2d(in_planes, out_planes, kernel_size=3, stride=stride, padding=dilation, groups=groups, bias=False,
                     dilation=dilation)


def conv3x3_dcn(in_planes: int, out_planes: int, stride: int = 1, groups: int = 1, dilation: int = 1) -> DeformConv2dPack:
    return DeformConv2dPack(in_planes, out_planes, kernel_size=3, stride=stride, padding=dilation, groups=groups, bias=False,
                            dilation=dilation)


def _core(conv: nn.Module) -> nn.Module:
    """The module that holds a conv's geometry and main weight: a ``DeformConv2dPack``'s ``deform_conv2d``, else itself."""
    return conv.deform_conv2d if isinstance(conv, DeformConv2dPack) else conv


def conv1x1(in_planes: int, out_planes: int, stride: int = 1) -> nn.Conv2d:
    return nn.Conv2d(in_planes, out_planes, kernel_size=1, stride=stride, bias=False)


class BasicBlock(nn.Module):
    expansion: int = 1

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: Optional[nn.Module] = None, groups: int = 1,
                 base_width: int = 64, dilation: int = 1, norm_layer: Optional[Callable[..., nn.Module]] = None,
                 with_dcn: bool = False):
        super().__init__()
        norm_layer = norm_layer or FrozenBatchNorm2d
        if groups != 1 or base_width != 64:
            raise ValueError("BasicBlock only supports groups=1 and base_width=64")
        if dilation > 1:
            raise NotImplementedError("Dilation > 1 not supported in BasicBlock")
        self.conv1 = conv3x3(inplanes, planes, stride)
        self.bn1 = norm_layer(planes)
        self.relu = nn.ReLU(inplace=True)
        self.conv2 = conv3x3_dcn(planes, planes) if with_dcn else conv3x3(planes, planes)
        self.bn2 = norm_layer(planes)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x: Tensor) -> Tensor:
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        out += identity
        return self.relu(out)


class Bottleneck(nn.Module):
    expansion: int = 4

    def __init__(self, inplanes: int, planes: int, stride: int = 1, downsample: Optional[nn.Module] = None, groups: int = 1,
                 base_width: int = 64, dilation: int = 1, norm_layer: Optional[Callable[..., nn.Module]] = None,
                 with_dcn: bool = False):
        super().__init__()
        norm_layer = norm_layer or FrozenBatchNorm2d
        width = int(planes * (base_width / 64.0)) * groups
        self.conv1 = conv1x1(inplanes, width)
        self.bn1 = norm_layer(width)
        self.conv2 = (conv3x3_dcn if with_dcn else conv3x3)(width, width, stride, groups, dilation)
        self.bn2 = norm_layer(width)
        self.conv3 = conv1x1(width, planes * self.expansion)
        self.bn3 = norm_layer(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward(self, x: Tensor) -> Tensor:
        identity = x if self.downsample is None else self.downsample(x)
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        out += identity
        return self.relu(out)


class ResNet(nn.Module):
    """The reference's ``ResNet`` without ``avgpool`` / ``fc`` (which its feature extractor drops); ``num_stages`` keeps
    only ``layer1`` .. ``layer{num_stages}``, as the extractor does for its deepest returned stage.  ``norm_layer``
    defaults to ``FrozenBatchNorm2d``."""

    def __init__(self, block: Type[Union[BasicBlock, Bottleneck]], layers: Sequence[int], num_classes: int = 1000,
                 zero_init_residual: bool = False, groups: int = 1, width_per_group: int = 64,
                 replace_stride_with_dilation: Optional[List[bool]] = None, stage_with_dcn: Optional[List[bool]] = None,
                 norm_layer: Optional[Callable[..., nn.Module]] = None, num_stages: int = 4):
        super().__init__()
        stage_with_dcn = stage_with_dcn or [False] * 4
        self._norm_layer = norm_layer = norm_layer or FrozenBatchNorm2d
        self.inplanes, self.dilation = 64, 1
        replace_stride_with_dilation = replace_stride_with_dilation or [False, False, False]
        if len(replace_stride_with_dilation) != 3:
            raise ValueError("replace_stride_with_dilation should be None or a 3-element tuple, "
                             f"got {replace_stride_with_dilation}")
        self.groups, self.base_width, self.block = groups, width_per_group, block
        self.conv1 = nn.Conv2d(3, self.inplanes, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = norm_layer(self.inplanes)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        for i in range(num_stages):
            setattr(self, f"layer{i + 1}", self._make_layer(block, 64 * 2 ** i, layers[i], stride=1 if i == 0 else 2,
                                                            dilate=i > 0 and replace_stride_with_dilation[i - 1],
                                                            with_dcn=stage_with_dcn[i]))
        self.num_stages = num_stages
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.GroupNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, Bottleneck):
                    nn.init.constant_(m.bn3.weight, 0)
                elif isinstance(m, BasicBlock):
                    nn.init.constant_(m.bn2.weight, 0)

    def _make_layer(self, block, planes: int, blocks: int, stride: int = 1, dilate: bool = False,
                    with_dcn: bool = False) -> nn.Sequential:
        norm_layer, downsample, previous_dilation = self._norm_layer, None, self.dilation
        if dilate:
            self.dilation *= stride
            stride = 1
        if stride != 1 or self.inplanes != planes * block.expansion:
            downsample = nn.Sequential(conv1x1(self.inplanes, planes * block.expansion, stride),
                                       norm_layer(planes * block.expansion))
        layers = [block(self.inplanes, planes, stride, downsample, self.groups, self.base_width, previous_dilation,
                        norm_layer, with_dcn)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, groups=self.groups, base_width=self.base_width,
                                dilation=self.dilation, norm_layer=norm_layer, with_dcn=with_dcn))
        return nn.Sequential(*layers)


ARCHS = {
    "resnet18": dict(block=BasicBlock, layers=(2, 2, 2, 2)),
    "resnet34": dict(block=BasicBlock, layers=(3, 4, 6, 3)),
    "resnet50": dict(block=Bottleneck, layers=(3, 4, 6, 3)),
    "resnet101": dict(block=Bottleneck, layers=(3, 4, 23, 3)),
    "resnet152": dict(block=Bottleneck, layers=(3, 8, 36, 3)),
    "resnext50_32x4d": dict(block=Bottleneck, layers=(3, 4, 6, 3), groups=32, width_per_group=4),
    "resnext101_32x4d": dict(block=Bottleneck, layers=(3, 4, 23, 3), groups=32, width_per_group=4),
    "resnext101_32x8d": dict(block=Bottleneck, layers=(3, 4, 23, 3), groups=32, width_per_group=8),
    "resnext101_64x4d": dict(block=Bottleneck, layers=(3, 4, 23, 3), groups=64, width_per_group=4),
    "wide_resnet50_2": dict(block=Bottleneck, layers=(3, 4, 6, 3), width_per_group=128),
    "wide_resnet101_2": dict(block=Bottleneck, layers=(3, 4, 23, 3), width_per_group=128),
}


def _out_hw(n: int, k: int, s: int, p: int) -> int:
    return (n + 2 * p - k) // s + 1


def plan_shapes(block, layers: Sequence[int], num_stages: int, height: int, width: int, width_per_group: int = 64
                ) -> List[Tuple[str, int, int, int]]:
    """``(name, channels, H, W)`` of the stem, the max pool and every stage's output for an ``H x W`` canvas."""
    h, w = _out_hw(height, 7, 2, 3), _out_hw(width, 7, 2, 3)
    shapes = [("stem", 64, h, w)]
    h, w = _out_hw(h, 3, 2, 1), _out_hw(w, 3, 2, 1)
    shapes.append(("maxpool", 64, h, w))
    for i in range(num_stages):
        if i > 0:
            h, w = _out_hw(h, 3, 2, 1), _out_hw(w, 3, 2, 1)   # the 3x3 / 1x1 stride-2 convs agree on this
        shapes.append((f"layer{i + 1}", 64 * 2 ** i * block.expansion, h, w))
    return shapes


class ResNetBackbone(HipBackbone):
    def __init__(self, arch: str, weights: Union[None, str, Dict[str, Tensor]] = None,
                 return_indices: Tuple[int, ...] = (0, 1, 2, 3), freeze_indices: Tuple[int, ...] = (), **kwargs):
        super().__init__()
        if arch not in ARCHS:
            raise ValueError(f"Expected architecture in {tuple(ARCHS)} but got {arch}")
        config = dict(ARCHS[arch])
        config.update({k: v for k, v in kwargs.items() if v is not None})
        config.pop("url", None)
        self.return_indices = tuple(return_indices)
        net = ResNet(num_stages=max(self.return_indices) + 1, **config)
        self.conv1, self.bn1, self.relu, self.maxpool = net.conv1, net.bn1, net.relu, net.maxpool
        self.num_stages = net.num_stages
        for i in range(net.num_stages):
            setattr(self, f"layer{i + 1}", getattr(net, f"layer{i + 1}"))
        self.block, self.groups, self.width_per_group = net.block, net.groups, net.base_width
        self.dilation = net.dilation
        self.num_channels = [64 * self.block.expansion * 2 ** i for i in self.return_indices]
        self.compute_dtype = torch.float32
        if weights is not None:
            self.load_weights(weights)
        if len(freeze_indices) > 0:
            for m in (self.conv1, self.bn1):
                self._freeze(m)
        for i in freeze_indices:
            self._freeze(getattr(self, f"layer{i + 1}"))

    def stages(self) -> List[nn.Sequential]:
        return [getattr(self, f"layer{i + 1}") for i in range(self.num_stages)]

    # ------------------------------------------------------------------------------------------ form checks
    def _convs(self):
        """Every conv of the network; a ``DeformConv2dPack`` is ONE conv (its ``deform_conv2d``; the offset and mask convs
        inside it are part of that conv's HIP form)."""
        yield self.conv1
        for stage in self.stages():
            for blk in stage:
                inner = {id(c) for m in blk.modules() if isinstance(m, DeformConv2dPack) for c in (m.conv_offset, m.conv_mask)}
                for m in blk.modules():
                    if isinstance(m, DeformConv2dPack):
                        yield m.deform_conv2d
                    elif isinstance(m, nn.Conv2d) and id(m) not in inner:
                        yield m

    def hip_form(self) -> bool:
        """True when every conv is one the HIP kernels serve (see the module docstring)."""
        if self.groups != 1 or self.dilation != 1:
            return False
        for c in self._convs():
            if c.groups != 1 or tuple(c.dilation) != (1, 1) or c.bias is not None:
                return False
            if not isinstance(c, nn.Conv2d) and (tuple(c.kernel_size) != (3, 3) or tuple(c.padding) != (1, 1)):
                return False   # (the deformable product is the 3x3 one)
            if c is not self.conv1 and (c.in_channels % 32 or c.out_channels % 8):
                return False
        norms = [self.bn1] + [m for stage in self.stages() for blk in stage for name, m in blk.named_modules()
                              if name in ("bn1", "bn2", "bn3", "downsample.1")]
        return all(isinstance(m, FrozenBatchNorm2d) for m in norms)

    # ------------------------------------------------------------------------------------------ forward
    def forward_torch(self, x: Tensor) -> Dict[str, Tensor]:
        """The differentiable composite (``F.conv2d`` + the frozen affine) on the input's device."""
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        outs = {}
        for i, stage in enumerate(self.stages()):
            x = stage(x)
            if i in self.return_indices:
                outs[f"layer{i + 1}"] = x
        return outs

    def _packed_conv_bn(self, conv: nn.Conv2d, bn: FrozenBatchNorm2d, layout: int) -> Tuple[Tensor, Tensor]:
        """``(packed weight, folded bias)`` of ``conv`` + ``bn`` (``sdetr_backbone_pack``), built once per parameter
        version, precision and compute dtype."""
        sources = (conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var)

        def build():
            f32 = [t.detach().to(torch.float32).contiguous() for t in sources]
            return self._pack(f32[0], f32[1:], float(bn.eps), layout)
        return derived(conv, "backbone_packed", sources, build,
                       extra=(float(bn.eps), self._precision(), self.compute_dtype, layout))

    def _packed_offset_mask(self, pack: DeformConv2dPack) -> Tuple[Tensor, Tensor]:
        """``(packed weight, bias [32])`` of ``conv_offset`` and ``conv_mask`` as one 3x3 conv: 18 + 9 channels, zero rows up
        to 32, the two biases as the folded bias (a unit norm); ALWAYS the three exact planes (precision 0).  Built once
        per parameter version."""
        off, msk = pack.conv_offset, pack.conv_mask
        sources = (off.weight, off.bias, msk.weight, msk.bias)

        def build():
            dev, n_off, n_msk = off.weight.device, off.out_channels, msk.out_channels
            w32 = torch.zeros((32, off.in_channels, 3, 3), dtype=torch.float32, device=dev)
            beta = torch.zeros(32, dtype=torch.float32, device=dev)
            w32[:n_off], w32[n_off:n_off + n_msk] = off.weight.detach().float(), msk.weight.detach().float()
            beta[:n_off], beta[n_off:n_off + n_msk] = off.bias.detach().float(), msk.bias.detach().float()
            unit = (torch.ones(32, device=dev), beta, torch.zeros(32, device=dev), torch.ones(32, device=dev))
            return self._pack(w32, unit, 0.0, 0, precision=0)
        return derived(pack, "backbone_packed_offset_mask", sources, build)

    def build_plan(self, x: Tensor, splits: int = 0, acts: Optional[Dict[str, Tensor]] = None):
        """The op list of one forward on ``x`` ``[B, 3, H, W]`` (fp32 NCHW on the device): ``(ops, outputs, keep, names)``:
        ``outputs`` the returned fp32 NCHW maps, ``keep`` every tensor the plan points into, ``names`` one label per op
        (``"conv1"``, ``"pool"``, ``"layer2.0.conv1"``, ``"layer2.0.downsample.0"`` ..).  ``acts`` (a dict) receives the
        channels-last output of every op under the op's name, in op order: what the training backward reads."""
        names = {id(m): n for n, m in self.named_modules() if isinstance(m, (nn.Conv2d, DeformConv2dPack))}
        act = torch.float32 if self._precision() == 0 else self.compute_dtype
        batch = x.shape[0]
        pb = PlanBuilder(_hip.BackboneOpStruct, x, batch=batch)
        new, keep, outputs = pb.new, pb.keep, pb.outputs

        def dcn_op(pack, bn, src, h, w, relu, residual=None, nchw_out=None):
            """A DCN conv: its offsets and mask logits (an exact conv, fp32 rows of 32), then the deformable product."""
            dc, name = pack.deform_conv2d, names[id(pack)]
            s = dc.stride[0]
            ho, wo = _out_hw(h, 3, s, 1), _out_hw(w, 3, s, 1)
            om_packed, om_bias = self._packed_offset_mask(pack)
            packed, bias = self._packed_conv_bn(dc, bn, 0)
            keep.extend((om_packed, om_bias, packed, bias))
            om = new((batch, ho, wo, 32), torch.float32)
            out = new((batch, ho, wo, dc.out_channels), act)
            if acts is not None:
                acts[name + ".offset"], acts[name] = om, out
            shape = dict(in_channels=dc.in_channels, height=h, width=w, kernel_size=3, stride=s, padding=1, x_nchw=0)
            pb.op(name + ".offset", 3, x=src.data_ptr(), weight=om_packed.data_ptr(), bias=om_bias.data_ptr(), out=om.data_ptr(),
                  out_channels=32, relu=0, splits=splits, **shape)
            pb.op(name, 2, x=src.data_ptr(), weight=packed.data_ptr(), bias=bias.data_ptr(), residual=_hip.ptr(residual),
                  out=out.data_ptr(), out_nchw=_hip.ptr(nchw_out), out_channels=dc.out_channels, relu=1 if relu else 0,
                  splits=0, offset_mask=om.data_ptr(), **shape)
            return out, ho, wo

        def conv_op(conv, bn, src, h, w, relu, residual=None, nchw_out=None, x_nchw=False):
            if isinstance(conv, DeformConv2dPack):
                return dcn_op(conv, bn, src, h, w, relu, residual, nchw_out)
            k, s, p = conv.kernel_size[0], conv.stride[0], conv.padding[0]
            ho, wo = _out_hw(h, k, s, p), _out_hw(w, k, s, p)
            packed, bias = self._packed_conv_bn(conv, bn, 1 if x_nchw else 0)
            keep.extend((packed, bias))
            out = new((batch, ho, wo, conv.out_channels), act)
            if acts is not None:
                acts[names[id(conv)]] = out
            pb.op(names[id(conv)], 0, x=src.data_ptr(), weight=packed.data_ptr(), bias=bias.data_ptr(),
                  residual=_hip.ptr(residual), out=out.data_ptr(), out_nchw=_hip.ptr(nchw_out), in_channels=conv.in_channels,
                  height=h, width=w, out_channels=conv.out_channels, kernel_size=k, stride=s, padding=p,
                  relu=1 if relu else 0, x_nchw=1 if x_nchw else 0, splits=splits)
            return out, ho, wo

        h, w = x.shape[2], x.shape[3]
        y, h, w = conv_op(self.conv1, self.bn1, x, h, w, True, x_nchw=True)
        ho, wo = _out_hw(h, 3, 2, 1), _out_hw(w, 3, 2, 1)
        pooled = new((batch, ho, wo, 64), act)
        if acts is not None:
            acts["pool"] = pooled
        pb.op("pool", 1, x=y.data_ptr(), out=pooled.data_ptr(), in_channels=64, height=h, width=w, out_channels=64,
              kernel_size=3, stride=2, padding=1)
        y, h, w = pooled, ho, wo
        for i, stage in enumerate(self.stages()):
            for j, blk in enumerate(stage):
                last = i in self.return_indices and j == len(stage) - 1
                nchw = None
                if last:
                    nchw = new((batch, self._block_out_channels(blk), _out_hw(h, 1, blk.stride, 0),
                                _out_hw(w, 1, blk.stride, 0)), torch.float32)
                    outputs[f"layer{i + 1}"] = nchw
                identity = y
                if blk.downsample is not None:
                    identity, _, _ = conv_op(blk.downsample[0], blk.downsample[1], y, h, w, False)
                t, th, tw = conv_op(blk.conv1, blk.bn1, y, h, w, True)
                if isinstance(blk, Bottleneck):
                    t, th, tw = conv_op(blk.conv2, blk.bn2, t, th, tw, True)
                    y, h, w = conv_op(blk.conv3, blk.bn3, t, th, tw, True, residual=identity, nchw_out=nchw)
                else:
                    y, h, w = conv_op(blk.conv2, blk.bn2, t, th, tw, True, residual=identity, nchw_out=nchw)
        return pb.ops, outputs, keep, pb.names

    @staticmethod
    def _block_out_channels(blk) -> int:
        return blk.conv3.out_channels if isinstance(blk, Bottleneck) else _core(blk.conv2).out_channels

    def forward_hip(self, x: Tensor, splits: int = 0, state: Optional[dict] = None) -> Dict[str, Tensor]:
        """``state`` (a dict): a training forward; it receives ``"acts"``, see ``build_plan``."""
        x = self._check_image(x)
        for t in self.buffers():
            _hip.require_device("ResNetBackbone", parameter=t.detach())
        acts = None if state is None else state.setdefault("acts", {})
        ops, outputs, keep, _ = self.build_plan(x, splits, acts)
        self._run_plan(_hip.BackboneOpStruct, "sdetr_backbone", ops, x.device)
        return outputs

    # ------------------------------------------------------------------------------------------ training in HIP
    # (the interface is HipBackbone's: the node keeps the plan's channels-last activations; its backward runs
    # ``_backward_ops`` with one ``sdetr_backbone_bwd_run`` call and returns the fp32 weight gradients)
    train_reasons = ("the architecture is not one the HIP kernels serve (grouped / dilated convs, a bias or a norm layer "
                     "other than FrozenBatchNorm2d)",
                     "the stem (conv1) is not frozen: the stem and max-pool backward are out of scope")
    dcn_train_reason = ("a deformable conv (DCN) stage is trainable or has something trainable upstream of it: the "
                        "deformable backward in HIP is out of scope (freeze the DCN stages and everything below them, or "
                        "train through the composite)")

    def _extra_train_reason(self) -> Optional[str]:
        """The DCN rule: no weight gradient of, and no data gradient through, a deformable conv."""
        upstream = False   # a trainable parameter below the current block
        for stage in self.stages():
            for blk in stage:
                if isinstance(blk.conv2, DeformConv2dPack) and (
                        upstream or blk.conv1.weight.requires_grad or any(p.requires_grad for p in blk.conv2.parameters())):
                    return self.dcn_train_reason
                upstream = upstream or any(p.requires_grad for p in blk.parameters())
        return None

    def _stem_modules(self):
        return self.conv1, self.bn1

    def _output_name(self, i: int) -> str:
        return f"layer{i + 1}"

    def _blocks(self, height: int, width: int):
        """Every residual block in forward order with its convs ``(name, conv, bn, in_h, in_w)``, its input tensor's name
        and whether that input needs a gradient (a trainable conv lies upstream of it)."""
        h, w = _out_hw(_out_hw(height, 7, 2, 3), 3, 2, 1), _out_hw(_out_hw(width, 7, 2, 3), 3, 2, 1)
        src, needs, src_returned = "pool", self.conv1.weight.requires_grad, False
        blocks = []
        for i, stage in enumerate(self.stages()):
            for j, blk in enumerate(stage):
                prefix = f"layer{i + 1}.{j}"
                chain, ch, cw = [], h, w
                for n in ("conv1", "conv2", "conv3") if isinstance(blk, Bottleneck) else ("conv1", "conv2"):
                    conv = _core(getattr(blk, n))
                    chain.append((f"{prefix}.{n}", conv, getattr(blk, "bn" + n[-1]), ch, cw))
                    ch, cw = (_out_hw(v, conv.kernel_size[0], conv.stride[0], conv.padding[0]) for v in (ch, cw))
                ds = None if blk.downsample is None else (f"{prefix}.downsample.0", blk.downsample[0], blk.downsample[1], h, w)
                returned = i in self.return_indices and j == len(stage) - 1
                blocks.append(dict(chain=chain, ds=ds, input=src, input_needs=needs, input_returned=src_returned,
                                   returned=f"layer{i + 1}" if returned else None, out_hw=(ch, cw)))
                needs = needs or any(c[1].weight.requires_grad for c in chain + ([ds] if ds else []))
                src, src_returned, h, w = chain[-1][0], returned, ch, cw
        return blocks

    def build_backward_plan(self, batch: int, height: int, width: int) -> List[dict]:
        """The backward of one forward on a ``[batch, 3, height, width]`` canvas as host data (no library, no tensors):
        dicts ``kind`` (``"ingest"`` / ``"wgrad"`` / ``"dgrad"``), ``conv`` (the module name, or the stage for an ingest),
        the operand NAMES ``dz``, ``x``, ``add``, ``mask``, ``out`` and the shape fields of ``sdetr_backbone_bwd_op``.
        Names: a stored activation is called after the op that wrote it (``"layer2.0.conv1"``, ``"pool"``); ``"cot:layerN"``
        is a returned map's incoming gradient, ``"dz:<op>"`` the gradient at that op's pre-activation, ``"raw:<op>"`` the
        unmasked gradient of a returned stage's output arriving from the next stage (its ingest adds and masks it),
        ``"tmp:<op>"`` a downsample branch's input gradient (the ``add`` of the block's first conv), ``"dw:<op>"`` the
        weight gradient.  One wgrad per trainable conv, one dgrad per conv whose input has a trainable conv upstream, one
        ingest per returned stage."""
        plan: List[dict] = []
        pending: Dict[str, str] = {}   # returned tensor -> the raw gradient the next stage produced

        def op(kind, rec, **names):
            name, conv, _, h, w = rec
            d = dict(kind=kind, conv=name, dz=None, x=None, add=None, mask=None, out=None, batch=batch,
                     in_channels=conv.in_channels, height=h, width=w, out_channels=conv.out_channels,
                     kernel_size=conv.kernel_size[0], stride=conv.stride[0], padding=conv.padding[0])
            d.update(names)
            plan.append(d)

        for blk in reversed(self._blocks(height, width)):
            chain, ds = blk["chain"], blk["ds"]
            out_name = chain[-1][0]
            trainable = any(c[1].weight.requires_grad for c in chain + ([ds] if ds else []))
            if blk["returned"] is not None and (trainable or blk["input_needs"]):
                channels = chain[-1][1].out_channels
                plan.append(dict(kind="ingest", conv=blk["returned"], dz="cot:" + blk["returned"], x=None,
                                 add=pending.get(out_name), mask=out_name, out="dz:" + out_name, batch=batch,
                                 in_channels=channels, height=blk["out_hw"][0], width=blk["out_hw"][1],
                                 out_channels=channels, kernel_size=1, stride=1, padding=0))
            if not (trainable or blk["input_needs"]):
                break   # nothing at or below this block has a trainable conv
            cur = "dz:" + out_name
            if ds is not None and ds[1].weight.requires_grad:
                op("wgrad", ds, dz=cur, x=blk["input"], out="dw:" + ds[0])
            for idx in reversed(range(len(chain))):
                rec = chain[idx]
                src = blk["input"] if idx == 0 else chain[idx - 1][0]
                if rec[1].weight.requires_grad:
                    op("wgrad", rec, dz=cur, x=src, out="dw:" + rec[0])
                if idx == 0:
                    if blk["input_needs"]:
                        add = "dz:" + out_name   # the identity branch
                        if ds is not None:
                            add = "tmp:" + ds[0]
                            op("dgrad", ds, dz="dz:" + out_name, out=add)
                        if blk["input_returned"]:
                            pending[src] = "raw:" + src
                            op("dgrad", rec, dz=cur, add=add, out="raw:" + src)
                        else:
                            op("dgrad", rec, dz=cur, add=add, mask=src, out="dz:" + src)
                elif blk["input_needs"] or any(c[1].weight.requires_grad for c in chain[:idx]):
                    op("dgrad", rec, dz=cur, mask=src, out="dz:" + src)
                    cur = "dz:" + src
                else:
                    break
        return plan

    def _packed_dgrad(self, conv: nn.Conv2d, bn: FrozenBatchNorm2d, with_weight: bool) -> Tuple[Optional[Tensor], Tensor]:
        """``(backward-data packed weight, s[out])`` of ``conv`` + ``bn`` (``sdetr_backbone_pack_dgrad``), built once per
        parameter version, precision and compute dtype; without ``with_weight`` only the scale."""
        sources = (conv.weight, bn.weight, bn.running_var)

        def build():
            return self._pack_dgrad(*[t.detach().to(torch.float32).contiguous() for t in sources], float(bn.eps), with_weight)
        return derived(conv, "backbone_packed_dgrad" if with_weight else "backbone_bn_scale", sources, build,
                       extra=(float(bn.eps), self._precision(), self.compute_dtype))

    def _trainable_convs(self) -> List[Tuple[str, nn.Conv2d]]:
        return [(n, m) for n, m in self.named_modules() if isinstance(m, nn.Conv2d) and m.weight.requires_grad]

    def _trainable(self) -> List[Tuple[str, Tensor]]:
        return [(n, m.weight) for n, m in self._trainable_convs()]

    def saved_activations(self) -> List[Tuple[str, Tensor]]:
        """Test hook (read-only): ``(op name, post-activation output [B, H, W, C] in the compute dtype)`` of every op with
        a ReLU, in op order (the stem first), as stored by the last ``"hip"`` training forward.  Valid while that
        forward's autograd graph is alive."""
        return [(n, t) for n, t in self._train_state()["acts"].items()
                if n != "pool" and ".downsample." not in n and not n.endswith(".offset")]

    backward_struct, backward_prefix = _hip.BackboneBwdOpStruct, "sdetr_backbone_bwd"

    def _backward_ops(self, acts: Dict[str, Tensor], factors, shape, cotangents: Dict[str, Optional[Tensor]], splits: int = 0):
        """The name records of ``build_backward_plan`` as ops on the stored activations: ``(ops, names, grads, keep)``,
        ``grads`` being ``{conv name: fp32 weight gradient}``."""
        batch, _, height, width = shape
        modules = dict(self.named_modules())
        act = torch.float32 if self._precision() == 0 else self.compute_dtype
        pb = PlanBuilder(_hip.BackboneBwdOpStruct, acts["pool"], batch=batch, splits=splits)
        tensors: Dict[str, Tensor] = dict(acts)
        grads: Dict[str, Tensor] = {}
        for d in self.build_backward_plan(batch, height, width):
            weight = scale = None
            rows = (batch, d["height"], d["width"], d["in_channels"])
            if d["kind"] == "ingest":
                g = cotangents.get(d["conv"])
                if g is None:
                    g = torch.zeros((batch, d["in_channels"], d["height"], d["width"]), device=pb.device)
                g = g.to(torch.float32).contiguous()
                pb.keep.append(g)
                tensors[d["dz"]] = g
                out = pb.new(rows, act)
            else:
                conv = modules[d["conv"]]
                bn = modules[d["conv"][:-len("conv1")] + "bn" + d["conv"][-1]] if ".downsample." not in d["conv"] \
                    else modules[d["conv"][:-1] + "1"]
                if d["kind"] == "wgrad":
                    scale = self._packed_dgrad(conv, bn, False)[1]
                    out = grads[d["conv"]] = pb.new(conv.weight.shape, torch.float32)
                else:
                    weight = self._packed_dgrad(conv, bn, True)[0]
                    out = pb.new(rows, act)
                pb.keep.append(scale if weight is None else weight)
            tensors[d["out"]] = out
            pb.op(f"{d['conv']} ({d['kind']})", {"dgrad": 0, "wgrad": 1, "ingest": 2}[d["kind"]], dz=tensors[d["dz"]].data_ptr(),
                  x=_hip.ptr(tensors.get(d["x"])), weight=_hip.ptr(weight), scale=_hip.ptr(scale),
                  add=_hip.ptr(tensors.get(d["add"])), mask=_hip.ptr(tensors.get(d["mask"])), out=out.data_ptr(),
                  **{f: d[f] for f in ("in_channels", "height", "width", "out_channels", "kernel_size", "stride", "padding")})
        return pb.ops, pb.names, grads, pb.keep


def batch_images(images: Sequence[Tensor], size_divisible: int = 32, normalize: bool = True,
                 resize: Optional[Tuple[int, Optional[int]]] = None) -> Tuple[Tensor, Tensor]:
    """ONE launch: ``images`` ``[3, h_i, w_i]`` (float in [0, 1], or uint8 read as ``v / 255``) normalised with the
    ImageNet mean / std and padded with 0 after normalisation into ``canvas`` ``[B, 3, Hp, Wp]`` (Hp, Wp = the largest
    size rounded up to ``size_divisible``) and ``mask`` ``[B, Hp, Wp]`` (bool, True on padding): the reference's eval
    ``ConvertImageDtype`` + ``Normalize`` + ``image_list_from_tensors`` + ``construct_mask``.  ``normalize=False`` (the
    reference's training mode, whose images arrive normalised from the dataset transforms: float32 only) only pads and
    builds the mask: the canvas equals the inputs bit for bit inside every image.

    ``resize=(min_size, max_size)`` puts the reference's ``EvalResize`` in front (``eval_resize.py``), still as ONE
    launch: every image is resized to ``eval_resize_size(h, w, min_size, max_size)`` with the antialiased bilinear filter
    (uint8: rounded to uint8 values first, as the reference's cast round trip), the canvas is sized from the RESIZED
    sizes, and no resized image exists in memory.  Bit for bit ``batch_images([EvalResize(*resize)(i) for i in images])``.
    Eval only: ``resize`` with ``normalize=False`` raises (the reference never resizes in training mode)."""
    if len(images) == 0:
        raise ValueError("batch_images: no images")
    if resize is not None and not normalize:
        raise ValueError("batch_images: resize is the eval transform's first step; it does not combine with "
                         "normalize=False (the reference never resizes in training mode)")
    dev, dt = images[0].device, images[0].dtype
    if dt not in (torch.float32, torch.uint8):
        raise RuntimeError(f"batch_images: images must be float32 or uint8, got {dt}")
    if not normalize and dt != torch.float32:
        raise RuntimeError(f"batch_images: normalize=False takes float32 images only, got {dt}")
    for im in images:
        if im.dim() != 3 or im.shape[0] != 3 or im.dtype != dt or im.device != dev:
            raise RuntimeError("batch_images: every image must be [3, h, w] of one dtype on one device")
        _hip.require_device("batch_images", image=im)
    if resize is not None:
        return _resize_batch_images(images, size_divisible, resize)
    hp = -(-max(int(im.shape[1]) for im in images) // size_divisible) * size_divisible
    wp = -(-max(int(im.shape[2]) for im in images) // size_divisible) * size_divisible
    canvas = torch.empty(len(images), 3, hp, wp, device=dev, dtype=torch.float32)
    mask = torch.empty(len(images), hp, wp, device=dev, dtype=torch.bool)
    ptrs = (ctypes.c_void_p * len(images))(*[im.data_ptr() for im in images])
    hw = (ctypes.c_int * (2 * len(images)))(*[int(v) for im in images for v in im.shape[1:]])
    _hip.launch("sdetr_backbone_batch_images_ex", None, dev, ptrs, hw, len(images), 1 if dt == torch.uint8 else 0,
                1 if normalize else 0, hp, wp, canvas.data_ptr(), mask.data_ptr(), what="batch_images")
    return canvas, mask


def _resize_batch_images(images: Sequence[Tensor], size_divisible: int, resize) -> Tuple[Tensor, Tensor]:
    """The fused form of ``batch_images`` (``sdetr_backbone_resize_batch_images``); ``images`` already checked."""
    from .eval_resize import MAX_IMAGES, eval_resize_size
    min_size, max_size = resize
    if len(images) > MAX_IMAGES:
        raise ValueError(f"batch_images: at most {MAX_IMAGES} images per call, got {len(images)}")
    dev, dt = images[0].device, images[0].dtype
    sizes = [eval_resize_size(im.shape[1], im.shape[2], min_size, max_size) for im in images]
    if any(nh < 1 or nw < 1 for nh, nw in sizes):
        raise ValueError(f"batch_images: resize={tuple(resize)} leaves an image without pixels (sizes {sizes})")
    hp = -(-max(nh for nh, _ in sizes) // size_divisible) * size_divisible
    wp = -(-max(nw for _, nw in sizes) // size_divisible) * size_divisible
    canvas = torch.empty(len(images), 3, hp, wp, device=dev, dtype=torch.float32)
    mask = torch.empty(len(images), hp, wp, device=dev, dtype=torch.bool)
    ptrs = (ctypes.c_void_p * len(images))(*[im.data_ptr() for im in images])
    hw = (ctypes.c_int * (2 * len(images)))(*[int(v) for im in images for v in im.shape[1:]])
    out_hw = (ctypes.c_int * (2 * len(images)))(*[v for s in sizes for v in s])
    _hip.launch("sdetr_backbone_resize_batch_images", None, dev, ptrs, hw, out_hw, len(images),
                1 if dt == torch.uint8 else 0, hp, wp, canvas.data_ptr(), mask.data_ptr(), what="batch_images (resize)")
    return canvas, mask
