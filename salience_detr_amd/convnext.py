"""The ConvNeXt backbone in front of ``ChannelMapper`` (reference ``models/backbones/convnext.py``): DESIGN.md §4
"ConvNeXt backbone".

``ConvNeXtBackbone(arch, weights=None, return_indices=(0, 1, 2, 3), freeze_indices=(), **kwargs)`` has the reference's
constructor, ``num_channels`` and state-dict keys (``features.0`` .. ``features.{2 * max(return_indices) + 1}``: what its
feature extractor keeps; no ``avgpool`` / ``classifier``).  ``arch`` is ``conv_t`` / ``conv_s`` / ``conv_b`` / ``conv_l``
or ``None`` with ``block_setting=[CNBlockConfig ..]`` (which also overrides an arch's), ``stochastic_depth_prob`` and
``layer_scale`` in ``kwargs``.  ``forward(x)`` returns ``{"features.{2 * i + 1}": map}`` for ``i in return_indices``, fp32
NCHW.  ``weights`` is a state dict (optionally under ``"model"``) or a local file path, loaded non-strictly with shape
filtering; nothing is ever downloaded (``weights=None`` keeps the reference's initialisation).

How it runs (inference: grad disabled, or nothing that requires grad) -- ``csrc/convnext.hip``, one precomputed plan, one
``sdetr_convnext_run`` call per forward:
  * stem: the 4x4 stride-4 patchify GEMM on the fp32 NCHW canvas, then a LayerNorm launch;
  * a block is THREE launches: depthwise 7x7 + bias + LayerNorm fused, Linear 1 with the GELU epilogue, Linear 2 with
    ``layer_scale`` folded into its weight and bias and the residual added in the epilogue (the last block of a returned
    stage also writes the stage's fp32 NCHW map);
  * a down-sampler is a LayerNorm launch and the 2x2 stride-2 patchify GEMM;
  * the residual stream is channels-last fp32 in every mode; ``set_dtype(bfloat16 | float16)`` takes one 16-bit product
    with fp32 accumulation and keeps the GEMM A operands (normalised rows, the hidden rows) in that type, ``float32``
    (default) multiplies at fp32 accuracy (exact three-way bf16 split of both operands).
A call with grad enabled on something that requires grad takes the plain-torch composite (``F.conv2d``,
``F.layer_norm``, ``F.linear``, ``F.gelu``, row-mode stochastic depth), which is the autograd path; ConvNeXt backward in
HIP is out of scope.  A CPU tensor on the HIP form raises: the hot path has no CPU fallback.
"""
from functools import partial
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import _hip
from .backbone_base import HipBackbone, Permute, PlanBuilder, StochasticDepth  # noqa: F401 (both modules re-exported)
from .derived import derived


class LayerNorm2d(nn.LayerNorm):
    """LayerNorm over the channels of an NCHW map."""

    def forward(self, x: Tensor) -> Tensor:
        x = x.permute(0, 2, 3, 1)
        x = F.layer_norm(x, self.normalized_shape, self.weight, self.bias, self.eps)
        return x.permute(0, 3, 1, 2)


class CNBlock(nn.Module):
    def __init__(self, dim: int, layer_scale: float, stochastic_depth_prob: float,
                 norm_layer: Optional[Callable[..., nn.Module]] = None):
        super().__init__()
        if norm_layer is None:
            norm_layer = partial(nn.LayerNorm, eps=1e-6)
        self.block = nn.Sequential(
            nn.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim, bias=True),
            Permute([0, 2, 3, 1]),
            norm_layer(dim),
            nn.Linear(in_features=dim, out_features=4 * dim, bias=True),
            nn.GELU(),
            nn.Linear(in_features=4 * dim, out_features=dim, bias=True),
            Permute([0, 3, 1, 2]),
        )
        self.layer_scale = nn.Parameter(torch.ones(dim, 1, 1) * layer_scale)
        self.stochastic_depth = StochasticDepth(stochastic_depth_prob, "row")

    def forward(self, input: Tensor) -> Tensor:
        result = self.layer_scale * self.block(input)
        result = self.stochastic_depth(result)
        result += input
        return result


class CNBlockConfig:
    """One stage: ``input_channels``, the ``out_channels`` of the down-sampler after it (``None``: none), ``num_layers``."""

    def __init__(self, input_channels: int, out_channels: Optional[int], num_layers: int):
        self.input_channels = input_channels
        self.out_channels = out_channels
        self.num_layers = num_layers

    def __repr__(self) -> str:
        return (f"{self.__class__.__name__}(input_channels={self.input_channels}, out_channels={self.out_channels}, "
                f"num_layers={self.num_layers})")


class ConvNeXt(nn.Module):
    """The reference's ``ConvNeXt`` without ``avgpool`` / ``classifier`` (which its feature extractor drops);
    ``num_stages`` keeps ``features.0`` .. ``features.{2 * num_stages - 1}``.  The stochastic-depth probabilities count
    the blocks of the WHOLE ``block_setting``, as the reference's do."""

    def __init__(self, block_setting: List[CNBlockConfig], stochastic_depth_prob: float = 0.0, layer_scale: float = 1e-6,
                 num_classes: int = 1000, block: Optional[Callable[..., nn.Module]] = None,
                 norm_layer: Optional[Callable[..., nn.Module]] = None, num_stages: Optional[int] = None, **kwargs: Any):
        super().__init__()
        if not block_setting:
            raise ValueError("The block_setting should not be empty")
        if not (isinstance(block_setting, Sequence) and all(isinstance(s, CNBlockConfig) for s in block_setting)):
            raise TypeError("The block_setting should be List[CNBlockConfig]")
        block = block or CNBlock
        norm_layer = norm_layer or partial(LayerNorm2d, eps=1e-6)
        num_stages = len(block_setting) if num_stages is None else num_stages
        first = block_setting[0].input_channels
        layers: List[nn.Module] = [nn.Sequential(nn.Conv2d(3, first, kernel_size=4, stride=4, padding=0, bias=True),
                                                 norm_layer(first))]
        total_stage_blocks = sum(cnf.num_layers for cnf in block_setting)
        stage_block_id = 0
        for i, cnf in enumerate(block_setting):
            if i >= num_stages:   # (dropped by the feature extractor: only its blocks' share of the depth counts)
                stage_block_id += cnf.num_layers
                continue
            stage: List[nn.Module] = []
            for _ in range(cnf.num_layers):
                sd_prob = stochastic_depth_prob * stage_block_id / (total_stage_blocks - 1.0) if total_stage_blocks > 1 else 0.0
                stage.append(block(cnf.input_channels, layer_scale, sd_prob))
                stage_block_id += 1
            layers.append(nn.Sequential(*stage))
            if cnf.out_channels is not None and i < num_stages - 1:
                layers.append(nn.Sequential(norm_layer(cnf.input_channels),
                                            nn.Conv2d(cnf.input_channels, cnf.out_channels, kernel_size=2, stride=2)))
        self.features = nn.Sequential(*layers)
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)


def _setting(*rows) -> List[CNBlockConfig]:
    return [CNBlockConfig(*r) for r in rows]


ARCHS = {
    "conv_t": dict(block_setting=_setting((96, 192, 3), (192, 384, 3), (384, 768, 9), (768, None, 3)),
                   stochastic_depth_prob=0.1),
    "conv_s": dict(block_setting=_setting((96, 192, 3), (192, 384, 3), (384, 768, 27), (768, None, 3)),
                   stochastic_depth_prob=0.4),
    "conv_b": dict(block_setting=_setting((128, 256, 3), (256, 512, 3), (512, 1024, 27), (1024, None, 3)),
                   stochastic_depth_prob=0.5),
    "conv_l": dict(block_setting=_setting((192, 384, 3), (384, 768, 3), (768, 1536, 27), (1536, None, 3)),
                   stochastic_depth_prob=0.5),
}
MAX_CHANNELS = 3072   # the depthwise + LayerNorm tile (csrc/convnext.hip)


class ConvNeXtBackbone(HipBackbone):
    def __init__(self, arch: Optional[str], weights: Union[None, str, Dict[str, Tensor]] = None,
                 return_indices: Tuple[int, ...] = (0, 1, 2, 3), freeze_indices: Tuple[int, ...] = (), **kwargs):
        super().__init__()
        if arch is not None and arch not in ARCHS:
            raise ValueError(f"Expected architecture in {tuple(ARCHS)} but got {arch}")
        config = dict(ARCHS[arch]) if arch is not None else {}
        config.update({k: v for k, v in kwargs.items() if v is not None})
        config.pop("url", None)
        if "block_setting" not in config:
            raise ValueError("ConvNeXtBackbone: arch=None needs block_setting=[CNBlockConfig, ...]")
        self.return_indices = tuple(return_indices)
        self.block_setting = list(config["block_setting"])
        if not self.return_indices or max(self.return_indices) >= len(self.block_setting) or min(self.return_indices) < 0:
            raise ValueError(f"ConvNeXtBackbone: return_indices {self.return_indices} do not fit "
                             f"{len(self.block_setting)} stages")
        self.num_stages = max(self.return_indices) + 1
        net = ConvNeXt(num_stages=self.num_stages, **config)
        self.features = net.features
        self.num_channels = [self.block_setting[i].input_channels for i in self.return_indices]
        self.compute_dtype = torch.float32
        if weights is not None:
            self.load_weights(weights)
        if len(freeze_indices) > 0:
            self._freeze(self.features[0])
        for i in freeze_indices:
            self._freeze(self.features[2 * i + 1])
            if 2 * i + 2 < len(self.features):
                self._freeze(self.features[2 * i + 2])

    def stages(self) -> List[nn.Sequential]:
        return [self.features[2 * i + 1] for i in range(self.num_stages)]

    # ------------------------------------------------------------------------------------------ form checks
    def hip_form(self) -> bool:
        """True when every layer is one the HIP kernels serve: the reference's own blocks (``CNBlock`` with
        ``nn.LayerNorm``, ``LayerNorm2d`` in the stem and the down-samplers) at widths that are multiples of 32."""
        for i, stage in enumerate(self.stages()):
            c = self.block_setting[i].input_channels
            if c % 32 or c > MAX_CHANNELS:
                return False
            for blk in stage:
                if type(blk) is not CNBlock or type(blk.block[2]) is not nn.LayerNorm:
                    return False
        norms = [self.features[0][1]] + [self.features[2 * i + 2][0] for i in range(self.num_stages - 1)]
        return all(type(m) is LayerNorm2d for m in norms)

    def forward_torch(self, x: Tensor) -> Dict[str, Tensor]:
        """The differentiable composite (the holder modules themselves) on the input's device."""
        outs = {}
        for idx, layer in enumerate(self.features):
            x = layer(x)
            if idx % 2 == 1 and idx // 2 in self.return_indices:
                outs[f"features.{idx}"] = x
        return outs

    def _taps(self, conv: nn.Conv2d) -> Tuple[Tensor, Tensor]:
        """The depthwise taps tap-major ``[49, C]`` and the bias, fp32."""
        def build():
            c = conv.weight.shape[0]
            return (conv.weight.detach().to(torch.float32).reshape(c, 49).t().contiguous(),
                    conv.bias.detach().to(torch.float32).contiguous())
        return derived(conv, "convnext_taps", (conv.weight, conv.bias), build)

    def build_plan(self, x: Tensor, splits: int = 0):
        """The op list of one forward on ``x`` ``[B, 3, H, W]`` (fp32 NCHW on the device): ``(ops, outputs, keep, names)``:
        ``outputs`` the returned fp32 NCHW maps, ``keep`` every tensor the plan points into, ``names`` one label per op."""
        act = torch.float32 if self._precision() == 0 else self.compute_dtype
        batch = x.shape[0]
        pb = PlanBuilder(_hip.ConvnextOpStruct, x, batch=batch, kernel_size=1, stride=1)
        new, keep, outputs = pb.new, pb.keep, pb.outputs

        def gemm(name, kind, layer, src, h, w, ci, k, scale=None, residual=None, nchw=None, x_nchw=False):
            packed, bias = self._packed(layer, 1 if x_nchw else 0, scale)
            keep.extend((packed, bias))
            co, ho, wo = layer.weight.shape[0], (h - k) // k + 1, (w - k) // k + 1
            out = new((batch, ho, wo, co), act if kind == 1 else torch.float32)
            pb.op(name, kind, x=src.data_ptr(), weight=packed.data_ptr(), bias=bias.data_ptr(), residual=_hip.ptr(residual),
                  out=out.data_ptr(), out_nchw=_hip.ptr(nchw), in_channels=ci, height=h, width=w, out_channels=co,
                  kernel_size=k, stride=k, x_nchw=1 if x_nchw else 0, splits=splits)
            return out, ho, wo

        def layer_norm(name, norm, src, h, w, c, out_f32):
            out = new((batch, h, w, c), torch.float32 if out_f32 else act)
            pb.layer_norm(name, 3, self._affine(norm), norm.eps, src, out, h, w, c, out_f32)
            return out

        h, w = x.shape[2], x.shape[3]
        stem = self.features[0]
        y, h, w = gemm("features.0.0", 0, stem[0], x, h, w, 3, 4, x_nchw=True)
        c = stem[0].weight.shape[0]
        y = layer_norm("features.0.1", stem[1], y, h, w, c, True)
        for i, stage in enumerate(self.stages()):
            for j, blk in enumerate(stage):
                prefix = f"features.{2 * i + 1}.{j}"
                dw, norm, fc1, fc2 = blk.block[0], blk.block[2], blk.block[3], blk.block[5]
                taps, dw_bias = self._taps(dw)
                gamma, beta = self._affine(norm)
                keep.extend((taps, dw_bias, gamma, beta))
                rows = new((batch, h, w, c), act)
                pb.op(prefix + ".block.0+2", 2, x=y.data_ptr(), weight=taps.data_ptr(), bias=dw_bias.data_ptr(),
                      gamma=gamma.data_ptr(), beta=beta.data_ptr(), out=rows.data_ptr(), in_channels=c, height=h, width=w,
                      out_channels=c, kernel_size=7, eps=float(norm.eps))
                hidden, _, _ = gemm(prefix + ".block.3", 1, fc1, rows, h, w, c, 1)
                nchw = None
                if i in self.return_indices and j == len(stage) - 1:
                    nchw = new((batch, c, h, w), torch.float32)
                    outputs[f"features.{2 * i + 1}"] = nchw
                y, _, _ = gemm(prefix + ".block.5", 0, fc2, hidden, h, w, 4 * c, 1, scale=blk.layer_scale, residual=y,
                               nchw=nchw)
            if i < self.num_stages - 1:
                down = self.features[2 * i + 2]
                t = layer_norm(f"features.{2 * i + 2}.0", down[0], y, h, w, c, False)
                y, h, w = gemm(f"features.{2 * i + 2}.1", 0, down[1], t, h, w, c, 2)
                c = down[1].weight.shape[0]
        return pb.ops, outputs, keep, pb.names

    def forward_hip(self, x: Tensor, splits: int = 0) -> Dict[str, Tensor]:
        if x.dtype != torch.float32:
            x = x.float()
        _hip.require_device("ConvNeXtBackbone", x=x)
        for t in self.parameters():
            _hip.require_device("ConvNeXtBackbone", parameter=t.detach())
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError(f"ConvNeXtBackbone: expected [B, 3, H, W], got {tuple(x.shape)}")
        if min(x.shape[2], x.shape[3]) < 4 * 2 ** (self.num_stages - 1):
            raise RuntimeError(f"ConvNeXtBackbone: a {tuple(x.shape[2:])} canvas leaves a stage without pixels")
        ops, outputs, keep, _ = self.build_plan(x, splits)
        self._run_plan(_hip.ConvnextOpStruct, "sdetr_convnext", ops, x.device)
        return outputs
