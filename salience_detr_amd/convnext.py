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
By default a call with grad enabled on something that requires grad takes the plain-torch composite (``F.conv2d``,
``F.layer_norm``, ``F.linear``, ``F.gelu``, row-mode stochastic depth), which is the default autograd path.  A CPU tensor
on the HIP form raises: the hot path has no CPU fallback.

Training in HIP (``set_train_form("hip")``, ``csrc/convnext_backward.hip``; the interface and its autograd node are
``backbone_base.HipBackbone``'s, as are ``_trainable``, ``_first_trainable``, the test hooks and ``_run_backward``; this
module gives ``_sequence``, the stored state and ``_backward_ops``, its own kinds next to the emitters of the base's
``BackwardPlanBuilder``): a forward that needs autograd runs the same plan inside one autograd node, with three
additions to its launches (``aux`` / ``row_scale`` of ``sdetr_convnext_op``): the depthwise launch also stores its fp32 values before the LayerNorm, Linear 1
its values before the GELU, and Linear 2 multiplies by the block's stochastic-depth factor per sample (drawn on the
device exactly as ``StochasticDepth`` draws it).  The backward is one ``sdetr_convnext_bwd_run`` call over ``_backward_ops``: it stops below the lowest trainable
module and returns fp32 gradients for the parameters that require them.  Served: ``hip_form()`` with a frozen stem, an
input without gradient, float32 or bfloat16.  The stem's backward, a gradient to the image and float16 training are out
of scope; anything else raises at forward.
"""
from functools import partial
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import _hip
from .backbone_base import HipBackbone
from .backbone_base import Permute, StochasticDepth  # noqa: F401 (both modules re-exported)
from .derived import derived
from .hip_module import BackwardPlanBuilder, PlanBuilder


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

    def build_plan(self, x: Tensor, splits: int = 0, train: Optional[dict] = None):
        """The op list of one forward on ``x`` ``[B, 3, H, W]`` (fp32 NCHW on the device): ``(ops, outputs, keep, names)``:
        ``outputs`` the returned fp32 NCHW maps, ``keep`` every tensor the plan points into, ``names`` one label per op.
        ``train`` (a dict with ``"first"``, the index in ``_sequence()`` of the lowest module whose backward will run):
        a training forward; it receives ``"acts"`` (what the backward reads, by op name) and ``"factors"`` (the
        stochastic-depth factors ``[B]`` of every block that drew some, by block name)."""
        act = torch.float32 if self._precision() == 0 else self.compute_dtype
        batch = x.shape[0]
        pb = PlanBuilder(_hip.ConvnextOpStruct, x, batch=batch, kernel_size=1, stride=1)
        new, keep, outputs = pb.new, pb.keep, pb.outputs

        acts: Dict[str, Tensor] = {}
        factors: Dict[str, Tensor] = {}
        if train is not None:
            train["acts"], train["factors"] = acts, factors
        index = 0   # of the current module in _sequence()

        def gemm(name, kind, layer, src, h, w, ci, k, scale=None, residual=None, nchw=None, x_nchw=False, aux=None,
                 row_scale=None):
            packed, bias = self._packed(layer, 1 if x_nchw else 0, scale)
            keep.extend((packed, bias))
            co, ho, wo = layer.weight.shape[0], (h - k) // k + 1, (w - k) // k + 1
            out = new((batch, ho, wo, co), act if kind == 1 else torch.float32)
            pb.op(name, kind, x=src.data_ptr(), weight=packed.data_ptr(), bias=bias.data_ptr(), residual=_hip.ptr(residual),
                  out=out.data_ptr(), out_nchw=_hip.ptr(nchw), in_channels=ci, height=h, width=w, out_channels=co,
                  kernel_size=k, stride=k, x_nchw=1 if x_nchw else 0, splits=splits, aux=_hip.ptr(aux),
                  row_scale=_hip.ptr(row_scale))
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
                stored = train is not None and index >= train["first"]
                pre_norm = new((batch, h, w, c), torch.float32) if stored else None
                pre_gelu = new((batch, h, w, 4 * c), act) if stored else None
                factor = pb.draw(blk.stochastic_depth, batch, train is not None)
                if factor is not None:
                    factors[prefix] = factor.view(batch)
                pb.op(prefix + ".block.0+2", 2, x=y.data_ptr(), weight=taps.data_ptr(), bias=dw_bias.data_ptr(),
                      gamma=gamma.data_ptr(), beta=beta.data_ptr(), out=rows.data_ptr(), in_channels=c, height=h, width=w,
                      out_channels=c, kernel_size=7, eps=float(norm.eps), aux=_hip.ptr(pre_norm))
                hidden, _, _ = gemm(prefix + ".block.3", 1, fc1, rows, h, w, c, 1, aux=pre_gelu)
                nchw = None
                if i in self.return_indices and j == len(stage) - 1:
                    nchw = new((batch, c, h, w), torch.float32)
                    outputs[f"features.{2 * i + 1}"] = nchw
                if stored:
                    acts.update({prefix + ".in": y, prefix + ".block.0": pre_norm, prefix + ".block.2": rows,
                                 prefix + ".block.3": pre_gelu, prefix + ".block.4": hidden})
                y, _, _ = gemm(prefix + ".block.5", 0, fc2, hidden, h, w, 4 * c, 1, scale=blk.layer_scale, residual=y,
                               nchw=nchw, row_scale=factor)
                index += 1
            if i < self.num_stages - 1:
                down = self.features[2 * i + 2]
                t = layer_norm(f"features.{2 * i + 2}.0", down[0], y, h, w, c, False)
                if train is not None and index >= train["first"]:
                    acts.update({f"features.{2 * i + 2}.in": y, f"features.{2 * i + 2}.0": t})
                y, h, w = gemm(f"features.{2 * i + 2}.1", 0, down[1], t, h, w, c, 2)
                c = down[1].weight.shape[0]
                index += 1
        return pb.ops, outputs, keep, pb.names

    def forward_hip(self, x: Tensor, splits: int = 0, state: Optional[dict] = None) -> Dict[str, Tensor]:
        """``state`` (a dict): a training forward; it receives ``"first"``, ``"acts"`` and ``"factors"``, see
        ``build_plan``."""
        x = self._check_image(x)
        if min(x.shape[2], x.shape[3]) < 4 * 2 ** (self.num_stages - 1):
            raise RuntimeError(f"ConvNeXtBackbone: a {tuple(x.shape[2:])} canvas leaves a stage without pixels")
        if state is not None:
            state["first"] = self._first_trainable()
        ops, outputs, keep, _ = self.build_plan(x, splits, state)
        self._run_plan(_hip.ConvnextOpStruct, "sdetr_convnext", ops, x.device)
        return outputs

    # ------------------------------------------------------------------------------------------ training in HIP
    # (the interface is HipBackbone's: the node keeps the activations the backward reads; its backward is one
    # ``sdetr_convnext_bwd_run`` call over ``_backward_ops`` and returns the fp32 parameter gradients)
    train_reasons = ("the architecture is not one the HIP kernels serve (a block other than CNBlock with nn.LayerNorm, a "
                     "norm other than LayerNorm2d, or a width that is no multiple of 32 up to 3072)",
                     "the stem (features.0) is not frozen: the 4x4 patchify backward is out of scope")
    backward_struct, backward_prefix = _hip.ConvnextBwdOpStruct, "sdetr_convnext_bwd"

    def _stem_modules(self):
        return (self.features[0],)

    def _output_name(self, i: int) -> str:
        return f"features.{2 * i + 1}"

    def _sequence(self) -> List[Tuple[str, str, nn.Module]]:
        """``(kind, name, module)`` of every block (``"block"``) and down-sampler (``"down"``) in forward order."""
        seq = []
        for i, stage in enumerate(self.stages()):
            seq.extend(("block", f"features.{2 * i + 1}.{j}", blk) for j, blk in enumerate(stage))
            if i < self.num_stages - 1:
                seq.append(("down", f"features.{2 * i + 2}", self.features[2 * i + 2]))
        return seq

    # ``saved_activations()`` (HipBackbone's test hook) holds, by op name: ``<block>.in`` (the block's fp32 input rows),
    # ``<block>.block.0`` (fp32, before the LayerNorm), ``.block.2`` (normalised rows), ``.block.3`` (before the GELU),
    # ``.block.4`` (after it), and ``<down>.in`` / ``<down>.0`` of a down-sampler; ``stochastic_depth_factors()`` is
    # ``{block name: factors [B]}``.

    def _backward_ops(self, acts: Dict[str, Tensor], factors: Dict[str, Tensor], shape, cotangents: Dict[str, Optional[Tensor]],
                      splits: int = 0):
        """The backward of one forward as ``(ops, names, grads, keep)``: ``ops`` the ``sdetr_convnext_bwd_op`` list in run
        order, ``names`` one label per op, ``grads`` ``{parameter name: fp32 gradient}`` (as views of what the ops write),
        ``keep`` every tensor the ops point into.  Walks ``_sequence()`` from the top down to the lowest trainable module."""
        batch, _, height, width = shape
        seq, first = self._sequence(), self._first_trainable()
        act = torch.float32 if self._precision() == 0 else self.compute_dtype
        pb = BackwardPlanBuilder(self.backward_struct, next(iter(acts.values())), batch=batch, splits=splits)
        new, keep, tmp, want, grads = pb.new, pb.keep, pb.tmp, pb.want, pb.grads

        # the spatial size of every module's input
        sizes, h, w = [], height // 4, width // 4
        for kind, _, _ in seq:
            sizes.append((h, w))
            if kind == "down":
                h, w = h // 2, w // 2
        stage_of = {f"features.{2 * i + 1}.{len(st) - 1}": i for i, st in enumerate(self.stages())}

        dy = None
        for idx in range(len(seq) - 1, first - 1, -1):
            kind, name, m = seq[idx]
            h, w = sizes[idx]
            below = idx > first
            if kind == "block":
                c = m.block[0].weight.shape[0]
                stage = stage_of.get(name)
                if stage is not None and stage in self.return_indices:
                    dy = pb.ingest(name, 10, cotangents.get(f"features.{2 * stage + 1}"), dy, c, h, w)   # kind 10: NCHW ingest
                dw, norm, fc1, fc2 = m.block[0], m.block[2], m.block[3], m.block[5]
                dzs, db2p = tmp("dzs", (batch, h, w, c), act), tmp("db2p", (c,), torch.float32)
                pb.rows(name, dy, factors.get(name), dzs, db2p, c, h, w)
                if want(fc2.weight, fc2.bias, m.layer_scale):
                    # fc2's products carry the layer scale: kind 7 turns the plain sums into the three gradients
                    dw2p = tmp("dw2p", (c, 4 * c), torch.float32)
                    pb.op(name + ".block.5 (wgrad)", 1, dz=dzs.data_ptr(), x=acts[name + ".block.4"].data_ptr(),
                          scale=pb.ones(c).data_ptr(), out=dw2p.data_ptr(), channels=4 * c, height=h, width=w, out_channels=c)
                    dw2 = pb.grad(name + ".block.5.weight", (c, 4 * c), fc2.weight)
                    db2 = pb.grad(name + ".block.5.bias", (c,), fc2.bias)
                    dg = new((c,), torch.float32) if want(m.layer_scale) else None
                    w2, b2 = self._f32(fc2, "weight", fc2.weight), self._f32(fc2, "bias", fc2.bias)
                    g32 = self._f32(m, "layer_scale", m.layer_scale)
                    keep.extend((w2, b2, g32))
                    pb.op(name + " (layer scale)", 7, dz=db2p.data_ptr(), x=dw2p.data_ptr(), weight=w2.data_ptr(),
                          scale=b2.data_ptr(), gamma=g32.data_ptr(), out=_hip.ptr(dw2), dbias=_hip.ptr(db2), dgamma=_hip.ptr(dg),
                          batch=1, channels=c, height=1, width=1, out_channels=4 * c)
                    if dg is not None:
                        grads[name + ".layer_scale"] = dg.view(c, 1, 1)
                if not (below or want(dw.weight, dw.bias, norm.weight, norm.bias, fc1.weight, fc1.bias)):
                    continue
                dh = tmp("dh", (batch, h, w, 4 * c), act)
                pb.dgrad(name + ".block.5", self._packed_rows_dgrad(fc2, m.layer_scale), dzs, dh, 4 * c, c, h, w)
                pb.gelu(name + ".block.4", dh, acts[name + ".block.3"], pb.grad(name + ".block.3.bias", (4 * c,), fc1.bias),
                        4 * c, h, w)
                if want(fc1.weight):
                    pb.wgrad(name + ".block.3", dh, acts[name + ".block.2"], c, 4 * c, h, w)
                if not (below or want(dw.weight, dw.bias, norm.weight, norm.bias)):
                    continue
                dn = tmp("dn", (batch, h, w, c), act)
                pb.dgrad(name + ".block.3", self._packed_rows_dgrad(fc1), dh, dn, c, 4 * c, h, w)
                d = tmp("d", (batch, h, w, c), torch.float32)
                pb.layer_norm_bwd(name + ".block.2", norm, self._f32(norm, "weight", norm.weight), dz=dn,
                                  x=acts[name + ".block.0"], out=d, channels=c, height=h, width=w)
                if want(dw.weight, dw.bias):   # kind 5: the depthwise taps' and bias gradient
                    dtaps = new((49, c), torch.float32)
                    dbd = pb.grad(name + ".block.0.bias", (c,), dw.bias)
                    pb.op(name + ".block.0 (wgrad)", 5, dz=d.data_ptr(), x=acts[name + ".in"].data_ptr(), out=dtaps.data_ptr(),
                          dbias=_hip.ptr(dbd), channels=c, height=h, width=w)
                    if want(dw.weight):
                        grads[name + ".block.0.weight"] = dtaps.t().reshape(c, 1, 7, 7)
                if below:   # kind 6: the depthwise backward-data, the residual's gradient added
                    taps, _ = self._taps(dw)
                    keep.append(taps)
                    dx = pb.next_dy((batch, h, w, c))
                    pb.op(name + ".block.0 (dgrad)", 6, dz=d.data_ptr(), weight=taps.data_ptr(), add=dy.data_ptr(),
                          out=dx.data_ptr(), channels=c, height=h, width=w)
                    dy = dx
            else:
                norm, conv = m[0], m[1]
                c, co = conv.weight.shape[1], conv.weight.shape[0]
                ho, wo = h // 2, w // 2
                dzc = tmp("dzc", (batch, ho, wo, co), act)
                pb.rows(name + ".1", dy, None, dzc, pb.grad(name + ".1.bias", (co,), conv.bias), co, ho, wo)
                if want(conv.weight):   # kind 8: the normalised rows as 2x2 patches, the weight as [out, (ky, kx, in)] rows
                    patches = tmp("patches", (batch, ho, wo, 4 * c), act)
                    pb.op(name + ".1 (patches)", 8, x=acts[name + ".0"].data_ptr(), out=patches.data_ptr(), channels=c, height=h,
                          width=w)
                    dwp = pb.wgrad(name + ".1", dzc, patches, 4 * c, co, ho, wo)
                    grads[name + ".1.weight"] = dwp.view(co, 2, 2, c).permute(0, 3, 1, 2)
                dy_next = None
                if below or want(norm.weight, norm.bias):
                    dpatch = tmp("dpatch", (batch, ho, wo, 4 * c), act)
                    pb.dgrad(name + ".1", self._packed_rows_dgrad(conv), dzc, dpatch, 4 * c, co, ho, wo)
                    dn = tmp("dn", (batch, h, w, c), act)   # kind 9: the patches' gradient back on the pixels
                    pb.op(name + ".1 (pixels)", 9, dz=dpatch.data_ptr(), out=dn.data_ptr(), channels=c, height=h, width=w)
                    dy_next = pb.next_dy((batch, h, w, c))
                    pb.layer_norm_bwd(name + ".0", norm, self._f32(norm, "weight", norm.weight), dz=dn, x=acts[name + ".in"],
                                      out=dy_next, channels=c, height=h, width=w)
                dy = dy_next
        return pb.ops, pb.names, grads, keep
