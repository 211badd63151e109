"""Row N3 of SURVEY.md section 8(f): the RepVGGPluX neck that every reference config puts between the encoder and the
proposal stage (``models/necks/repnet.py:12-245``, called at ``models/bricks/salience_transformer.py:185-192``).

Same class names, constructor arguments and state-dict keys as the reference, so its checkpoints load unchanged:
``lateral_convs.{i}.{0,1}.*``, ``layer_blocks.{i}.{conv1,conv2}.{0,1}.*``,
``layer_blocks.{i}.bottlenecks.{j}.{conv1,conv2}.{0,1}.*``, ``...bottlenecks.{j}.se_module.{conv_mask,se_module.0,
se_module.2}.*``, ``downsample_blocks.{i}.{0,1}.*``, ``pan_blocks.{i}....``.  The ``nn.Conv2d`` / ``nn.BatchNorm2d``
objects below only HOLD those parameters; nothing here calls a library convolution.

How it runs (eval mode):
  * feature maps stay token-major ``[B, H*W, C]`` -- the encoder's memory IS channels-last, the reference's two
    transposes per level disappear (``forward_memory``);
  * every BatchNorm folds into the convolution before it; ``conv1(x) + alpha * conv2(x)`` of a RepVGG block
    (3x3 + 1x1, each with its norm, repnet.py:61-62) folds into ONE grouped 3x3 kernel with a bias;
  * a 1x1 convolution is a GEMM on the token rows (library GEMM) + ``sdetr_neck_combine`` (bias, SiLU); it commutes
    with nearest up-sampling, so the coarse half of ``cat([upsample(high), low])`` is multiplied at the COARSE
    resolution (4x fewer rows) and up-sampled inside the combine kernel; ``conv1`` and ``conv2`` of a CSP layer read
    the same input and run as one GEMM of twice the width;
  * 3x3 convolutions (fp32 LDS-tiled kernel; bf16 maps with the real channel counts: the MFMA kernel), the
    attention-pooled gate and the shortcuts are the HIP kernels of ``include/salience_hip.h`` (13).
Training mode (``.train()``): the differentiable form -- NCHW convolutions on the parameter holders, every BatchNorm on
BATCH statistics taken over all ranks' pixels (``data_parallel.sync_batch_norm_train``: one all-reduce per norm and
direction where the reference's ``nn.SyncBatchNorm`` issues an all_gather + all_reduce pair, ``main.py:126-127``),
running statistics updated as ``nn.BatchNorm2d`` does.  It is the autograd path of this row (device tensors only, like
every other operator here); the HIP kernels above are the inference path.
Training in HIP (``set_train_form("hip")``, opt-in, ``csrc/neck_backward.hip``; the interface, its autograd node and the
plan runner are ``hip_module.HipModule``'s): the token-major fp32 levels go into one autograd node whose forward keeps the
pre-norm maps, the batch statistics and what the gate's backward reads, and whose backward is one op list
(``forward_hip_train``, ``build_backward_plan``).  fp32 only, this process's statistics only; anything else raises at
forward with its reason (``hip_train_reason``), it never falls back.
"""
from collections import OrderedDict
from typing import Dict, List, Sequence, Tuple

import torch
from torch import Tensor, nn

from . import _hip
from . import filter_ops as FO
from .derived import derived
from .hip_module import BackwardPlanBuilder, HipModule, _TrainFunction


class Conv2dNormActivation(nn.Sequential):
    """Parameter holder with the reference's layout (``models/bricks/misc.py:61-158``): ``0`` = convolution
    (bias-free when a norm follows), ``1`` = norm, then the activation."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size: int = 3, stride: int = 1, padding=None,
                 groups: int = 1, norm_layer=nn.BatchNorm2d, activation_layer=nn.ReLU, inplace: bool = True):
        if padding is None:
            padding = (kernel_size - 1) // 2
        layers: List[nn.Module] = [nn.Conv2d(in_channels, out_channels, kernel_size, stride, padding, groups=groups,
                                             bias=norm_layer is None)]
        if norm_layer is not None:
            layers.append(norm_layer(out_channels))
        if activation_layer is not None:
            layers.append(activation_layer(inplace=inplace))
        super().__init__(*layers)

    def folded(self) -> Tuple[Tensor, Tensor]:
        """(weight [out, in / groups, k, k], bias [out]) of conv + norm on the running statistics, fp32."""
        conv = self[0]
        w = conv.weight.detach().float()
        b = conv.bias.detach().float() if conv.bias is not None else torch.zeros(w.shape[0], device=w.device)
        if len(self) > 1 and isinstance(self[1], nn.modules.batchnorm._BatchNorm):
            bn = self[1]
            scale = bn.weight.detach().float() * torch.rsqrt(bn.running_var.detach().float() + bn.eps)
            w = w * scale.view(-1, 1, 1, 1)
            b = (b - bn.running_mean.detach().float()) * scale + bn.bias.detach().float()
        return w, b


class SqueezeAndExcitation(nn.Module):
    """Parameter holder of ``models/bricks/basic.py:29-41``: ``conv_mask`` (C -> 1 attention-pooling logits) and the
    bias-free C -> C/16 -> C gate."""

    def __init__(self, channels: int, reduction: int = 16):
        super().__init__()
        self.conv_mask = nn.Conv2d(channels, 1, kernel_size=1)
        self.se_module = nn.Sequential(
            nn.Conv2d(channels, channels // reduction, kernel_size=1, bias=False), nn.ReLU(inplace=True),
            nn.Conv2d(channels // reduction, channels, kernel_size=1, bias=False), nn.Sigmoid())


class RepVggPluXBlock(nn.Module):
    """``models/necks/repnet.py:12-64``: grouped 3x3 + grouped 1x1 (own BatchNorms), activation, gate, shortcut."""

    def __init__(self, in_channels: int, out_channels: int, activation_layer=nn.ReLU, inplace: bool = True,
                 groups: int = 4, alpha: bool = False):
        super().__init__()
        if in_channels != out_channels:
            raise ValueError("RepVggPluXBlock: built for in_channels == out_channels (every reference config)")
        self.in_channels, self.out_channels, self.groups = in_channels, out_channels, groups
        self.activation = activation_layer(inplace=True)
        self.conv1 = Conv2dNormActivation(in_channels, out_channels, 3, 1, 1, groups=groups, activation_layer=None)
        self.conv2 = Conv2dNormActivation(in_channels, out_channels, 1, 1, 0, groups=groups, activation_layer=None)
        self.alpha = nn.Parameter(torch.tensor(1.0)) if alpha else 1.0
        self.se_module = SqueezeAndExcitation(out_channels)
        self.identity = nn.Identity()

    def folded(self, dtype=torch.float32) -> Dict[str, Tensor]:
        w3, b3 = self.conv1.folded()
        w1, b1 = self.conv2.folded()
        alpha = float(self.alpha)
        w = w3.clone()
        w[:, :, 1, 1] += alpha * w1[:, :, 0, 0]
        G, C = self.groups, self.out_channels
        # [out, in/G, 3, 3] -> [G, 3, 3, in/G, out/G]
        packed = w.view(G, C // G, C // G, 3, 3).permute(0, 3, 4, 2, 1).contiguous()
        se = self.se_module
        R = se.se_module[0].weight.shape[0]
        return dict(weight=packed, bias=(b3 + alpha * b1).contiguous(),
                    mfma=FO.neck_pack_conv3x3(packed, dtype) if dtype in (torch.bfloat16, torch.float16) and packed.is_cuda else None,
                    mask=se.conv_mask.weight.detach().float().reshape(C).contiguous(),
                    squeeze=se.se_module[0].weight.detach().float().reshape(R, C).contiguous(),
                    excite=se.se_module[2].weight.detach().float().reshape(C, R).contiguous())


class CSPRepPluXLayer(nn.Module):
    """``models/necks/repnet.py:67-123``."""

    def __init__(self, in_channels: int, out_channels: int, num_blocks: int = 3, expansion: float = 1.0,
                 groups: int = 4, norm_layer=nn.BatchNorm2d, activation_layer=nn.SiLU):
        super().__init__()
        hidden = int(out_channels * expansion)
        if hidden != out_channels:
            raise ValueError("CSPRepPluXLayer: built for expansion = 1 (every reference config)")
        self.conv1 = Conv2dNormActivation(in_channels, hidden, 1, 1, norm_layer=norm_layer,
                                          activation_layer=activation_layer)
        self.conv2 = Conv2dNormActivation(in_channels, hidden, 1, 1, norm_layer=norm_layer,
                                          activation_layer=activation_layer)
        self.bottlenecks = nn.Sequential(*[RepVggPluXBlock(hidden, hidden, groups=groups,
                                                           activation_layer=activation_layer)
                                           for _ in range(num_blocks)])
        self.conv3 = nn.Identity()

    def folded(self, dtype) -> Dict[str, object]:
        w1, b1 = self.conv1.folded()
        w2, b2 = self.conv2.folded()
        w = torch.cat([w1[:, :, 0, 0], w2[:, :, 0, 0]], 0)  # [2 * hidden, in]: conv1's outputs, then conv2's
        half = w.shape[1] // 2
        return dict(first=w[:, :half].to(dtype).contiguous(), second=w[:, half:].to(dtype).contiguous(),
                    bias=torch.cat([b1, b2]).contiguous(), blocks=[blk.folded(dtype) for blk in self.bottlenecks])


def _token_matmul(x: Tensor, weight: Tensor) -> Tensor:
    """``x @ weight.T`` for token-major ``[B, N, C]`` maps; a row range of a longer buffer (batch stride > N * C) goes
    through the strided-batched GEMM instead of being copied first."""
    if x.is_contiguous() or x.dim() != 3 or x.stride(2) != 1 or x.stride(1) != x.shape[2]:
        return torch.matmul(x, weight.t())
    return torch.bmm(x, weight.t().expand(x.shape[0], -1, -1))


def _is_silu(act) -> bool:
    return act is nn.SiLU or isinstance(act, nn.SiLU)


class RepVGGPluXNetwork(HipModule):
    """``models/necks/repnet.py:125-245``.  ``forward`` keeps the reference's interface (ordered dict of NCHW maps in,
    same keys out); ``forward_memory`` is the token-major entry the transformer uses.  ``set_train_form("hip")`` (the
    interface is ``HipModule``'s) trains on the kernels of ``csrc/neck_backward.hip``, see ``forward_hip_train``."""

    compute_dtype = torch.float32   # the "hip" training form is fp32 only; the inference form follows the rows' dtype

    def __init__(self, in_channels_list: List[int], out_channels_list: List[int], groups: int = 4,
                 norm_layer=nn.BatchNorm2d, activation=nn.SiLU, extra_block: bool = False):
        super().__init__()
        if any(c == 0 for c in in_channels_list):
            raise ValueError("in_channels=0 is currently not supported")
        if len(set(in_channels_list) | set(out_channels_list)) != 1:
            raise ValueError("RepVGGPluXNetwork: built for one channel count on all levels (every reference config)")
        if not _is_silu(activation):
            raise ValueError("RepVGGPluXNetwork: the kernels implement SiLU (every reference config)")
        C = out_channels_list[0]
        if C % (4 * groups) or C > 256 or C < 16:
            raise ValueError("RepVGGPluXNetwork: channels must be a multiple of 4 * groups, 16 <= channels <= 256")
        self.channels, self.groups = C, groups
        n = len(out_channels_list)
        self.lateral_convs = nn.ModuleList(Conv2dNormActivation(C, C, 1, 1, norm_layer=norm_layer,
                                                                activation_layer=activation) for _ in range(1, n))
        self.layer_blocks = nn.ModuleList(CSPRepPluXLayer(2 * C, C, groups=groups, norm_layer=norm_layer,
                                                          activation_layer=activation) for _ in range(1, n))
        self.downsample_blocks = nn.ModuleList(Conv2dNormActivation(C, C, 3, 2, 1, norm_layer=norm_layer,
                                                                    activation_layer=activation) for _ in range(n - 1))
        self.pan_blocks = nn.ModuleList(CSPRepPluXLayer(2 * C, C, groups=groups, norm_layer=norm_layer,
                                                        activation_layer=activation) for _ in range(n - 1))
        self.extra_block = extra_block
        self.process_group = None   # ranks whose pixels share the batch statistics in training mode (None = all)
        self.init_weights()

    def init_weights(self):
        """repnet.py:202-208: every convolution kaiming-uniform (a = 1), biases zero."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_uniform_(m.weight, a=1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    # ---- folded parameters ------------------------------------------------------------------------------------------
    def _folded(self, dtype) -> Dict[str, object]:
        return derived(self, "folded", list(self.parameters()) + list(self.buffers()), lambda: self._fold(dtype),
                       extra=dtype)

    def _fold(self, dtype) -> Dict[str, object]:
        plan: Dict[str, object] = dict(lateral=[], layer=[], down=[], pan=[])
        for m in self.lateral_convs:
            w, b = m.folded()
            plan["lateral"].append((w[:, :, 0, 0].to(dtype).contiguous(), b.contiguous()))
        for m in self.layer_blocks:
            plan["layer"].append(m.folded(dtype))
        for m in self.downsample_blocks:
            w, b = m.folded()  # dense [out, in, 3, 3] -> [1, 3, 3, in, out]
            wd = w.permute(2, 3, 1, 0).contiguous().unsqueeze(0)
            plan["down"].append((wd, b.contiguous(),
                                 FO.neck_pack_conv3x3(wd, dtype) if dtype in (torch.bfloat16, torch.float16) and wd.is_cuda else None))
        for m in self.pan_blocks:
            plan["pan"].append(m.folded(dtype))
        return plan

    # ---- token-major forward ----------------------------------------------------------------------------------------
    @staticmethod
    def _csp(p, first: Tensor, first_hw, second: Tensor, hw, upsample: bool) -> Tensor:
        """CSPRepPluXLayer on ``cat([first (up-sampled to hw when asked), second], channels)`` (repnet.py:120-123)."""
        h, w = hw
        C = second.shape[2]
        a_second = _token_matmul(second, p["second"])  # [B, N, 2C]: conv1 | conv2 outputs
        if upsample:
            a_first = torch.matmul(first, p["first"].t())  # at the coarse resolution
            both = FO.neck_combine(a_second, h, w, up=a_first, up_hw=first_hw, bias=p["bias"], activation=True)
        else:
            # (in place: the out-of-place form copies its first operand into the result before the GEMM)
            a_second = a_second.baddbmm_(first, p["first"].t().expand(first.shape[0], -1, -1))
            both = FO.neck_combine(a_second, h, w, bias=p["bias"], activation=True)
        x, branch = both[:, :, :C], both[:, :, C:]
        last = len(p["blocks"]) - 1
        for j, blk in enumerate(p["blocks"]):
            y = FO.neck_conv3x3(x, h, w, blk["weight"], blk["bias"], stride=1, activation=True, packed=blk["mfma"])
            x = FO.neck_gate_shortcut(y, blk["mask"], blk["squeeze"], blk["excite"], shortcut=x,
                                      shortcut2=branch if j == last else None)
        if last < 0:
            x = x + branch
        return x

    def forward_levels(self, levels: Sequence[Tensor], shapes: Sequence[Tuple[int, int]],
                       differentiable: bool = False) -> List[Tensor]:
        """Token-major levels ``[B, h*w, C]`` (fine to coarse) -> the same (repnet.py:211-245).  ``differentiable``: take
        the torch-op form also in eval mode (running statistics in the norms) -- the fused kernels have no backward."""
        if len(levels) != len(self.layer_blocks) + 1:
            raise RuntimeError("RepVGGPluXNetwork: wrong number of levels")
        if self.training or differentiable:
            if self.train_form == "hip" and self._needs_autograd(*levels):
                return self.forward_hip_train(levels, shapes)
            if not levels[0].is_cuda:
                raise RuntimeError("RepVGGPluXNetwork: HIP device tensors required; there is no CPU fallback")
            maps = [x.transpose(1, 2).reshape(x.shape[0], x.shape[2], int(h), int(w)) for x, (h, w) in zip(levels, shapes)]
            return [o.flatten(2).transpose(1, 2) for o in self.forward_train(maps)]
        plan = self._folded(levels[0].dtype)  # (the kernels' wrappers refuse CPU tensors: no fallback)
        shapes = [(int(h), int(w)) for h, w in shapes]
        L = len(levels)
        inner = [levels[-1]]
        for idx in range(L - 1, 0, -1):  # top-down
            hh, hw_ = shapes[idx]
            wl, bl = plan["lateral"][idx - 1]
            high = FO.neck_combine(_token_matmul(inner[0], wl), hh, hw_, bias=bl, activation=True)
            inner[0] = high
            inner.insert(0, self._csp(plan["layer"][idx - 1], high, shapes[idx], levels[idx - 1], shapes[idx - 1], True))
        outs = [inner[0]]
        for idx in range(L - 1):  # bottom-up
            h, w = shapes[idx]
            wd, bd, pd = plan["down"][idx]
            down = FO.neck_conv3x3(outs[-1], h, w, wd, bd, stride=2, activation=True, packed=pd)
            if down.shape[1] != shapes[idx + 1][0] * shapes[idx + 1][1]:
                raise RuntimeError("RepVGGPluXNetwork: level sizes are not a stride-2 pyramid")
            outs.append(self._csp(plan["pan"][idx], down, shapes[idx + 1], inner[idx + 1], shapes[idx + 1], False))
        return outs

    # ---- training form (repnet.py:211-245 with batch-statistics norms) ---------------------------------------------
    def _conv_norm(self, m: Conv2dNormActivation, x: Tensor, act: bool = True) -> Tensor:
        from .data_parallel import sync_batch_norm_train
        conv = m[0]
        y = torch.nn.functional.conv2d(x, conv.weight, conv.bias, conv.stride, conv.padding, 1, conv.groups)
        if self.training:
            y = sync_batch_norm_train(y, m[1], self.process_group)
        else:   # eval mode under autograd: running statistics, as nn.BatchNorm2d.eval()
            bn = m[1]
            y = torch.nn.functional.batch_norm(y, bn.running_mean, bn.running_var, bn.weight, bn.bias, False, 0.0, bn.eps)
        return torch.nn.functional.silu(y) if act else y

    @staticmethod
    def _gate(se: "SqueezeAndExcitation", x: Tensor) -> Tensor:
        """Attention-pooled gate (models/bricks/basic.py:29-54): softmax over the pixels of conv_mask(x) weights the
        pixels, the pooled vector goes through C -> C/16 -> ReLU -> C -> sigmoid and scales x."""
        B, C, H, W = x.shape
        logit = torch.nn.functional.conv2d(x, se.conv_mask.weight, se.conv_mask.bias).view(B, H * W)
        context = torch.einsum("bcp,bp->bc", x.reshape(B, C, H * W), logit.softmax(-1))
        hidden = torch.relu(context @ se.se_module[0].weight.view(-1, C).t())
        gate = torch.sigmoid(hidden @ se.se_module[2].weight.view(C, -1).t())
        return gate.view(B, C, 1, 1) * x

    def _csp_train(self, layer: CSPRepPluXLayer, x: Tensor) -> Tensor:
        y = self._conv_norm(layer.conv1, x)
        for blk in layer.bottlenecks:
            z = self._conv_norm(blk.conv1, y, act=False) + blk.alpha * self._conv_norm(blk.conv2, y, act=False)
            y = self._gate(blk.se_module, torch.nn.functional.silu(z)) + y
        return y + self._conv_norm(layer.conv2, x)

    def forward_train(self, feats: Sequence[Tensor]) -> List[Tensor]:
        """NCHW levels (fine to coarse) -> the same, training mode: differentiable, batch statistics over the
        process group ``self.process_group`` (None = all ranks / this process), running statistics updated."""
        L = len(feats)
        inner = [feats[-1]]
        for idx in range(L - 1, 0, -1):  # top-down
            high = self._conv_norm(self.lateral_convs[idx - 1], inner[0])
            inner[0] = high
            up = torch.nn.functional.interpolate(high, size=feats[idx - 1].shape[-2:], mode="nearest")
            inner.insert(0, self._csp_train(self.layer_blocks[idx - 1], torch.cat([up, feats[idx - 1]], 1)))
        outs = [inner[0]]
        for idx in range(L - 1):  # bottom-up
            down = self._conv_norm(self.downsample_blocks[idx], outs[-1])
            outs.append(self._csp_train(self.pan_blocks[idx], torch.cat([down, inner[idx + 1]], 1)))
        return outs

    # ---- training in HIP (the interface is HipModule's; kernels: csrc/neck_backward.hip) ---------------------------
    def _norms(self) -> List[nn.Module]:
        return [m[1] for m in self.modules() if isinstance(m, Conv2dNormActivation)]

    def hip_train_reason(self, inputs=None):
        """Why the ``"hip"`` training form cannot serve this module (and the token-major levels ``inputs``); ``None``
        when it can."""
        if not self.training:
            return ("eval() mode: the 'hip' form normalises on batch statistics (differentiable=True in eval() mode "
                    "differentiates through the running statistics: the 'torch' form)")
        if torch.is_autocast_enabled() or torch.is_autocast_enabled("cpu"):
            return "autocast is on: the 'hip' form takes fp32 rows only"
        if torch.distributed.is_available() and torch.distributed.is_initialized() \
                and torch.distributed.get_world_size(self.process_group) > 1:
            return "several ranks share the batch statistics: the 'hip' form takes this process's statistics alone"
        for bn in self._norms():
            if not isinstance(bn, nn.modules.batchnorm._BatchNorm) or not bn.affine or not bn.track_running_stats:
                return "a norm is not an affine BatchNorm with running statistics"
            if bn.momentum is None:
                return "a BatchNorm has momentum=None (the cumulative moving average)"
        for m in self.modules():
            if isinstance(m, RepVggPluXBlock) and isinstance(m.alpha, nn.Parameter):
                return "alpha of a RepVggPluXBlock is a Parameter (a float in every reference config)"
            if isinstance(m, CSPRepPluXLayer) and len(m.bottlenecks) == 0:
                return "a CSPRepPluXLayer without bottlenecks"
        if any(p.dtype != torch.float32 for p in self.parameters()):
            return "a parameter is not float32"
        if inputs is not None:
            if any(x.dtype in (torch.bfloat16, torch.float16) for x in inputs):
                return "16-bit rows: the 'hip' form takes fp32 rows only"
            if any(x.dtype != torch.float32 for x in inputs):
                return "the rows are not float32"
            if any(not x.is_cuda for x in inputs) or any(not p.is_cuda for p in self.parameters()):
                return "an input or a parameter is a CPU tensor: the hot path has no CPU fallback"
        return None

    def forward_hip_train(self, levels: Sequence[Tensor], shapes: Sequence[Tuple[int, int]]) -> List[Tensor]:
        """The ``"hip"`` training form of ``forward_levels``: ONE autograd node over the token-major fp32 levels
        ``[B, h*w, C]`` and the trainable parameters.  Forward, per conv + norm: the convolution without bias
        (``sdetr_neck_conv3x3``; dense 1x1: a library GEMM on the rows, the up-sampled half at the coarse resolution; the
        grouped 1x1: the 3x3 kernel's centre tap), ``sdetr_neck_bn_stats`` (fixed-order batch statistics over the
        fine-resolution rows, the running statistics updated as ``nn.BatchNorm2d`` does) and ``sdetr_neck_bn_apply``
        (normalise + affine + SiLU; a RepVGG block's two norms in one launch); the gate is ``sdetr_neck_gate_train``.
        Backward: ``build_backward_plan``.  Stored (``saved_activations``): per conv + norm ``<name>.z`` (the pre-norm
        map) and ``<name>.stats`` (mean, rstd); per block ``<block>.s`` (the gate's input), ``<block>.logits``,
        ``<block>.saved`` (gate | context | hidden | softmax max, sum); ``input.<l>`` and the maps the convolutions read."""
        levels = list(levels)
        self._check_train_form(levels)
        if len({x.shape[0] for x in levels}) != 1 or any(x.dim() != 3 or x.shape[2] != self.channels for x in levels):
            raise RuntimeError("RepVGGPluXNetwork: levels must be [B, h*w, channels] of one batch size")
        self.__dict__["_hip_shapes"] = [(int(h), int(w)) for h, w in shapes]
        named = [(n, p) for n, p in self.named_parameters() if p.requires_grad]
        return list(_TrainFunction.apply(self, len(levels), 0, tuple(n for n, _ in named), *levels, *[p for _, p in named]))

    @staticmethod
    def _train_weights(conv: nn.Conv2d) -> Tuple[Tensor, Tensor]:
        """``(forward [G, 3, 3, Ci/G, Co/G] -- a 1x1 as the centre tap --, backward-data [G, k, k, Co/G, Ci/G] with the
        taps flipped)`` of a convolution's weight, once per parameter version."""
        def build():
            w = conv.weight.detach()
            G, k = conv.groups, w.shape[2]
            v = w.view(G, w.shape[0] // G, w.shape[1], k, k)
            fwd = v.permute(0, 3, 4, 2, 1).contiguous()
            if k == 1:
                full = torch.zeros((G, 3, 3) + tuple(fwd.shape[3:]), device=w.device, dtype=w.dtype)
                full[:, 1, 1] = fwd[:, 0, 0]
                fwd = full
            return fwd, v.flip(3, 4).permute(0, 3, 4, 1, 2).contiguous()
        return derived(conv, "neck_train_weights", (conv.weight,), build)

    def _bn_stats(self, bn, z: Tensor, cols: slice, acts: dict, name: str) -> Tensor:
        view = z[:, :, cols]
        rows, C, lib = z.shape[0] * z.shape[1], bn.num_features, self._lib()
        stats = torch.empty((2, C), device=z.device, dtype=torch.float32)
        ws_bytes = lib.sdetr_neck_bn_stats_workspace_bytes(rows, C)
        ws = torch.empty(max(int(ws_bytes), 16), dtype=torch.uint8, device=z.device)
        _hip.launch("sdetr_neck_bn_stats", lib, z.device, view.data_ptr(), z.shape[2], rows, C, float(bn.eps), float(bn.momentum),
                    bn.running_mean.data_ptr(), bn.running_var.data_ptr(), stats.data_ptr(), ws.data_ptr(), ws_bytes)
        bn.num_batches_tracked.add_(1)
        acts[name + ".z"], acts[name + ".stats"] = view, stats
        return stats

    def _bn_apply(self, bn, z: Tensor, cols: slice, stats: Tensor, out: Tensor, second=None, alpha: float = 0.0):
        view, oview = z[:, :, cols], out[:, :, cols]
        bn2, z2, stats2 = second if second is not None else (None, None, None)
        _hip.launch("sdetr_neck_bn_apply", self._lib(), z.device, view.data_ptr(), stats.data_ptr(), bn.weight.data_ptr(),
                    bn.bias.data_ptr(), _hip.ptr(z2), _hip.ptr(stats2), None if bn2 is None else bn2.weight.data_ptr(),
                    None if bn2 is None else bn2.bias.data_ptr(), float(alpha), z.shape[2], z.shape[0] * z.shape[1],
                    bn.num_features, 1, oview.data_ptr(), out.shape[2])

    def _conv_norm_hip(self, m: Conv2dNormActivation, name: str, x: Tensor, hw, acts: dict) -> Tensor:
        """Lateral (dense 1x1) or down-sampler (dense 3x3 stride 2) + norm + SiLU."""
        conv, bn = m[0], m[1]
        acts[name + ".in"] = x
        if conv.kernel_size[0] == 1:
            z = torch.matmul(x, conv.weight.detach()[:, :, 0, 0].t())
        else:
            z = FO.neck_conv3x3(x, hw[0], hw[1], self._train_weights(conv)[0], None, stride=conv.stride[0], activation=False)
        stats = self._bn_stats(bn, z, slice(None), acts, name)
        out = torch.empty_like(z)
        self._bn_apply(bn, z, slice(None), stats, out)
        return out

    def _csp_hip(self, layer: CSPRepPluXLayer, name: str, first: Tensor, first_hw, second: Tensor, hw, upsample: bool,
                 acts: dict) -> Tensor:
        h, w = hw
        B, P, C = second.shape
        wc = torch.cat([layer.conv1[0].weight.detach()[:, :, 0, 0], layer.conv2[0].weight.detach()[:, :, 0, 0]], 0)  # [2C, 2C]
        acts[name + ".first"], acts[name + ".second"], acts[name + ".weight"] = first, second, wc
        zz = torch.matmul(second, wc[:, C:].t())
        if upsample:   # the statistics are those of the fine-resolution sum: materialised, it is what the backward reads
            zz = FO.neck_combine(zz, h, w, up=torch.matmul(first, wc[:, :C].t()), up_hw=first_hw, bias=None, activation=False)
        else:
            zz = zz.baddbmm_(first, wc[:, :C].t().expand(B, -1, -1))
        both = torch.empty_like(zz)
        for conv, cols, tag in ((layer.conv1, slice(0, C), ".conv1"), (layer.conv2, slice(C, 2 * C), ".conv2")):
            self._bn_apply(conv[1], zz, cols, self._bn_stats(conv[1], zz, cols, acts, name + tag), both)
        x, branch = both[:, :, :C], both[:, :, C:]
        lib, last = self._lib(), len(layer.bottlenecks) - 1
        for j, blk in enumerate(layer.bottlenecks):
            bname = f"{name}.bottlenecks.{j}"
            acts[bname + ".in"] = x
            z3 = FO.neck_conv3x3(x, h, w, self._train_weights(blk.conv1[0])[0], None, stride=1, activation=False)
            z1 = FO.neck_conv3x3(x, h, w, self._train_weights(blk.conv2[0])[0], None, stride=1, activation=False)
            st3 = self._bn_stats(blk.conv1[1], z3, slice(None), acts, bname + ".conv1")
            st1 = self._bn_stats(blk.conv2[1], z1, slice(None), acts, bname + ".conv2")
            s = torch.empty_like(z3)
            self._bn_apply(blk.conv1[1], z3, slice(None), st3, s, second=(blk.conv2[1], z1, st1), alpha=float(blk.alpha))
            se = blk.se_module
            R = se.se_module[0].weight.shape[0]
            logits = torch.empty((B, P), device=s.device, dtype=torch.float32)
            saved = torch.empty((B, 2 * C + 68), device=s.device, dtype=torch.float32)
            ws_bytes = lib.sdetr_neck_gate_train_workspace_bytes(B, P, C)
            ws = torch.empty(max(int(ws_bytes), 16), dtype=torch.uint8, device=s.device)
            out = torch.empty_like(s)
            _hip.launch("sdetr_neck_gate_train", lib, s.device, s.data_ptr(), B, P, C, se.conv_mask.weight.data_ptr(),
                        _hip.ptr(se.conv_mask.bias), se.se_module[0].weight.data_ptr(), se.se_module[2].weight.data_ptr(), R,
                        x.data_ptr(), x.stride(1), branch.data_ptr() if j == last else None, branch.stride(1), logits.data_ptr(),
                        saved.data_ptr(), ws.data_ptr(), ws_bytes, out.data_ptr())
            acts[bname + ".s"], acts[bname + ".logits"], acts[bname + ".saved"] = s, logits, saved
            x = out
        return x

    def _train_forward(self, inputs: Sequence[Tensor], splits: int, state: dict) -> Tuple[Tensor, ...]:
        """(The node's forward hook; the stored names are ``forward_hip_train``'s.)"""
        shapes = self.__dict__.pop("_hip_shapes")
        acts = state.setdefault("acts", {})
        state["shapes"] = shapes
        levels = [x.detach() if x.is_contiguous() else x.detach().contiguous() for x in inputs]
        L = len(levels)
        for l, x in enumerate(levels):
            acts[f"input.{l}"] = x
        inner = [levels[-1]]
        for idx in range(L - 1, 0, -1):  # top-down
            high = self._conv_norm_hip(self.lateral_convs[idx - 1], f"lateral_convs.{idx - 1}", inner[0], shapes[idx], acts)
            inner[0] = high
            inner.insert(0, self._csp_hip(self.layer_blocks[idx - 1], f"layer_blocks.{idx - 1}", high, shapes[idx],
                                          levels[idx - 1], shapes[idx - 1], True, acts))
        outs = [inner[0]]
        for idx in range(L - 1):  # bottom-up
            down = self._conv_norm_hip(self.downsample_blocks[idx], f"downsample_blocks.{idx}", outs[-1], shapes[idx], acts)
            if down.shape[1] != shapes[idx + 1][0] * shapes[idx + 1][1]:
                raise RuntimeError("RepVGGPluXNetwork: level sizes are not a stride-2 pyramid")
            outs.append(self._csp_hip(self.pan_blocks[idx], f"pan_blocks.{idx}", down, shapes[idx + 1], inner[idx + 1],
                                      shapes[idx + 1], False, acts))
        return tuple(outs)

    def build_backward_plan(self, acts: Dict[str, Tensor], shapes, cotangents: Sequence[Tensor]):
        """The backward of one training forward: ``(builder, hosts, finish, input gradients)``.  ``builder.ops`` are
        ``sdetr_neck_bwd_op`` ops (kinds: 0 dgrad, 1 wgrad, 2 sum, 3 norm, 4 gate, 5 upsample) in order; ``hosts`` are
        ``(op index, call)``: the library GEMMs of the dense 1x1 convolutions, which run before the op of that index;
        ``finish()`` assembles the CSP layers' 1x1 weight gradients.  The bottom-up path runs from the last level down,
        then the top-down path from the first level up; a level that feeds both paths gets the sum of its two gradients."""
        L, C, G = len(shapes), self.channels, self.groups
        B = acts["input.0"].shape[0]
        b = BackwardPlanBuilder(_hip.NeckBwdOpStruct, acts["input.0"], batch=B)
        hosts: List[tuple] = []
        b.keep.extend(t for t in acts.values())

        def host(fn):
            hosts.append((len(b.ops), fn))

        def rows(hw, c=C):
            return b.new((B, hw[0] * hw[1], c), torch.float32)

        def total(parts, hw):
            parts = [p for p in parts if p is not None]
            if len(parts) == 1:
                return parts[0]
            out = rows(hw)
            b.op("sum", 2, dz=parts[0].data_ptr(), add=parts[1].data_ptr(), x2=parts[2].data_ptr() if len(parts) > 2 else None,
                 out=out.data_ptr(), height=hw[0], width=hw[1], channels=C)
            return out

        def norm(name, bn, dy, z, stats, out, hw, second=None, alpha=0.0):
            """kind 3 on column views: ``dy``, ``z`` (and the second norm's) and ``out`` carry their own row strides."""
            dgam, dbet = b.new((C,), torch.float32), b.new((C,), torch.float32)
            b.grads[name + ".1.weight"], b.grads[name + ".1.bias"] = dgam, dbet
            extra = {}
            if second is not None:
                name2, bn2, z2, stats2, out2 = second
                dgam2, dbet2 = b.new((C,), torch.float32), b.new((C,), torch.float32)
                b.grads[name2 + ".1.weight"], b.grads[name2 + ".1.bias"] = dgam2, dbet2
                extra = dict(x2=z2.data_ptr(), stats2=stats2.data_ptr(), gamma2=bn2.weight.data_ptr(), beta2=bn2.bias.data_ptr(),
                             out2=out2.data_ptr(), dgamma2=dgam2.data_ptr(), dbeta2=dbet2.data_ptr(), alpha=float(alpha))
            b.op(name + " (norm)", 3, dz=dy.data_ptr(), x=z.data_ptr(), stats=stats.data_ptr(), gamma=bn.weight.data_ptr(),
                 beta=bn.bias.data_ptr(), out=out.data_ptr(), dgamma=dgam.data_ptr(), dbeta=dbet.data_ptr(), height=hw[0],
                 width=hw[1], channels=C, act=1, ld_dz=dy.stride(1), ld_x=z.stride(1), ld_out=out.stride(1), **extra)

        def conv_bwd(name, conv, dz, x, hw, want_dx=True):
            """wgrad (+ dgrad) of a grouped / 3x3 convolution whose input ``x`` has the map size ``hw``."""
            k, s, g = conv.kernel_size[0], conv.stride[0], conv.groups
            dw = b.grads[name + ".0.weight"] = b.new(tuple(conv.weight.shape), torch.float32)
            geo = dict(height=hw[0], width=hw[1], channels=C, out_channels=C, groups=g, kernel_size=k, stride=s)
            b.op(name + " (wgrad)", 1, dz=dz.data_ptr(), x=x.data_ptr(), ld_x=x.stride(1), dweight=dw.data_ptr(), **geo)
            if not want_dx:
                return None
            packed = self._train_weights(conv)[1]
            b.keep.append(packed)
            dx = rows(hw)
            b.op(name + " (dgrad)", 0, dz=dz.data_ptr(), weight=packed.data_ptr(), out=dx.data_ptr(), **geo)
            return dx

        def conv_norm_bwd(name, m, dy, hw_in, hw_out):
            """Lateral or down-sampler: the gradient at its input."""
            conv, bn = m[0], m[1]
            z, x = acts[name + ".z"], acts[name + ".in"]
            dz = rows(hw_out)
            norm(name, bn, dy, z, acts[name + ".stats"], dz, hw_out)
            if conv.kernel_size[0] == 3:
                return conv_bwd(name, conv, dz, x, hw_in)
            dw = b.grads[name + ".0.weight"] = b.new(tuple(conv.weight.shape), torch.float32)
            dx, w2d = rows(hw_in), conv.weight.detach()[:, :, 0, 0]
            host(lambda: (torch.matmul(dz.reshape(-1, C).t(), x.reshape(-1, C), out=dw.view(C, C)),
                          torch.matmul(dz, w2d, out=dx)))
            return dx

        pending: Dict[str, Tensor] = {}   # the 1x1 weight gradients of the CSP layers, by half

        def csp_bwd(name, layer, d_out, hw, first_hw, upsample):
            """``(gradient at first (at first_hw when up-sampled), gradient at second)``."""
            dcur = d_out
            for j in reversed(range(len(layer.bottlenecks))):
                blk, bname = layer.bottlenecks[j], f"{name}.bottlenecks.{j}"
                se, s = blk.se_module, acts[bname + ".s"]
                R = se.se_module[0].weight.shape[0]
                ds = rows(hw)
                gr = {k: b.new(tuple(p.shape), torch.float32) for k, p in
                      (("conv_mask.weight", se.conv_mask.weight), ("conv_mask.bias", se.conv_mask.bias),
                       ("se_module.0.weight", se.se_module[0].weight), ("se_module.2.weight", se.se_module[2].weight))}
                for k, t in gr.items():
                    b.grads[f"{bname}.se_module.{k}"] = t
                b.op(bname + " (gate)", 4, dz=dcur.data_ptr(), x=s.data_ptr(), x2=acts[bname + ".logits"].data_ptr(),
                     stats=acts[bname + ".saved"].data_ptr(), gamma=se.conv_mask.weight.data_ptr(),
                     weight=se.se_module[0].weight.data_ptr(), weight2=se.se_module[2].weight.data_ptr(), out=ds.data_ptr(),
                     dgamma=gr["conv_mask.weight"].data_ptr(), dbeta=gr["conv_mask.bias"].data_ptr(),
                     dweight=gr["se_module.0.weight"].data_ptr(), dweight2=gr["se_module.2.weight"].data_ptr(), height=hw[0],
                     width=hw[1], channels=C, hidden=R)
                dz3, dz1 = rows(hw), rows(hw)
                norm(bname + ".conv1", blk.conv1[1], ds, acts[bname + ".conv1.z"], acts[bname + ".conv1.stats"], dz3, hw,
                     second=(bname + ".conv2", blk.conv2[1], acts[bname + ".conv2.z"], acts[bname + ".conv2.stats"], dz1),
                     alpha=float(blk.alpha))
                x = acts[bname + ".in"]
                dx3 = conv_bwd(bname + ".conv1", blk.conv1[0], dz3, x, hw)
                dx1 = conv_bwd(bname + ".conv2", blk.conv2[0], dz1, x, hw)
                dcur = total([dx3, dx1, dcur], hw)
            zz_names = (name + ".conv1", name + ".conv2")
            dzz = rows(hw, 2 * C)
            for half, (cname, conv, dy) in enumerate(zip(zz_names, (layer.conv1, layer.conv2), (dcur, d_out))):
                norm(cname, conv[1], dy, acts[cname + ".z"], acts[cname + ".stats"], dzz[:, :, half * C:(half + 1) * C], hw)
            first, second, wc = acts[name + ".first"], acts[name + ".second"], acts[name + ".weight"]
            d_second, d_first = rows(hw), rows(first_hw)
            dwf, dws = b.new((2 * C, C), torch.float32), b.new((2 * C, C), torch.float32)
            pending[name] = (dwf, dws)
            dcoarse = dzz
            if upsample:
                dcoarse = rows(first_hw, 2 * C)
                b.op(name + " (upsample)", 5, dz=dzz.data_ptr(), out=dcoarse.data_ptr(), height=hw[0], width=hw[1], channels=2 * C,
                     src_height=first_hw[0], src_width=first_hw[1])
            host(lambda: (torch.matmul(dzz, wc[:, C:], out=d_second),
                          torch.matmul(dzz.reshape(-1, 2 * C).t(), second.reshape(-1, C), out=dws),
                          torch.matmul(dcoarse, wc[:, :C], out=d_first),
                          torch.matmul(dcoarse.reshape(-1, 2 * C).t(), first.reshape(-1, C), out=dwf)))
            return d_first, d_second

        cots = [None if c is None else c.to(torch.float32).contiguous() for c in cotangents]
        b.keep.extend(c for c in cots if c is not None)
        zero = lambda hw: torch.zeros((B, hw[0] * hw[1], C), device=b.device)   # noqa: E731
        g_out = [c if c is not None else zero(shapes[i]) for i, c in enumerate(cots)]
        b.keep.extend(g_out)
        from_pan: List[Tensor] = [None] * L     # what pan block idx - 1 hands to high_idx
        for idx in range(L - 2, -1, -1):         # bottom-up path, from the last level down
            d_down, from_pan[idx + 1] = csp_bwd(f"pan_blocks.{idx}", self.pan_blocks[idx], g_out[idx + 1], shapes[idx + 1],
                                                shapes[idx + 1], False)
            dx = conv_norm_bwd(f"downsample_blocks.{idx}", self.downsample_blocks[idx], d_down, shapes[idx], shapes[idx + 1])
            g_out[idx] = total([g_out[idx], dx], shapes[idx])
        dxs: List[Tensor] = [None] * L
        g_inner = g_out[0]                       # the gradient at layer block idx - 1's output
        for idx in range(1, L):                  # top-down path, from the first level up
            d_high, dxs[idx - 1] = csp_bwd(f"layer_blocks.{idx - 1}", self.layer_blocks[idx - 1], g_inner, shapes[idx - 1],
                                           shapes[idx], True)
            g_high = total([d_high, from_pan[idx]], shapes[idx])
            g_inner = conv_norm_bwd(f"lateral_convs.{idx - 1}", self.lateral_convs[idx - 1], g_high, shapes[idx], shapes[idx])
        dxs[L - 1] = g_inner

        def finish():
            for name, (dwf, dws) in pending.items():
                dw = torch.cat([dwf, dws], 1)
                b.grads[name + ".conv1.0.weight"] = dw[:C].reshape(C, 2 * C, 1, 1)
                b.grads[name + ".conv2.0.weight"] = dw[C:].reshape(C, 2 * C, 1, 1)
        return b, hosts, finish, dxs

    def _train_backward(self, state: dict, cotangents, wanted, splits: int = 0):
        """Runs the backward plan on what the forward stored: ``({parameter name: fp32 gradient}, input gradients)``.  The
        ops between two library GEMMs go to ``sdetr_neck_bwd_run`` in one call."""
        b, hosts, finish, dxs = self.build_backward_plan(state["acts"], state["shapes"], cotangents)
        start = 0
        for index, call in hosts + [(len(b.ops), None)]:
            if index > start:
                self._run_plan(_hip.NeckBwdOpStruct, "sdetr_neck_bwd", b.ops[start:index], b.device)
                start = index
            if call is not None:
                call()
        finish()
        return b.grads, [dx if want else None for dx, want in zip(dxs, wanted)]

    def forward_memory(self, memory: Tensor, level_shapes: Sequence[Tuple[int, int]], differentiable: bool = False) -> Tensor:
        """``memory`` ``[B, sum h*w, C]`` -> the neck's output in the same layout
        (models/bricks/salience_transformer.py:185-192 without its transposes)."""
        sizes = [int(h) * int(w) for h, w in level_shapes]
        # (row ranges of the memory as they lie: the levels only enter the neck through ``_token_matmul``, which takes
        #  the batch stride as it is -- four copies of the pyramid less per step)
        levels = list(memory.split(sizes, 1))
        return torch.cat(self.forward_levels(levels, level_shapes, differentiable), 1)

    def forward(self, x: "OrderedDict[str, Tensor]"):
        keys = list(x.keys())
        feats = list(x.values())
        shapes = [tuple(f.shape[-2:]) for f in feats]
        outs = self.forward_levels([f.flatten(2).transpose(1, 2).contiguous() for f in feats], shapes)
        output = OrderedDict()
        for k, o, (h, w) in zip(keys, outs, shapes):
            output[k] = o.transpose(1, 2).reshape(o.shape[0], o.shape[2], h, w)
        if self.extra_block:  # F.max_pool2d(last, 1, 2, 0): every second pixel
            output["pool"] = list(output.values())[-1][:, :, ::2, ::2]
        return output


def build_neck(channels: int = 256, num_levels: int = 4, groups: int = 4) -> RepVGGPluXNetwork:
    """The neck of ``configs/salience_detr/salience_detr_resnet50_800_1333.py:57-63``."""
    return RepVGGPluXNetwork([channels] * num_levels, [channels] * num_levels, groups=groups,
                             norm_layer=nn.BatchNorm2d, activation=nn.SiLU)
