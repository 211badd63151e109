"""The FocalNet backbone in front of ``ChannelMapper`` (reference ``models/backbones/focalnet.py``): DESIGN.md §4
"FocalNet backbone".

``FocalNetBackbone(arch, weights=None, return_indices=(0, 1, 2, 3), freeze_indices=(), **kwargs)`` has the reference's
constructor, ``num_channels`` and state-dict keys: those of its ``nn.Sequential(feature_extractor, PostProcess)``, i.e.
``0.patch_embed.*``, ``0.layers.{i}.blocks.{j}.*``, ``0.layers.{i}.downsample.*`` (for ``i < max(return_indices)``; later
stages are not held) and ``1.norm{i}.*``.  ``arch`` is one of ``ARCHS`` (``focalnet_tiny_srf`` .. ``focalnet_huge_fl4``)
or ``None`` with ``embed_dim`` / ``depths`` / ... in ``kwargs`` (which also override an arch's).  ``forward(x)`` returns
``{"layers.{i}.blocks": map}`` for ``i in return_indices``: fp32 NCHW, each after its ``norm{i}``.  ``weights`` is a state
dict (optionally under ``"model"``) or a local file path, loaded non-strictly with shape filtering; nothing is ever
downloaded.

How it runs (inference: grad disabled, or nothing that requires grad) -- ``csrc/focalnet.hip``, one plan, one
``sdetr_focalnet_run`` call per forward.  The residual stream is channels-last fp32 in every mode:
  * patch embedding: the conv (7x7 stride 4 padding 2 / 3x3 stride 2 padding 1, or the 4x4 / 2x2 patchify) as an implicit
    GEMM whose output size is ``ceil(H / patch)`` -- the reference's zero padding up to a patch multiple --, then LayerNorm;
  * focal modulation: ``f`` (one GEMM, fp32 rows ``[q | ctx | gates]``, width padded to a multiple of 32), one launch per
    focal level (depthwise k x k + GELU, gated accumulation; the last leaves per-tile channel sums), the modulator finish
    (mean in tile order, ``ctx_all + gelu(mean) * gate``), ``h`` with the ``* q`` epilogue (``normalize_modulator`` folded
    into its weight), an optional LayerNorm, ``proj``;
  * post-LN blocks (large / xlarge / huge): ``x + gamma * LN(branch)`` is one LayerNorm launch with ``gamma`` folded into
    its affine; pre-LN blocks: LayerNorm -> A operand, ``gamma`` folded into ``proj`` / ``fc2``, residual in the epilogue;
  * a returned stage's ``norm{i}`` writes the fp32 NCHW map through LDS; the stream goes on un-normed.
``set_dtype(bfloat16 | float16)`` takes one 16-bit product with fp32 accumulation and 16-bit GEMM A operands; depthwise
work, gates, means, LayerNorm statistics and ``q`` stay fp32.  A call with grad enabled on something that requires grad
takes the plain-torch composite, which is the autograd path; FocalNet backward in HIP is out of scope.  A CPU tensor on
the HIP form raises: the hot path has no CPU fallback.
"""
from functools import partial
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import _hip
from .backbone_base import HipBackbone, StochasticDepth
from .derived import derived
from .hip_module import PlanBuilder

MAX_CHANNELS = 3072          # a LayerNorm row in registers (csrc/backbone_rows_core.h)
FOCAL_KERNELS = (3, 5, 7, 9)


class Mlp(nn.Module):
    def __init__(self, dim: int, hidden: int, dropout: float = 0.0):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.act = nn.GELU()
        self.fc2 = nn.Linear(hidden, dim)
        self.drop = nn.Dropout(dropout)

    def forward(self, x: Tensor) -> Tensor:
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


class FocalModulation(nn.Module):
    """``x [B, H, W, C]`` -> ``proj(q * h(ctx_all))``: ``f`` gives ``q``, the context and ``focal_level + 1`` gates per
    pixel; level ``l`` is a depthwise ``focal_window + focal_factor * l`` conv + GELU of the previous level, gated and
    summed; the last level's mean over the map (through GELU) enters with the last gate."""

    def __init__(self, dim: int, focal_level: int, focal_window: int, focal_factor: int = 2, proj_drop: float = 0.0,
                 use_postln_in_modulation: bool = False, normalize_modulator: bool = False):
        super().__init__()
        self.dim, self.focal_level = dim, focal_level
        self.use_postln_in_modulation, self.normalize_modulator = use_postln_in_modulation, normalize_modulator
        self.f = nn.Linear(dim, 2 * dim + focal_level + 1)
        self.h = nn.Conv2d(dim, dim, kernel_size=1)
        self.act = nn.GELU()
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        self.focal_layers = nn.ModuleList()
        if use_postln_in_modulation:
            self.ln = nn.LayerNorm(dim)
        for level in range(focal_level):
            k = focal_window + focal_factor * level
            self.focal_layers.append(nn.Sequential(nn.Conv2d(dim, dim, k, padding=k // 2, groups=dim, bias=False), nn.GELU()))

    def forward(self, x: Tensor) -> Tensor:
        c, levels = self.dim, self.focal_level
        q, ctx, gates = self.f(x).permute(0, 3, 1, 2).contiguous().split((c, c, levels + 1), 1)
        total = 0
        for level, layer in enumerate(self.focal_layers):
            ctx = layer(ctx)
            total = total + ctx * gates[:, level:level + 1]
        total = total + self.act(ctx.mean(2, keepdim=True).mean(3, keepdim=True)) * gates[:, levels:]
        if self.normalize_modulator:
            total = total / (levels + 1)
        out = (q * self.h(total)).permute(0, 2, 3, 1).contiguous()
        if self.use_postln_in_modulation:
            out = self.ln(out)
        return self.proj_drop(self.proj(out))


class FocalModulationBlock(nn.Module):
    def __init__(self, dim: int, mlp_ratio: float, focal_level: int, focal_window: int, dropout: float,
                 stochastic_depth_prob: float, norm_layer, use_postln: bool, use_postln_in_modulation: bool,
                 normalize_modulator: bool, use_layerscale: bool):
        super().__init__()
        self.use_postln, self.use_layerscale = use_postln, use_layerscale
        self.norm1 = norm_layer(dim)
        self.modulation = FocalModulation(dim, focal_level, focal_window, proj_drop=dropout,
                                          use_postln_in_modulation=use_postln_in_modulation,
                                          normalize_modulator=normalize_modulator)
        self.drop_path = StochasticDepth(stochastic_depth_prob, "row")
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(dim, int(dim * mlp_ratio), dropout)
        if use_layerscale:
            self.gamma_1 = nn.Parameter(torch.full((dim,), 1e-4))
            self.gamma_2 = nn.Parameter(torch.full((dim,), 1e-4))
        else:
            self.gamma_1 = self.gamma_2 = 1.0

    def forward(self, x: Tensor) -> Tensor:
        if self.use_postln:
            x = x + self.drop_path(self.gamma_1 * self.norm1(self.modulation(x)))
            return x + self.drop_path(self.gamma_2 * self.norm2(self.mlp(x)))
        x = x + self.drop_path(self.gamma_1 * self.modulation(self.norm1(x)))
        return x + self.drop_path(self.gamma_2 * self.mlp(self.norm2(x)))


class PatchEmbed(nn.Module):
    """``[B, H, W, C]`` zero-padded at the bottom / right to a multiple of ``patch_size``, a strided conv, LayerNorm.  The
    overlapped form is 7x7 stride 4 padding 2 (stem) or 3x3 stride 2 padding 1."""

    def __init__(self, in_channels: int, out_channels: int, patch_size: Sequence[int], norm_layer, use_conv_embed: bool,
                 is_stem: bool):
        super().__init__()
        self.patch_size = tuple(patch_size)
        if use_conv_embed:
            k, s, p = (7, 4, 2) if is_stem else (3, 2, 1)
            self.proj = nn.Conv2d(in_channels, out_channels, kernel_size=k, stride=s, padding=p)
        else:
            self.proj = nn.Conv2d(in_channels, out_channels, kernel_size=self.patch_size, stride=self.patch_size)
        self.norm = norm_layer(out_channels)

    def forward(self, x: Tensor) -> Tensor:
        h, w = x.shape[-3], x.shape[-2]
        x = F.pad(x, (0, 0, 0, -w % self.patch_size[1], 0, -h % self.patch_size[0]))
        return self.norm(self.proj(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1))


class FocalStage(nn.Module):
    def __init__(self, blocks: List[nn.Module], downsample: Optional[nn.Module]):
        super().__init__()
        self.blocks = nn.Sequential(*blocks)
        if downsample is not None:
            self.downsample = downsample


class FocalNet(nn.Module):
    """The reference's ``FocalNet`` as its feature extractor keeps it: ``num_stages`` stages, the last one without its
    down-sampler.  The stochastic-depth probabilities count the blocks of the WHOLE ``depths``, as the reference's do."""

    def __init__(self, embed_dim: int, depths: Sequence[int], patch_size: Sequence[int] = (4, 4), mlp_ratio: float = 4.0,
                 dropout: float = 0.0, stochastic_depth_prob: float = 0.3, norm_layer=None,
                 focal_levels: Sequence[int] = (3, 3, 3, 3), focal_windows: Sequence[int] = (3, 3, 3, 3),
                 use_conv_embed: bool = False, use_postln: bool = False, use_postln_in_modulation: bool = False,
                 use_layerscale: bool = False, normalize_modulator: bool = False, num_stages: Optional[int] = None):
        super().__init__()
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-5)
        num_stages = len(depths) if num_stages is None else num_stages
        self.patch_embed = PatchEmbed(3, embed_dim, patch_size, norm_layer, use_conv_embed, True)
        self.pos_drop = nn.Dropout(dropout)
        self.layers = nn.ModuleList()
        total, block_id = sum(depths), 0
        for i in range(num_stages):
            dim = embed_dim * 2 ** i
            blocks = []
            for _ in range(depths[i]):
                sd_prob = stochastic_depth_prob * block_id / (total - 1) if total > 1 else 0.0
                blocks.append(FocalModulationBlock(dim, mlp_ratio, focal_levels[i], focal_windows[i], dropout, sd_prob,
                                                   norm_layer, use_postln, use_postln_in_modulation, normalize_modulator,
                                                   use_layerscale))
                block_id += 1
            down = PatchEmbed(dim, 2 * dim, (2, 2), norm_layer, use_conv_embed, False) if i < num_stages - 1 else None
            self.layers.append(FocalStage(blocks, down))
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.LayerNorm):
                nn.init.ones_(m.weight)
                nn.init.zeros_(m.bias)


class PostNorms(nn.Module):
    """``norm{i}`` per returned stage (the reference's ``PostProcess``)."""

    def __init__(self, channels: Sequence[int], return_indices: Sequence[int], norm_layer):
        super().__init__()
        for c, i in zip(channels, return_indices):
            self.add_module(f"norm{i}", norm_layer(c))


def _arch(embed_dim, depths, sd, levels, window, big=False, **flags):
    cfg = dict(embed_dim=embed_dim, patch_size=(4, 4), depths=depths, stochastic_depth_prob=sd, focal_levels=(levels,) * 4,
               focal_windows=(window,) * 4, use_conv_embed=big, use_postln=big, use_postln_in_modulation=False,
               use_layerscale=big, normalize_modulator=False)
    cfg.update(flags)
    return cfg


ARCHS = {
    "focalnet_tiny_srf": _arch(96, (2, 2, 6, 2), 0.2, 2, 3),
    "focalnet_tiny_lrf": _arch(96, (2, 2, 18, 2), 0.2, 3, 3),
    "focalnet_small_srf": _arch(96, (2, 2, 18, 2), 0.3, 2, 3),
    "focalnet_small_lrf": _arch(96, (2, 2, 18, 2), 0.3, 3, 3),
    "focalnet_base_srf": _arch(128, (2, 2, 18, 2), 0.5, 2, 3),
    "focalnet_base_lrf": _arch(128, (2, 2, 18, 2), 0.5, 3, 3),
    "focalnet_large_lrf": _arch(192, (2, 2, 18, 2), 0.5, 3, 5, big=True),
    "focalnet_large_lrf_fl4": _arch(192, (2, 2, 18, 2), 0.5, 4, 3, big=True, normalize_modulator=True),
    "focalnet_xlarge_lrf": _arch(256, (2, 2, 18, 2), 0.5, 3, 5, big=True),
    "focalnet_xlarge_lrf_fl4": _arch(256, (2, 2, 18, 2), 0.5, 4, 3, big=True, normalize_modulator=True),
    "focalnet_huge_fl3": _arch(352, (2, 2, 18, 2), 0.5, 3, 3, big=True, use_postln_in_modulation=True),
    "focalnet_huge_fl4": _arch(352, (2, 2, 18, 2), 0.5, 4, 3, big=True, use_postln_in_modulation=True),
}


def _ceil_div(a: int, b: int) -> int:
    return -(-a // b)


class FocalNetBackbone(HipBackbone):
    def __init__(self, arch: Optional[str], weights: Union[None, str, Dict[str, Tensor]] = None,
                 return_indices: Tuple[int, ...] = (0, 1, 2, 3), freeze_indices: Tuple[int, ...] = (), **kwargs):
        super().__init__()
        if arch is not None and arch not in ARCHS:
            raise ValueError(f"Expected architecture in {tuple(ARCHS)} but got {arch}")
        config = dict(ARCHS[arch]) if arch is not None else {}
        config.update({k: v for k, v in kwargs.items() if v is not None})
        config.pop("url", None)
        if "embed_dim" not in config or "depths" not in config:
            raise ValueError("FocalNetBackbone: arch=None needs embed_dim=... and depths=(...)")
        self.return_indices = tuple(return_indices)
        depths = tuple(config["depths"])
        if not self.return_indices or max(self.return_indices) >= len(depths) or min(self.return_indices) < 0:
            raise ValueError(f"FocalNetBackbone: return_indices {self.return_indices} do not fit {len(depths)} stages")
        self.num_stages = max(self.return_indices) + 1
        self.config = dict(config)
        norm_layer = config.get("norm_layer") or partial(nn.LayerNorm, eps=1e-5)
        self.num_channels = [config["embed_dim"] * 2 ** i for i in self.return_indices]
        self.add_module("0", FocalNet(num_stages=self.num_stages, **config))
        self.add_module("1", PostNorms(self.num_channels, self.return_indices, norm_layer))
        self.compute_dtype = torch.float32
        if weights is not None:
            self.load_weights(weights)
        if len(freeze_indices) > 0:
            self._freeze(self.body.patch_embed)
        for i in freeze_indices:
            if i < self.num_stages:
                self._freeze(self.body.layers[i])

    @property
    def body(self) -> FocalNet:
        return self._modules["0"]

    @property
    def post(self) -> PostNorms:
        return self._modules["1"]

    # ------------------------------------------------------------------------------------------ form checks
    def _embeds(self) -> List[PatchEmbed]:
        return [self.body.patch_embed] + [s.downsample for s in self.body.layers if hasattr(s, "downsample")]

    def hip_form(self) -> bool:
        """True when every layer is one the HIP kernels serve: widths (and MLP widths) that are multiples of 32 up to
        ``MAX_CHANNELS``, focal kernels in ``FOCAL_KERNELS``, ``nn.LayerNorm`` norms, square patches up to 4."""
        norms = [getattr(self.post, f"norm{i}") for i in self.return_indices]
        for emb in self._embeds():
            k, s = emb.proj.kernel_size, emb.proj.stride
            if k[0] != k[1] or s[0] != s[1] or k[0] > 7 or s[0] > 4 or emb.patch_size != tuple(s):
                return False
            norms.append(emb.norm)
        for stage in self.body.layers:
            for blk in stage.blocks:
                mod = blk.modulation
                c = mod.dim
                if c % 32 or c > MAX_CHANNELS or blk.mlp.fc1.out_features % 32:
                    return False
                if any(layer[0].kernel_size[0] not in FOCAL_KERNELS for layer in mod.focal_layers) or not mod.focal_layers:
                    return False
                norms += [blk.norm1, blk.norm2] + ([mod.ln] if mod.use_postln_in_modulation else [])
        return all(type(n) is nn.LayerNorm and len(n.normalized_shape) == 1 and n.elementwise_affine and n.bias is not None
                   for n in norms)

    def forward_torch(self, x: Tensor) -> Dict[str, Tensor]:
        """The differentiable composite (the holder modules themselves) on the input's device."""
        outs = {}
        x = self.body.pos_drop(self.body.patch_embed(x.permute(0, 2, 3, 1)))
        for i, stage in enumerate(self.body.layers):
            x = stage.blocks(x)
            if i in self.return_indices:
                outs[f"layers.{i}.blocks"] = getattr(self.post, f"norm{i}")(x).permute(0, 3, 1, 2).contiguous()
            if hasattr(stage, "downsample"):
                x = stage.downsample(x)
        return {f"layers.{i}.blocks": outs[f"layers.{i}.blocks"] for i in self.return_indices}

    def _taps(self, conv: nn.Conv2d) -> Tensor:
        """The depthwise taps tap-major ``[k * k, C]``, fp32."""
        def build():
            c, k = conv.weight.shape[0], conv.weight.shape[-1]
            return conv.weight.detach().to(torch.float32).reshape(c, k * k).t().contiguous()
        return derived(conv, "focalnet_taps", (conv.weight,), build)

    def build_plan(self, x: Tensor, splits: int = 0):
        """The op list of one forward on ``x`` ``[B, 3, H, W]`` (fp32 NCHW on the device): ``(ops, outputs, keep, names)``:
        ``outputs`` the returned fp32 NCHW maps, ``keep`` every tensor the plan points into, ``names`` one label per op.
        The buffers of a stage are shared by its blocks (the launches of a plan run in order on one stream)."""
        p16 = self._precision() == 1
        act = self.compute_dtype if p16 else torch.float32
        batch = x.shape[0]
        pb = PlanBuilder(_hip.FocalnetOpStruct, x, batch=batch, height=1, width=1, out_height=1, out_width=1, kernel_size=1,
                         stride=1, splits=splits)
        new, op, keep, outputs = pb.new, pb.op, pb.keep, pb.outputs

        def gemm(name, kind, layer, src, out, h, w, ho=None, wo=None, layout=0, **kw):
            pack = {k: kw.pop(k) for k in ("scale", "scale_bias", "pad_to") if k in kw}
            packed, bias = self._packed(layer, layout, **pack)
            keep.extend((packed, bias))
            k, s, p = ((layer.kernel_size[0], layer.stride[0], layer.padding[0]) if isinstance(layer, nn.Conv2d) else (1, 1, 0))
            op(name, kind, x=src.data_ptr(), weight=packed.data_ptr(), bias=bias.data_ptr(), out=out.data_ptr(),
               in_channels=layer.weight.shape[1], height=h, width=w, out_channels=bias.numel(), out_height=ho or h,
               out_width=wo or w, kernel_size=k, stride=s, padding=p, x_nchw=layout, **kw)

        def layer_norm(name, norm, src, out, h, w, c, out_f32, scale=None, residual=None, out2=None, nchw=False):
            pb.layer_norm(name, 6 if nchw else 5, self._affine(norm, scale), norm.eps, src, out, h, w, c, out_f32,
                          residual=_hip.ptr(residual), out2=_hip.ptr(out2))

        def embed(name, emb, src, h, w, layout, copy):
            """conv + LayerNorm of a patch embedding: the new stream, its 16-bit copy (or None), and its size"""
            ps = emb.patch_size[0]
            ho, wo, co = _ceil_div(h, ps), _ceil_div(w, ps), emb.proj.weight.shape[0]
            raw = new((batch, ho, wo, co), torch.float32)
            gemm(name + ".proj", 0, emb.proj, src, raw, h, w, ho, wo, layout)
            stream = new((batch, ho, wo, co), torch.float32)
            stream16 = new((batch, ho, wo, co), act) if copy else None
            layer_norm(name + ".norm", emb.norm, raw, stream, ho, wo, co, True, out2=stream16)
            return stream, stream16, ho, wo, co

        postln = bool(self.config.get("use_postln", False))
        copy = p16 and postln                       # the post-LN stream is itself a GEMM A operand
        stream, stream16, h, w, c = embed("0.patch_embed", self.body.patch_embed, x, x.shape[2], x.shape[3], 1, copy)
        for i, stage in enumerate(self.body.layers):
            mod0 = stage.blocks[0].modulation
            levels, hidden = mod0.focal_level, stage.blocks[0].mlp.fc1.out_features
            fw = _ceil_div(2 * c + levels + 1, 32) * 32
            rows = (batch, h, w)
            frow, ctx_all = new(rows + (fw,), torch.float32), new(rows + (c,), torch.float32)
            ctx = [new(rows + (c,), torch.float32) for _ in range(min(2, levels - 1))]
            a_in = new(rows + (c,), act)                            # LayerNorm / finish output: a GEMM A operand
            a_mod = new(rows + (c,), act)
            branch = new(rows + (c,), torch.float32)
            mid = new(rows + (hidden,), act)
            for j, blk in enumerate(stage.blocks):
                prefix = f"0.layers.{i}.blocks.{j}"
                mod = blk.modulation
                g1 = blk.gamma_1 if blk.use_layerscale else None
                g2 = blk.gamma_2 if blk.use_layerscale else None
                if postln:
                    src = stream16 if p16 else stream
                else:
                    layer_norm(prefix + ".norm1", blk.norm1, stream, a_in, h, w, c, False)
                    src = a_in
                gemm(prefix + ".modulation.f", 0, mod.f, src, frow, h, w, pad_to=32)
                for level, layer in enumerate(mod.focal_layers):
                    taps = self._taps(layer[0])
                    keep.append(taps)
                    last = level == levels - 1
                    # level 0 reads f's rows at column C; a later level the previous one's output
                    src_ptr = frow.data_ptr() + 4 * c if level == 0 else ctx[(level - 1) % 2].data_ptr()
                    op(prefix + f".modulation.focal_layers.{level}", 3, x=src_ptr, weight=taps.data_ptr(),
                       q=frow.data_ptr() + 4 * (2 * c + level), out=None if last else ctx[level % 2].data_ptr(),
                       out2=ctx_all.data_ptr(), in_channels=c, height=h, width=w, out_channels=c,
                       kernel_size=layer[0].kernel_size[0], x_ld=fw if level == 0 else c, q_ld=fw,
                       accumulate=0 if level == 0 else 1, last=1 if last else 0)
                op(prefix + ".modulation.finish", 4, x=ctx_all.data_ptr(), q=frow.data_ptr() + 4 * (2 * c + levels),
                   out=a_mod.data_ptr(), in_channels=c, height=h, width=w, out_channels=c, q_ld=fw)
                norm_scale = 1.0 / (levels + 1) if mod.normalize_modulator else None
                if mod.use_postln_in_modulation:
                    gemm(prefix + ".modulation.h", 2, mod.h, a_mod, branch, h, w, scale=norm_scale, scale_bias=False,
                         q=frow.data_ptr(), q_ld=fw, out_f32=1)
                    layer_norm(prefix + ".modulation.ln", mod.ln, branch, a_in, h, w, c, False)
                    a_proj = a_in
                else:
                    gemm(prefix + ".modulation.h", 2, mod.h, a_mod, a_in, h, w, scale=norm_scale, scale_bias=False,
                         q=frow.data_ptr(), q_ld=fw)
                    a_proj = a_in
                if postln:
                    gemm(prefix + ".modulation.proj", 0, mod.proj, a_proj, branch, h, w)
                    layer_norm(prefix + ".norm1", blk.norm1, branch, stream, h, w, c, True, scale=g1, residual=stream,
                               out2=stream16)
                    gemm(prefix + ".mlp.fc1", 1, blk.mlp.fc1, stream16 if p16 else stream, mid, h, w)
                    gemm(prefix + ".mlp.fc2", 0, blk.mlp.fc2, mid, branch, h, w)
                    layer_norm(prefix + ".norm2", blk.norm2, branch, stream, h, w, c, True, scale=g2, residual=stream,
                               out2=stream16)
                else:
                    gemm(prefix + ".modulation.proj", 0, mod.proj, a_proj, stream, h, w, scale=g1, residual=stream.data_ptr())
                    layer_norm(prefix + ".norm2", blk.norm2, stream, a_in, h, w, c, False)
                    gemm(prefix + ".mlp.fc1", 1, blk.mlp.fc1, a_in, mid, h, w)
                    gemm(prefix + ".mlp.fc2", 0, blk.mlp.fc2, mid, stream, h, w, scale=g2, residual=stream.data_ptr())
            if i in self.return_indices:
                nchw = new((batch, c, h, w), torch.float32)
                outputs[f"layers.{i}.blocks"] = nchw
                layer_norm(f"1.norm{i}", getattr(self.post, f"norm{i}"), stream, nchw, h, w, c, True, nchw=True)
            if hasattr(stage, "downsample"):
                src = stream
                if p16 and stream16 is None:                        # the pre-LN stream exists in fp32 only
                    src = new(rows + (c,), act)
                    op(f"0.layers.{i}.downsample.cast", 7, x=stream.data_ptr(), out=src.data_ptr(), in_channels=c, height=h,
                       width=w, out_channels=c)
                elif p16:
                    src = stream16
                stream, stream16, h, w, c = embed(f"0.layers.{i}.downsample", stage.downsample, src, h, w, 0, copy)
        outputs = {f"layers.{i}.blocks": outputs[f"layers.{i}.blocks"] for i in self.return_indices}
        return pb.ops, outputs, keep, pb.names

    def forward_hip(self, x: Tensor, splits: int = 0) -> Dict[str, Tensor]:
        x = self._check_image(x)
        ops, outputs, keep, _ = self.build_plan(x, splits)
        self._run_plan(_hip.FocalnetOpStruct, "sdetr_focalnet", ops, x.device)
        return outputs
