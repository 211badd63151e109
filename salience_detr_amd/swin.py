"""The Swin backbone, V1, in front of ``ChannelMapper`` (reference ``models/backbones/swin.py``): DESIGN.md §4 "Swin
backbone".

``SwinBackbone(arch, weights=None, return_indices=(0, 1, 2, 3), freeze_indices=(), **kwargs)`` has the reference's
constructor, ``num_channels`` and state-dict keys: those of its ``nn.Sequential(feature_extractor, PostProcess)``, i.e.
``0.features.0.{0,2}.*`` (stem conv and LayerNorm), ``0.features.{2i+1}.{j}.*`` (the blocks of stage ``i``: ``norm1``,
``attn.relative_position_bias_table``, ``attn.relative_position_index`` -- an integer buffer --, ``attn.qkv``,
``attn.proj``, ``norm2``, ``mlp.0``, ``mlp.3``) and ``0.features.{2i+2}.{reduction.weight,norm.*}`` (patch merging) for
``i < max(return_indices)``; later stages are not held.  ``arch`` is one of ``ARCHS`` (``swin_t`` .. ``swin_l_384``) or
``None`` with ``embed_dim`` / ``depths`` / ``num_heads`` / ``window_size`` in ``kwargs`` (which also override an arch's).
The V2 names raise: cosine attention, ``cpb_mlp`` and ``PatchMergingV2`` are not built.  ``forward(x)`` returns
``{"features.{2i+1}": map}`` for ``i in return_indices``: fp32 NCHW, the stage's stream as it is (the reference's
``PostProcess`` only permutes).  ``weights`` is a state dict (optionally under ``"model"``) or a local file path, loaded
non-strictly with shape filtering; nothing is ever downloaded.

How it runs (inference: grad disabled, or nothing that requires grad) -- ``csrc/swin.hip``, one plan, one
``sdetr_swin_run`` call per forward.  The residual stream is channels-last fp32 in every mode:
  * stem: the 4x4 stride-4 conv on the fp32 NCHW canvas as an implicit GEMM (floor output size, no padding), LayerNorm;
  * a block is 7 launches: LayerNorm -> qkv (GEMM, rows in the compute dtype) -> window attention (one workgroup per
    window and head; the padding to a window multiple, the cyclic shift and its reverse are index arithmetic, the tokens of
    the padding carry the qkv bias) -> proj + residual -> LayerNorm -> fc1 + GELU -> fc2 + residual; the last fc2 of a
    returned stage also writes the fp32 NCHW map;
  * patch merging: the 2x2 gather + LayerNorm(4C) in one launch, then the ``reduction`` GEMM.
``set_dtype(bfloat16 | float16)`` takes one 16-bit product with fp32 accumulation and 16-bit rows between launches;
LayerNorm and softmax statistics and the stream stay fp32.  By default a call with grad enabled on something that
requires grad takes the plain-torch composite, which is the default autograd path.  Explicit arguments with a window other
than 7 / 12 or a head dimension other than 32 run the composite too (``hip_form()`` is False).  A CPU tensor on the HIP
form raises: the hot path has no CPU fallback.

Training in HIP (``set_train_form("hip")``, ``csrc/swin_backward.hip``; the interface and its autograd node are
``backbone_base.HipBackbone``'s, as are ``_trainable``, ``_first_trainable``, the test hooks and ``_run_backward``; this
module gives ``_sequence``, the stored state and ``_backward_ops``, its own kinds next to the emitters of the base's
``BackwardPlanBuilder``): a forward that needs autograd runs the same plan inside one autograd node.  Every block from
the lowest trainable module on gets buffers of its own (the stream at its input and after the attention branch, both LayerNorm outputs, the qkv rows, the attention
rows, the values before the GELU and after it), fc1 also stores its pre-GELU values (``aux``) and proj / fc2 multiply by
the branch's stochastic-depth factor per sample (``row_scale``; two draws per block, on the device, exactly as
``StochasticDepth`` draws them).  The backward is one ``sdetr_swin_bwd_run`` call over ``_backward_ops``: it stops below
the lowest trainable module and returns fp32 gradients for the parameters that require them, the relative position bias
tables included.  Served: ``hip_form()`` with a frozen stem, ``dropout == attention_dropout == 0``, an input without
gradient, float32 or bfloat16.  The stem's backward, a gradient to the image and float16 training are out of scope;
anything else raises at forward.
"""
from functools import partial
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import _hip
from .backbone_base import HipBackbone, Permute, StochasticDepth
from .derived import derived
from .hip_module import BackwardPlanBuilder, PlanBuilder

MAX_CHANNELS = 3072          # a LayerNorm row in registers (csrc/backbone_rows_core.h); the merging norm sees 4 C
WINDOWS = (7, 12)
HEAD_DIM = 32


def _axis_regions(padded: int, window: int, shift: int, device) -> Tensor:
    """The mask region of every coordinate of a rolled axis: 0 below ``padded - window``, 1 below ``padded - shift``,
    else 2; one region when the axis is not shifted."""
    c = torch.arange(padded, device=device)
    if shift == 0:
        return torch.zeros_like(c)
    return (c >= padded - window).long() + (c >= padded - shift).long()


class ShiftedWindowAttention(nn.Module):
    """Window attention with a relative position bias on ``[B, H, W, C]``: the map is zero-padded to multiples of the
    window, rolled by ``-shift`` on every axis longer than one window, cut into windows; pairs of tokens from different
    regions of the rolled map get -100."""

    def __init__(self, dim: int, window_size: Sequence[int], shift_size: Sequence[int], num_heads: int,
                 attention_dropout: float = 0.0, dropout: float = 0.0):
        super().__init__()
        if len(window_size) != 2 or len(shift_size) != 2:
            raise ValueError("window_size and shift_size must be of length 2")
        self.window_size, self.shift_size, self.num_heads = list(window_size), list(shift_size), num_heads
        self.attention_dropout, self.dropout = attention_dropout, dropout
        self.qkv = nn.Linear(dim, dim * 3)
        self.proj = nn.Linear(dim, dim)
        wh, ww = self.window_size
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * wh - 1) * (2 * ww - 1), num_heads))
        nn.init.trunc_normal_(self.relative_position_bias_table, std=0.02)
        ys, xs = torch.meshgrid(torch.arange(wh), torch.arange(ww), indexing="ij")
        dy = ys.reshape(-1, 1) - ys.reshape(1, -1) + wh - 1
        dx = xs.reshape(-1, 1) - xs.reshape(1, -1) + ww - 1
        self.register_buffer("relative_position_index", (dy * (2 * ww - 1) + dx).reshape(-1))

    def position_bias(self) -> Tensor:
        """``[heads, N, N]``: the table looked up per (query, key)."""
        n = self.window_size[0] * self.window_size[1]
        return self.relative_position_bias_table[self.relative_position_index].view(n, n, -1).permute(2, 0, 1).contiguous()

    def forward(self, x: Tensor) -> Tensor:
        b, h, w, c = x.shape
        (wh, ww), heads = self.window_size, self.num_heads
        ph, pw = -(-h // wh) * wh, -(-w // ww) * ww
        x = F.pad(x, (0, 0, 0, pw - w, 0, ph - h))
        sh = 0 if wh >= ph else self.shift_size[0]
        sw = 0 if ww >= pw else self.shift_size[1]
        rolled = sh + sw > 0
        if rolled:
            x = torch.roll(x, shifts=(-sh, -sw), dims=(1, 2))
        nh, nw, n = ph // wh, pw // ww, wh * ww
        tokens = x.view(b, nh, wh, nw, ww, c).permute(0, 1, 3, 2, 4, 5).reshape(b * nh * nw, n, c)
        q, k, v = self.qkv(tokens).reshape(-1, n, 3, heads, c // heads).permute(2, 0, 3, 1, 4).unbind(0)
        scores = (q * (c // heads) ** -0.5).matmul(k.transpose(-2, -1)) + self.position_bias().unsqueeze(0)
        if rolled:
            ids = 3 * _axis_regions(ph, wh, sh, x.device)[:, None] + _axis_regions(pw, ww, sw, x.device)[None, :]
            ids = ids.view(nh, wh, nw, ww).permute(0, 2, 1, 3).reshape(nh * nw, n)
            mask = torch.where(ids[:, None, :] != ids[:, :, None], -100.0, 0.0).to(scores.dtype)
            scores = (scores.view(b, nh * nw, heads, n, n) + mask[None, :, None]).view(-1, heads, n, n)
        p = F.dropout(F.softmax(scores, dim=-1), p=self.attention_dropout, training=self.training)
        out = p.matmul(v).transpose(1, 2).reshape(-1, n, c)
        out = F.dropout(self.proj(out), p=self.dropout, training=self.training)
        out = out.view(b, nh, nw, wh, ww, c).permute(0, 1, 3, 2, 4, 5).reshape(b, ph, pw, c)
        if rolled:
            out = torch.roll(out, shifts=(sh, sw), dims=(1, 2))
        return out[:, :h, :w, :].contiguous()


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim: int, num_heads: int, window_size: Sequence[int], shift_size: Sequence[int], mlp_ratio: float,
                 dropout: float, attention_dropout: float, stochastic_depth_prob: float, norm_layer):
        super().__init__()
        self.norm1 = norm_layer(dim)
        self.attn = ShiftedWindowAttention(dim, window_size, shift_size, num_heads, attention_dropout, dropout)
        self.stochastic_depth = StochasticDepth(stochastic_depth_prob, "row")
        self.norm2 = norm_layer(dim)
        hidden = int(dim * mlp_ratio)
        self.mlp = nn.Sequential(nn.Linear(dim, hidden), nn.GELU(), nn.Dropout(dropout), nn.Linear(hidden, dim),
                                 nn.Dropout(dropout))
        for m in self.mlp:
            if isinstance(m, nn.Linear):
                nn.init.xavier_uniform_(m.weight)
                nn.init.normal_(m.bias, std=1e-6)

    def forward(self, x: Tensor) -> Tensor:
        x = x + self.stochastic_depth(self.attn(self.norm1(x)))
        return x + self.stochastic_depth(self.mlp(self.norm2(x)))


class PatchMerging(nn.Module):
    """``[.., H, W, C]`` -> ``[.., ceil(H / 2), ceil(W / 2), 2 C]``: the 2 x 2 neighbours side by side (row parity first),
    zeros beyond an odd size, LayerNorm(4 C), a Linear without bias."""

    def __init__(self, dim: int, norm_layer):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = norm_layer(4 * dim)

    def forward(self, x: Tensor) -> Tensor:
        h, w = x.shape[-3], x.shape[-2]
        x = F.pad(x, (0, 0, 0, w % 2, 0, h % 2))
        x = torch.cat([x[..., dy::2, dx::2, :] for dx in (0, 1) for dy in (0, 1)], -1)
        return self.reduction(self.norm(x))


class SwinTransformer(nn.Module):
    """The reference's ``SwinTransformer`` as its feature extractor keeps it: ``features`` up to the last returned stage,
    that one without its merging layer, no ``norm`` / ``head``.  The stochastic-depth probabilities count the blocks of
    the WHOLE ``depths``, as the reference's do."""

    def __init__(self, patch_size: Sequence[int], embed_dim: int, depths: Sequence[int], num_heads: Sequence[int],
                 window_size: Sequence[int], mlp_ratio: float = 4.0, dropout: float = 0.0, attention_dropout: float = 0.0,
                 stochastic_depth_prob: float = 0.1, norm_layer=None, num_stages: Optional[int] = None):
        super().__init__()
        norm_layer = norm_layer or partial(nn.LayerNorm, eps=1e-5)
        num_stages = len(depths) if num_stages is None else num_stages
        patch = tuple(patch_size)
        layers: List[nn.Module] = [nn.Sequential(nn.Conv2d(3, embed_dim, kernel_size=patch, stride=patch),
                                                 Permute([0, 2, 3, 1]), norm_layer(embed_dim))]
        total, block_id = sum(depths), 0
        for i in range(num_stages):
            dim = embed_dim * 2 ** i
            blocks = []
            for j in range(depths[i]):
                sd_prob = stochastic_depth_prob * float(block_id) / (total - 1) if total > 1 else 0.0
                shift = [0 if j % 2 == 0 else w // 2 for w in window_size]
                blocks.append(SwinTransformerBlock(dim, num_heads[i], list(window_size), shift, mlp_ratio, dropout,
                                                   attention_dropout, sd_prob, norm_layer))
                block_id += 1
            layers.append(nn.Sequential(*blocks))
            if i < num_stages - 1:
                layers.append(PatchMerging(dim, norm_layer))
        self.features = nn.Sequential(*layers)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)


class PostProcess(nn.Module):
    """The reference's ``PostProcess``: channels-last maps to NCHW; no parameters."""

    def forward(self, feats: Dict[str, Tensor]) -> Dict[str, Tensor]:
        return {k: v.permute(0, 3, 1, 2) for k, v in feats.items()}


def _arch(embed_dim, depths, num_heads, window, sd):
    return dict(patch_size=(4, 4), embed_dim=embed_dim, depths=depths, num_heads=num_heads, window_size=(window, window),
                stochastic_depth_prob=sd)


ARCHS = {
    "swin_t": _arch(96, (2, 2, 6, 2), (3, 6, 12, 24), 7, 0.2),
    "swin_s": _arch(96, (2, 2, 18, 2), (3, 6, 12, 24), 7, 0.3),
    "swin_b": _arch(128, (2, 2, 18, 2), (4, 8, 16, 32), 7, 0.5),
    "swin_l": _arch(192, (2, 2, 18, 2), (6, 12, 24, 48), 7, 0.2),
    "swin_b_384": _arch(128, (2, 2, 18, 2), (4, 8, 16, 32), 12, 0.2),
    "swin_l_384": _arch(192, (2, 2, 18, 2), (6, 12, 24, 48), 12, 0.2),
}
V2_ARCHS = ("swin_v2_t", "swin_v2_b")


class SwinBackbone(HipBackbone):
    def __init__(self, arch: Optional[str], weights: Union[None, str, Dict[str, Tensor]] = None,
                 return_indices: Tuple[int, ...] = (0, 1, 2, 3), freeze_indices: Tuple[int, ...] = (), **kwargs):
        super().__init__()
        if arch in V2_ARCHS:
            raise ValueError(f"SwinBackbone: {arch} is a Swin V2 architecture (cosine attention, cpb_mlp, PatchMergingV2); "
                             f"V2 is not built, only the V1 architectures {tuple(ARCHS)}")
        if arch is not None and arch not in ARCHS:
            raise ValueError(f"Expected architecture in {tuple(ARCHS)} but got {arch}")
        config = dict(ARCHS[arch]) if arch is not None else {}
        config.update({k: v for k, v in kwargs.items() if v is not None})
        config.pop("url", None)
        config.pop("num_classes", None)
        for unbuilt in ("block", "downsample_layer"):
            if config.pop(unbuilt, None) is not None:
                raise ValueError(f"SwinBackbone: a custom {unbuilt} (Swin V2) is not built")
        missing = [k for k in ("embed_dim", "depths", "num_heads", "window_size") if k not in config]
        if missing:
            raise ValueError(f"SwinBackbone: arch=None needs {', '.join(k + '=...' for k in missing)}")
        config.setdefault("patch_size", (4, 4))
        self.return_indices = tuple(return_indices)
        depths = tuple(config["depths"])
        if not self.return_indices or max(self.return_indices) >= len(depths) or min(self.return_indices) < 0:
            raise ValueError(f"SwinBackbone: return_indices {self.return_indices} do not fit {len(depths)} stages")
        self.num_stages = max(self.return_indices) + 1
        self.config = dict(config)
        self.num_channels = [config["embed_dim"] * 2 ** i for i in self.return_indices]
        self.add_module("0", SwinTransformer(num_stages=self.num_stages, **config))
        self.add_module("1", PostProcess())
        self.compute_dtype = torch.float32
        if weights is not None:
            self.load_weights(weights)
        features = self.body.features
        if len(freeze_indices) > 0:
            self._freeze(features[0])
        for i in freeze_indices:
            for idx in (2 * i + 1, 2 * i + 2):
                if idx < len(features):
                    self._freeze(features[idx])

    @property
    def body(self) -> SwinTransformer:
        return self._modules["0"]

    def _remap_checkpoint_keys(self, weights: Dict[str, Tensor]) -> Dict[str, Tensor]:
        """A full ``SwinTransformer`` checkpoint (keys ``features.*``, ``norm.*``, ``head.*``) is taken too: what the
        extractor does not keep is dropped."""
        if not any(k.startswith("0.") for k in weights):
            weights = {"0." + k: v for k, v in weights.items()}
        return weights

    # ------------------------------------------------------------------------------------------ form checks
    def _stages(self):
        """``(i, blocks, merging or None)`` per held stage."""
        features = self.body.features
        for i in range(self.num_stages):
            yield i, features[2 * i + 1], (features[2 * i + 2] if 2 * i + 2 < len(features) else None)

    def hip_form(self) -> bool:
        """True when every layer is one the HIP kernels serve: a square patch up to 4, widths (and MLP widths) that are
        multiples of 32 with 4 C up to ``MAX_CHANNELS`` in front of a merging, square windows of 7 or 12 with one shift,
        head dimension 32, ``nn.LayerNorm`` norms."""
        stem = self.body.features[0]
        k, s = stem[0].kernel_size, stem[0].stride
        if k[0] != k[1] or k != s or k[0] > 4:
            return False
        norms = [stem[2]]
        for _, blocks, merging in self._stages():
            for blk in blocks:
                at = blk.attn
                c = at.qkv.in_features
                if c % 32 or c > MAX_CHANNELS or blk.mlp[0].out_features % 32 or c != at.num_heads * HEAD_DIM:
                    return False
                if at.window_size[0] != at.window_size[1] or at.window_size[0] not in WINDOWS:
                    return False
                if at.shift_size[0] != at.shift_size[1] or not 0 <= at.shift_size[0] < at.window_size[0]:
                    return False
                norms += [blk.norm1, blk.norm2]
            if merging is not None:
                if 4 * merging.dim > MAX_CHANNELS:
                    return False
                norms.append(merging.norm)
        return all(type(n) is nn.LayerNorm and len(n.normalized_shape) == 1 and n.elementwise_affine and n.bias is not None
                   for n in norms)

    def forward_torch(self, x: Tensor) -> Dict[str, Tensor]:
        """The differentiable composite (the holder modules themselves) on the input's device."""
        outs = {}
        features = self.body.features
        x = features[0](x)
        for i, blocks, merging in self._stages():
            x = blocks(x)
            if i in self.return_indices:
                outs[f"features.{2 * i + 1}"] = x
            if merging is not None:
                x = merging(x)
        outs = self._modules["1"](outs)
        return {f"features.{2 * i + 1}": outs[f"features.{2 * i + 1}"].contiguous() for i in self.return_indices}

    def _attention_operands(self, attn: ShiftedWindowAttention) -> Tuple[Tensor, Tensor]:
        """``(bias [heads, N, N], qkv bias [3 C])`` in fp32: the table expanded through the index buffer."""
        def build():
            with torch.no_grad():
                table = attn.position_bias().to(torch.float32).contiguous()
            return table, attn.qkv.bias.detach().to(torch.float32).contiguous()
        sources = (attn.relative_position_bias_table, attn.relative_position_index, attn.qkv.bias)
        return derived(attn, "swin_attention", sources, build)

    def build_plan(self, x: Tensor, splits: int = 0, train: Optional[dict] = None):
        """The op list of one forward on ``x`` ``[B, 3, H, W]`` (fp32 NCHW on the device): ``(ops, outputs, keep, names)``:
        ``outputs`` the returned fp32 NCHW maps, ``keep`` every tensor the plan points into, ``names`` one label per op.
        In inference the buffers of a stage are shared by its blocks (the launches of a plan run in order on one stream).
        ``train`` (a dict with ``"first"``, the index in ``_sequence()`` of the lowest module whose backward will run): a
        training forward; every module from there on gets buffers of its own, and ``train`` receives ``"acts"`` (what the
        backward reads, by name, see ``saved_activations``) and ``"factors"`` (the stochastic-depth factors ``[B]`` of
        every branch that drew some, by ``<block>.attn`` / ``<block>.mlp``)."""
        act = self.compute_dtype if self._precision() == 1 else torch.float32
        batch = x.shape[0]
        pb = PlanBuilder(_hip.SwinOpStruct, x, batch=batch, height=1, width=1, kernel_size=1, stride=1, splits=splits)
        new, op, keep, outputs = pb.new, pb.op, pb.keep, pb.outputs
        acts: Dict[str, Tensor] = {}
        factors: Dict[str, Tensor] = {}
        if train is not None:
            train["acts"], train["factors"] = acts, factors
        index = 0   # of the current module in _sequence()

        def gemm(name, kind, layer, src, out, h, w, layout=0, residual=None, nchw=None, aux=None, row_scale=None):
            packed, bias = self._packed(layer, layout)
            keep.extend((packed, bias))
            k = layer.kernel_size[0] if isinstance(layer, nn.Conv2d) else 1
            op(name, kind, x=src.data_ptr(), weight=packed.data_ptr(), bias=bias.data_ptr(), residual=_hip.ptr(residual),
               out=out.data_ptr(), out_nchw=_hip.ptr(nchw), in_channels=layer.weight.shape[1], height=h, width=w,
               out_channels=bias.numel(), kernel_size=k, stride=k, x_nchw=layout, aux=_hip.ptr(aux),
               row_scale=_hip.ptr(row_scale))

        def layer_norm(name, norm, src, out, h, w, c, out_f32=False):
            pb.layer_norm(name, 3, self._affine(norm), norm.eps, src, out, h, w, c, out_f32)

        stem = self.body.features[0]
        patch, c = stem[0].kernel_size[0], stem[0].out_channels
        h, w = x.shape[2] // patch, x.shape[3] // patch
        if h < 1 or w < 1:
            raise RuntimeError(f"SwinBackbone: a {x.shape[2]} x {x.shape[3]} input is smaller than one patch")
        raw = new((batch, h, w, c), torch.float32)
        gemm("0.features.0.0", 0, stem[0], x, raw, x.shape[2], x.shape[3], layout=1)
        stream = new((batch, h, w, c), torch.float32)
        layer_norm("0.features.0.2", stem[2], raw, stream, h, w, c, out_f32=True)
        for i, blocks, merging in self._stages():
            rows = (batch, h, w)
            hidden = blocks[0].mlp[0].out_features
            a_in = new(rows + (c,), act)                    # LayerNorm output: a GEMM A operand
            qkv = new(rows + (3 * c,), act)
            a_att = new(rows + (c,), act)
            mid = new(rows + (hidden,), act)
            for j, blk in enumerate(blocks):
                prefix = f"0.features.{2 * i + 1}.{j}"
                at = blk.attn
                stored = train is not None and train["first"] is not None and index >= train["first"]
                if stored:   # buffers of the block's own: the backward reads them
                    a1, a2, qkv_b, att_b = new(rows + (c,), act), new(rows + (c,), act), new(rows + (3 * c,), act), new(rows + (c,), act)
                    pre, mid_b = new(rows + (hidden,), act), new(rows + (hidden,), act)
                    x_in, x_mid, x_out = stream, new(rows + (c,), torch.float32), new(rows + (c,), torch.float32)
                else:
                    a1 = a2 = a_in
                    qkv_b, att_b, pre, mid_b = qkv, a_att, None, mid
                    x_in = x_mid = x_out = stream
                sd = blk.stochastic_depth   # two draws per block: the attention branch first, then the MLP branch
                f_attn, f_mlp = pb.draw(sd, batch, train is not None), pb.draw(sd, batch, train is not None)
                if f_attn is not None:
                    factors[prefix + ".attn"], factors[prefix + ".mlp"] = f_attn.view(batch), f_mlp.view(batch)
                layer_norm(prefix + ".norm1", blk.norm1, x_in, a1, h, w, c)
                gemm(prefix + ".attn.qkv", 2, at.qkv, a1, qkv_b, h, w)
                table, qkv_bias = self._attention_operands(at)
                keep.extend((table, qkv_bias))
                op(prefix + ".attn", 4, x=qkv_b.data_ptr(), bias=qkv_bias.data_ptr(), table=table.data_ptr(), out=att_b.data_ptr(),
                   in_channels=c, height=h, width=w, out_channels=c, window=at.window_size[0], shift=at.shift_size[0],
                   heads=at.num_heads)
                gemm(prefix + ".attn.proj", 0, at.proj, att_b, x_mid, h, w, residual=x_in, row_scale=f_attn)
                layer_norm(prefix + ".norm2", blk.norm2, x_mid, a2, h, w, c)
                gemm(prefix + ".mlp.0", 1, blk.mlp[0], a2, mid_b, h, w, aux=pre)
                nchw = None
                if j == len(blocks) - 1 and i in self.return_indices:
                    nchw = outputs[f"features.{2 * i + 1}"] = new((batch, c, h, w), torch.float32)
                gemm(prefix + ".mlp.3", 0, blk.mlp[3], mid_b, x_out, h, w, residual=x_mid, nchw=nchw, row_scale=f_mlp)
                if stored:
                    acts.update({prefix + ".in": x_in, prefix + ".norm1": a1, prefix + ".attn.qkv": qkv_b, prefix + ".attn": att_b,
                                 prefix + ".mid": x_mid, prefix + ".norm2": a2, prefix + ".mlp.0": pre, prefix + ".mlp.1": mid_b})
                stream = x_out
                index += 1
            if merging is not None:
                prefix = f"0.features.{2 * i + 2}"
                ho, wo = (h + 1) // 2, (w + 1) // 2
                gathered = new((batch, ho, wo, 4 * c), act)
                gamma, beta = self._affine(merging.norm)
                keep.extend((gamma, beta))
                op(prefix + ".norm", 5, x=stream.data_ptr(), gamma=gamma.data_ptr(), beta=beta.data_ptr(),
                   out=gathered.data_ptr(), in_channels=c, height=h, width=w, out_channels=4 * c, eps=float(merging.norm.eps))
                if train is not None and train["first"] is not None and index >= train["first"]:
                    acts.update({prefix + ".in": stream, prefix + ".norm": gathered})
                stream = new((batch, ho, wo, 2 * c), torch.float32)
                gemm(prefix + ".reduction", 0, merging.reduction, gathered, stream, ho, wo)
                h, w, c = ho, wo, 2 * c
                index += 1
        outputs = {f"features.{2 * i + 1}": outputs[f"features.{2 * i + 1}"] for i in self.return_indices}
        return pb.ops, outputs, keep, pb.names

    def forward_hip(self, x: Tensor, splits: int = 0, state: Optional[dict] = None) -> Dict[str, Tensor]:
        """``state`` (a dict): a training forward; it receives ``"first"``, ``"acts"`` and ``"factors"``, see
        ``build_plan``."""
        x = self._check_image(x)
        if not self.hip_form():
            raise RuntimeError("SwinBackbone: this configuration has no HIP form (window 7 / 12, head dimension 32)")
        if state is not None:
            state["first"] = self._first_trainable()
        ops, outputs, keep, _ = self.build_plan(x, splits, state)
        self._run_plan(_hip.SwinOpStruct, "sdetr_swin", ops, x.device)
        return outputs

    # ------------------------------------------------------------------------------------------ training in HIP
    # (the interface is HipBackbone's: the node keeps the activations the backward reads; its backward is one
    # ``sdetr_swin_bwd_run`` call over ``_backward_ops`` and returns the fp32 parameter gradients)
    train_reasons = ("the architecture is not one the HIP kernels serve (a window other than 7 / 12, a head dimension other "
                     "than 32, a width that is no multiple of 32, a norm other than nn.LayerNorm)",
                     "the stem (patch embedding and its LayerNorm, features.0) is trainable and has no HIP backward: freeze "
                     "it with freeze_indices")
    backward_struct, backward_prefix = _hip.SwinBwdOpStruct, "sdetr_swin_bwd"

    def _stem_modules(self):
        return (self.body.features[0],)

    def _extra_train_reason(self) -> Optional[str]:
        for _, blocks, _ in self._stages():
            for blk in blocks:
                drops = [blk.attn.attention_dropout, blk.attn.dropout] + [m.p for m in blk.mlp if isinstance(m, nn.Dropout)]
                if any(p != 0.0 for p in drops):
                    return "dropout / attention_dropout other than 0 is not served (the reference trains with 0)"
        return None

    def _output_name(self, i: int) -> str:
        return f"features.{2 * i + 1}"

    def _sequence(self) -> List[Tuple[str, str, nn.Module]]:
        """``(kind, name, module)`` of every block (``"block"``) and merging layer (``"merge"``) in forward order."""
        seq = []
        for i, blocks, merging in self._stages():
            seq.extend(("block", f"0.features.{2 * i + 1}.{j}", blk) for j, blk in enumerate(blocks))
            if merging is not None:
                seq.append(("merge", f"0.features.{2 * i + 2}", merging))
        return seq

    # ``saved_activations()`` (HipBackbone's test hook) holds, by name, of a block: ``<block>.in`` and ``.mid`` (the fp32
    # stream at its input and after the attention branch), ``.norm1`` / ``.norm2`` (the LayerNorm outputs), ``.attn.qkv``
    # (the qkv rows), ``.attn`` (the attention rows), ``.mlp.0`` (before the GELU), ``.mlp.1`` (after it); of a merging
    # layer ``<merging>.in`` (the stream it reads) and ``.norm`` (the gathered LayerNorm rows).
    # ``stochastic_depth_factors()`` is ``{<block>.attn | <block>.mlp: factors [B]}``, in forward order (the attention
    # branch, then the MLP branch).

    def _table_pairs(self, attn: ShiftedWindowAttention) -> Tuple[Tensor, Tensor]:
        """The (query, key) pairs of every table entry as a CSR list: ``(order int32 [N * N], offsets int32 [entries + 1])``."""
        def build():
            index = attn.relative_position_index.detach().reshape(-1).to(torch.int64)
            entries = attn.relative_position_bias_table.shape[0]
            order = torch.argsort(index, stable=True).to(torch.int32).contiguous()
            counts = torch.bincount(index, minlength=entries)
            offsets = torch.zeros(entries + 1, dtype=torch.int64, device=index.device)
            offsets[1:] = torch.cumsum(counts, 0)
            return order, offsets.to(torch.int32).contiguous()
        return derived(attn, "swin_table_pairs", (attn.relative_position_index, attn.relative_position_bias_table), build)

    def _backward_ops(self, acts: Dict[str, Tensor], factors: Dict[str, Tensor], shape, cotangents: Dict[str, Optional[Tensor]],
                      splits: int = 0):
        """The backward of one forward as ``(ops, names, grads, keep)``: ``ops`` the ``sdetr_swin_bwd_op`` list in run order,
        ``names`` one label per op, ``grads`` ``{parameter name: fp32 gradient}`` (as views of what the ops write), ``keep``
        every tensor the ops point into.  Walks ``_sequence()`` from the top down to the lowest trainable module."""
        batch, _, height, width = shape
        seq, first = self._sequence(), self._first_trainable()
        act = torch.float32 if self._precision() == 0 else self.compute_dtype
        pb = BackwardPlanBuilder(self.backward_struct, next(iter(acts.values())), batch=batch, splits=splits)
        keep, tmp, want, grad = pb.keep, pb.tmp, pb.want, pb.grad

        # the size and width of every module's input
        patch = self.body.features[0][0].kernel_size[0]
        sizes, h, w, c = [], height // patch, width // patch, self.body.features[0][0].out_channels
        for kind, _, _ in seq:
            sizes.append((h, w, c))
            if kind == "merge":
                h, w, c = (h + 1) // 2, (w + 1) // 2, 2 * c
        last_of = {f"0.features.{2 * i + 1}.{len(blocks) - 1}": i for i, blocks, _ in self._stages()}
        merge_of = {f"0.features.{2 * i + 2}": i for i, _, merging in self._stages() if merging is not None}

        dy = None
        for idx in range(len(seq) - 1, (first if first is not None else len(seq)) - 1, -1):
            kind, name, m = seq[idx]
            h, w, c = sizes[idx]
            below = idx > first
            if kind == "merge":
                stage = merge_of[name]
                ho, wo = (h + 1) // 2, (w + 1) // 2
                dzr = tmp("dzr", (batch, ho, wo, 2 * c), act)
                pb.rows(name + ".reduction", dy, None, dzr, None, 2 * c, ho, wo)
                dgath = tmp("dgath", (batch, ho, wo, 4 * c), act)
                if want(m.reduction.weight):
                    pb.wgrad(name + ".reduction", dzr, acts[name + ".norm"], 4 * c, 2 * c, ho, wo)
                pb.dgrad(name + ".reduction", self._packed_rows_dgrad(m.reduction), dzr, dgath, 4 * c, 2 * c, ho, wo)
                add = None
                if stage in self.return_indices:   # kind 5: the NCHW ingest
                    add = pb.ingest(name, 5, cotangents.get(f"features.{2 * stage + 1}"), None, c, h, w)
                dy = pb.next_dy((batch, h, w, c))   # kind 8: the LayerNorm backward scattered back over the 2 x 2 gather
                pb.layer_norm_bwd(name + ".norm", m.norm, self._f32(m.norm, "weight", m.norm.weight), 8, " (merging)", dz=dgath,
                                  x=acts[name + ".in"], add=add, out=dy, channels=c, height=h, width=w)
                continue
            stage = last_of.get(name)
            if stage is not None and stage in self.return_indices and f"0.features.{2 * stage + 2}" not in merge_of:
                dy = pb.ingest(name, 5, cotangents.get(f"features.{2 * stage + 1}"), dy, c, h, w)
            at, fc1, fc2 = m.attn, m.mlp[0], m.mlp[3]
            hidden = fc1.out_features
            # the MLP branch
            dzs = tmp("dzs", (batch, h, w, c), act)
            pb.rows(name + ".mlp.3", dy, factors.get(name + ".mlp"), dzs, grad(name + ".mlp.3.bias", (c,), fc2.bias), c, h, w)
            dh = tmp("dh", (batch, h, w, hidden), act)
            if want(fc2.weight):
                pb.wgrad(name + ".mlp.3", dzs, acts[name + ".mlp.1"], hidden, c, h, w)
            pb.dgrad(name + ".mlp.3", self._packed_rows_dgrad(fc2), dzs, dh, hidden, c, h, w)
            pb.gelu(name + ".mlp.1", dh, acts[name + ".mlp.0"], grad(name + ".mlp.0.bias", (hidden,), fc1.bias), hidden, h, w)
            dn = tmp("dn", (batch, h, w, c), act)
            if want(fc1.weight):
                pb.wgrad(name + ".mlp.0", dh, acts[name + ".norm2"], c, hidden, h, w)
            pb.dgrad(name + ".mlp.0", self._packed_rows_dgrad(fc1), dh, dn, c, hidden, h, w)
            dmid = tmp("dmid", (batch, h, w, c), torch.float32)
            pb.layer_norm_bwd(name + ".norm2", m.norm2, self._f32(m.norm2, "weight", m.norm2.weight), dz=dn, x=acts[name + ".mid"],
                              add=dy, out=dmid, channels=c, height=h, width=w)
            # the attention branch
            pb.rows(name + ".attn.proj", dmid, factors.get(name + ".attn"), dzs, grad(name + ".attn.proj.bias", (c,), at.proj.bias),
                    c, h, w)
            datt = tmp("datt", (batch, h, w, c), act)
            if want(at.proj.weight):
                pb.wgrad(name + ".attn.proj", dzs, acts[name + ".attn"], c, c, h, w)
            pb.dgrad(name + ".attn.proj", self._packed_rows_dgrad(at.proj), dzs, datt, c, c, h, w)
            table, qkv_bias = self._attention_operands(at)
            order, offsets = self._table_pairs(at)
            keep.extend((table, qkv_bias, order, offsets))
            dqkv, dpad = tmp("dqkv", (batch, h, w, 3 * c), act), tmp("dpad", (3 * c,), torch.float32)
            dtable = grad(name + ".attn.relative_position_bias_table", tuple(at.relative_position_bias_table.shape),
                          at.relative_position_bias_table)
            pb.op(name + ".attn (attention)", 6, x=acts[name + ".attn.qkv"].data_ptr(), dz=datt.data_ptr(), bias=qkv_bias.data_ptr(),
                  table=table.data_ptr(), order=order.data_ptr(), offsets=offsets.data_ptr(), out=dqkv.data_ptr(),
                  dbias=dpad.data_ptr(), dtable=_hip.ptr(dtable), channels=c, height=h, width=w, window=at.window_size[0],
                  shift=at.shift_size[0], heads=at.num_heads)
            dbq = grad(name + ".attn.qkv.bias", (3 * c,), at.qkv.bias)
            if dbq is not None:   # kind 7: the column sums of dqkv plus the padding tokens' share
                pb.op(name + ".attn.qkv (bias)", 7, dz=dqkv.data_ptr(), add=dpad.data_ptr(), dbias=dbq.data_ptr(), channels=3 * c,
                      height=h, width=w)
            if want(at.qkv.weight):
                pb.wgrad(name + ".attn.qkv", dqkv, acts[name + ".norm1"], c, 3 * c, h, w)
            pb.dgrad(name + ".attn.qkv", self._packed_rows_dgrad(at.qkv), dqkv, dn, c, 3 * c, h, w)
            # (the lowest block still needs norm1's dgamma / dbeta; its input gradient lands in a buffer nobody reads)
            dx = pb.next_dy((batch, h, w, c))
            pb.layer_norm_bwd(name + ".norm1", m.norm1, self._f32(m.norm1, "weight", m.norm1.weight), dz=dn, x=acts[name + ".in"],
                              add=dmid, out=dx, channels=c, height=h, width=w)
            dy = dx if below else None
        return pb.ops, pb.names, pb.grads, keep
