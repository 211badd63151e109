"""Pyramid plumbing that feeds the filtering stage and the two position
embeddings the hot path needs.  Device-side torch glue only; no arithmetic kernels live here.

Reference: ``models/bricks/base_transformer.py:22-56, 74-112`` and
``models/bricks/position_encoding.py:10-99``.
"""
from typing import List, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor, nn

from .derived import derived


def flatten_multi_level(multi_level_elements: Sequence[Tensor]) -> Tensor:
    """``[B,(C),H_l,W_l]`` per level -> token-major ``[B,S,(C)]`` (base_transformer.py:22-27)."""
    flat = torch.cat([e.flatten(-2) for e in multi_level_elements], -1)
    if flat.ndim == 3:
        flat = flat.transpose(1, 2).contiguous()
    return flat


class _LevelPosEmbed(torch.autograd.Function):
    """``cat_l(flatten(pos_l) + level_embeds[l])`` with the level embeddings' gradient as column sums of the token-major
    gradient: one sum over the batch, then one per level over its rows -- the broadcast add's own backward reduces each
    level's ``[B, hw, C]`` slice in up to three kernels (0.34 ms of the training step)."""

    @staticmethod
    def forward(ctx, level_embeds, *pos):
        ctx.sizes = [int(p.shape[-2]) * int(p.shape[-1]) for p in pos]
        return torch.cat([p.flatten(-2).transpose(1, 2) + level_embeds[l] for l, p in enumerate(pos)], 1)

    @staticmethod
    def backward(ctx, grad):
        out, cur = [], 0
        if grad.is_cuda and grad.dtype == torch.float32 and grad.stride(2) == 1 and grad.shape[2] % 4 == 0:
            # The device's own column-sum kernel (fixed-order tree, no atomics, no scratch): the framework's multi-block
            # reduction clears its semaphores with a hipMemsetAsync, which a REPLAYED hipGraph does not reproduce on this
            # stack (ROCm 7.2 / torch 2.10) -- the training step's replays then summed stale partial results (this
            # gradient came out 10x too large; found by comparing the replayed step's gradients with the eager step's).
            from .filter_ops import column_mean
            for n in ctx.sizes:
                per_image = column_mean(grad[:, cur:cur + n]) * float(n)      # [B, 1, C]
                out.append(per_image.sum(0)[0] if grad.shape[0] > 1 else per_image[0, 0])
                cur += n
            return (torch.stack(out),) + (None,) * len(ctx.sizes)
        g = grad.sum(0) if grad.shape[0] > 1 else grad[0]          # [S, C]
        for n in ctx.sizes:
            out.append(g[cur:cur + n].sum(0))
            cur += n
        return (torch.stack(out),) + (None,) * len(ctx.sizes)


def get_lvl_pos_embed(level_embeds: Tensor, multi_level_pos_embeds: Sequence[Tensor]) -> Tensor:
    """pos + level embedding, flattened (base_transformer.py:29-33).  The level embedding is added in the token-major
    layout (the same sums as the reference's NCHW add)."""
    if level_embeds.requires_grad and torch.is_grad_enabled() and not any(p.requires_grad for p in multi_level_pos_embeds):
        return _LevelPosEmbed.apply(level_embeds, *multi_level_pos_embeds)
    return torch.cat([p.flatten(-2).transpose(1, 2) + level_embeds[l] for l, p in enumerate(multi_level_pos_embeds)], 1)


def get_valid_ratios(mask: Tensor) -> Tensor:
    """(w, h) valid fraction read off row 0 / column 0 (base_transformer.py:48-56)."""
    _, h, w = mask.shape
    valid_h = torch.sum(~mask[:, :, 0], 1)
    valid_w = torch.sum(~mask[:, 0, :], 1)
    return torch.stack([valid_w.float() / w, valid_h.float() / h], -1)


# Small tensors whose content only depends on the pyramid geometry (spatial shapes, level starts,
# pixel-centre grids, host-computed budgets).  They originate on the host; caching them per
# (geometry, device) removes the per-forward H2D copies, which also keeps the forward capturable
# in a hipGraph (no host-memory copies inside the captured region).
_STATIC = {}          # insertion-ordered: least recently used first
_STATIC_LIMIT = 1024


def static_tensor(key, build):
    """Cached device constants (shape tensors, reference grids, token budgets).  Eviction is least-recently-used, one
    entry at a time: a captured hipGraph has the addresses of the tensors it was warmed up with baked in, so a
    wholesale clear() -- which hands all of them back to the caching allocator at once -- would let a later replay read
    recycled memory.  Entries in use by a live graph are the recently used ones; only a process that streams through
    more than `_STATIC_LIMIT` distinct (image size, canvas) combinations evicts, oldest first."""
    t = _STATIC.pop(key, None)
    if t is None:
        while len(_STATIC) >= _STATIC_LIMIT:
            _STATIC.pop(next(iter(_STATIC)))
        t = build()
    _STATIC[key] = t        # (re)insert as most recently used
    return t


def shape_tensors(level_shapes: Sequence[Tuple[int, int]], device) -> Tuple[Tensor, Tensor]:
    """spatial_shapes [L,2] / level_start_index [L], int64, on ``device`` (cached per geometry)."""
    def build():
        shapes = torch.as_tensor([tuple(s) for s in level_shapes], dtype=torch.int64)
        sizes = shapes.prod(1)
        lsi = torch.cat((sizes.new_zeros((1,)), sizes.cumsum(0)[:-1]))
        return shapes.to(device), lsi.to(device)
    return static_tensor(("shapes", tuple(map(tuple, level_shapes)), str(device)), build)


def multi_level_misc(multi_level_masks: Sequence[Tensor]) -> Tuple[Tensor, Tensor, Tensor]:
    """spatial_shapes [L,2] int64, level_start_index [L] int64 (both on the masks' device, as the
    reference op reads them from device memory) and valid_ratios [B,L,2] (base_transformer.py:35-46)."""
    shapes, lsi = shape_tensors(level_shapes_of(multi_level_masks), multi_level_masks[0].device)
    valid_ratios = torch.stack([get_valid_ratios(m) for m in multi_level_masks], 1)
    return shapes, lsi, valid_ratios


def level_shapes_of(multi_level_masks: Sequence[Tensor]) -> List[Tuple[int, int]]:
    return [tuple(int(s) for s in m.shape[-2:]) for m in multi_level_masks]


def encoder_output_memory(enc_output: nn.Linear, enc_output_norm: nn.LayerNorm, memory: Tensor,
                          memory_padding_mask: Tensor, level_shapes: Sequence[Tuple[int, int]]) -> Tensor:
    """First return value of ``gen_encoder_output_proposals`` (base_transformer.py:74-112): tokens that
    are padding, or whose proposal box (cx, cy, w, h) leaves (0.01, 0.99), are zeroed before
    ``LayerNorm(Linear(.))``.  The proposal geometry only depends on the masks, so the keep-mask is
    built with a handful of small ops and no host sync."""
    n = memory.shape[0]
    keep = []
    cur = 0
    for lvl, (h, w) in enumerate(level_shapes):
        m = memory_padding_mask[:, cur:cur + h * w].view(n, h, w)
        valid_h = torch.sum(~m[:, :, 0], 1).view(n, 1, 1).float()
        valid_w = torch.sum(~m[:, 0, :], 1).view(n, 1, 1).float()
        cy = (torch.arange(h, dtype=torch.float32, device=memory.device).view(1, h, 1) + 0.5) / valid_h
        cx = (torch.arange(w, dtype=torch.float32, device=memory.device).view(1, 1, w) + 0.5) / valid_w
        wh = 0.05 * 2.0 ** lvl
        ok = (cx > 0.01) & (cx < 0.99) & (cy > 0.01) & (cy < 0.99)
        if not (0.01 < wh < 0.99):
            ok = torch.zeros_like(ok)
        keep.append(ok.expand(n, h, w).reshape(n, h * w))
        cur += h * w
    keep = torch.cat(keep, 1) & ~memory_padding_mask
    from .layer_norm_train import add_layer_norm   # (one launch each way for fp32 HIP tensors, nn.LayerNorm otherwise)
    return add_layer_norm(enc_output(memory * keep.unsqueeze(-1).to(memory.dtype)), enc_output_norm)


class PositionEmbeddingLearned(nn.Module):
    """Learned row/column embedding (position_encoding.py:70-99); used as the encoder's background
    embedding.  ``flat(level_shapes)`` returns the batch-independent ``[S, 2*num_pos_feats]`` table."""

    def __init__(self, num_embeddings: int = 50, num_pos_feats: int = 256):
        super().__init__()
        self.row_embed = nn.Embedding(num_embeddings, num_pos_feats)
        self.col_embed = nn.Embedding(num_embeddings, num_pos_feats)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.uniform_(self.row_embed.weight)
        nn.init.uniform_(self.col_embed.weight)

    def level_table(self, h: int, w: int) -> Tensor:
        if h > self.row_embed.num_embeddings or w > self.col_embed.num_embeddings:
            raise IndexError(f"feature map {h}x{w} exceeds max_num_embedding={self.row_embed.num_embeddings}")
        x_emb = self.col_embed.weight[:w]
        y_emb = self.row_embed.weight[:h]
        return torch.cat([x_emb.unsqueeze(0).expand(h, w, -1), y_emb.unsqueeze(1).expand(h, w, -1)], dim=-1)

    def flat(self, level_shapes: Sequence[Tuple[int, int]]) -> Tensor:
        return torch.cat([self.level_table(h, w).reshape(h * w, -1) for h, w in level_shapes], 0)

    def flat_cached(self, level_shapes: Sequence[Tuple[int, int]], dtype: torch.dtype) -> Tensor:
        """``flat(level_shapes).to(dtype)`` detached, rebuilt only when the embeddings (or the request) change --
        for the no-grad path, where it is a constant of the weights."""
        def build():
            with torch.no_grad():
                return self.flat(level_shapes).to(dtype).contiguous()
        return derived(self, "flat", (self.row_embed.weight, self.col_embed.weight), build,
                       extra=(tuple(map(tuple, level_shapes)), dtype))

    def forward(self, mask: Tensor) -> Tensor:
        h, w = mask.shape[-2:]
        return self.level_table(h, w).permute(2, 0, 1).unsqueeze(0).repeat(mask.shape[0], 1, 1, 1)


# ------------------------------------------------------------------------------------------------
# host-side token budgets (no device sync): the data-dependent sizes of the filtering stage
# ------------------------------------------------------------------------------------------------
def _nearest_valid_extent(valid: int, size_in: int, size_out: int) -> int:
    """Number of output rows/cols of F.interpolate(mode='nearest') that map to a valid input index
    (< ``valid``); same float32 index arithmetic as ATen (src = floor(dst * in/out))."""
    scale = np.float32(size_in) / np.float32(size_out)
    src = np.minimum(np.floor(np.arange(size_out, dtype=np.float32) * scale).astype(np.int64), size_in - 1)
    return int((src < valid).sum())


def host_token_budgets(image_sizes: Sequence[Tuple[int, int]], canvas: Tuple[int, int],
                       level_shapes: Sequence[Tuple[int, int]], level_filter_ratio: Sequence[float]):
    """``focus_token_nums`` [B], ``level_token_nums`` [L] and valid tokens [B,L] computed on the HOST from
    the image sizes, reproducing salience_transformer.py:116-121 including the float32 product that is
    truncated by ``.int()``.  Lets a caller that knows its image sizes (the detector does) run the
    filtering stage without any device->host synchronisation."""
    ratio = np.asarray(level_filter_ratio, dtype=np.float32)
    valid = np.zeros((len(image_sizes), len(level_shapes)), dtype=np.int64)
    for b, (h, w) in enumerate(image_sizes):
        for l, (hl, wl) in enumerate(level_shapes):
            valid[b, l] = _nearest_valid_extent(h, canvas[0], hl) * _nearest_valid_extent(w, canvas[1], wl)
    focus = (valid.astype(np.float32) * ratio[None]).astype(np.int32)  # trunc toward zero like .int()
    return focus.sum(-1).astype(np.int64), focus.max(0).astype(np.int64), valid


def layer_token_counts(num_inds: int, layer_filter_ratio: Sequence[float]) -> List[int]:
    """``(num_inds * layer_filter_ratio).to(int64)`` in float32 (salience_transformer.py:161-165)."""
    r = np.asarray(layer_filter_ratio, dtype=np.float32)
    return [int(v) for v in (np.float32(num_inds) * r).astype(np.int64)]
