"""Sine position embedding and per-level padding masks (reference ``models/bricks/position_encoding.py:9-67`` and
``models/detectors/salience_detr.py:172-176``), on the HIP kernel ``sdetr_frontend_masks_positions``.

``PositionEmbeddingSine`` has the reference's constructor and ``dim_tx`` / ``dim_ty`` buffers; the kernel reads those
buffers (a device ``pow`` differs from the host's in the last bits, which the high-frequency phases amplify).  It keeps
the reference's fp32 order: ``(cumsum + offset) / (last + eps) * scale``, a true division by ``dim_t``, then ``sin`` of
the even and ``cos`` of the odd features; channels are (y features, x features).

``level_masks_and_positions`` returns every level's nearest-down-sampled mask
(``F.interpolate(mask[None].float(), size).to(bool)[0]``) and its position map in ONE launch, for any mask (not only
top-left rectangles).  There is no CPU fallback.
"""
import ctypes
import math
from typing import List, Sequence, Tuple, Union

import torch
from torch import Tensor, nn

from . import _hip


class PositionEmbeddingSine(nn.Module):
    def __init__(self, num_pos_feats=64, temperature: Union[int, Tuple[int, int]] = 10000, normalize=False,
                 scale=2 * math.pi, eps=1e-6, offset=0.0):
        super().__init__()
        dim_t = 2 * torch.arange(num_pos_feats).div(2, rounding_mode="floor") / num_pos_feats
        if isinstance(temperature, int):
            dim_tx = dim_ty = temperature**dim_t
        else:
            assert len(temperature) == 2, "Only support two elements as (t_x, t_y) in temperature"
            dim_tx, dim_ty = [t**dim_t for t in temperature]
        self.register_buffer("dim_tx", dim_tx)
        self.register_buffer("dim_ty", dim_ty)
        self.num_pos_feats = num_pos_feats
        self.normalize = normalize
        self.scale = scale
        self.eps = eps
        self.offset = offset

    def set_dtype(self, dtype: torch.dtype):
        """Positions are fp32 in every mode (the transformer reads them as such); kept for a uniform interface."""
        return self

    def forward(self, mask: Tensor) -> Tensor:
        """``mask`` ``[B, H, W]`` (True / nonzero on padding) -> ``[B, 2F, H, W]`` fp32."""
        _, pos = level_masks_and_positions(mask, [tuple(mask.shape[-2:])], self)
        return pos[0]


def level_masks_and_positions(mask: Tensor, level_shapes: Sequence[Tuple[int, int]],
                              position_embedding: PositionEmbeddingSine) -> Tuple[List[Tensor], List[Tensor]]:
    """Per-level masks ``[B, H_l, W_l]`` bool and positions ``[B, 2F, H_l, W_l]`` fp32 of the padded image mask
    ``[B, H, W]``, all levels in one launch."""
    pe = position_embedding
    if mask.dim() != 3:
        raise RuntimeError(f"level_masks_and_positions: mask must be [B, H, W], got {tuple(mask.shape)}")
    if not mask.is_cuda:
        raise RuntimeError("level_masks_and_positions: mask must be a HIP (cuda) tensor; the hot path has no CPU fallback")
    src = mask.to(torch.bool).contiguous().view(torch.uint8)
    dty = pe.dim_ty.to(device=mask.device, dtype=torch.float32).contiguous()
    dtx = pe.dim_tx.to(device=mask.device, dtype=torch.float32).contiguous()
    _hip.require_device("level_masks_and_positions", dim_ty=dty, dim_tx=dtx)
    B, H, W = src.shape
    shapes = [(int(h), int(w)) for h, w in level_shapes]
    n, F_ = len(shapes), pe.num_pos_feats
    masks = [torch.empty(B, h, w, dtype=torch.bool, device=mask.device) for h, w in shapes]
    pos = [torch.empty(B, 2 * F_, h, w, dtype=torch.float32, device=mask.device) for h, w in shapes]
    hw = (ctypes.c_int * (2 * n))(*[v for s in shapes for v in s])
    mptr = (ctypes.c_void_p * n)(*[m.data_ptr() for m in masks])
    pptr = (ctypes.c_void_p * n)(*[p.data_ptr() for p in pos])
    _hip.launch("sdetr_frontend_masks_positions", None, src.device, src.data_ptr(), B, H, W, n, hw, dty.data_ptr(),
                dtx.data_ptr(), F_, int(bool(pe.normalize)), float(pe.scale), float(pe.eps), float(pe.offset), mptr,
                pptr, what="level_masks_and_positions")
    return masks, pos
