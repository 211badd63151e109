"""Dense self-attention over a few hundred rows for the training step, one launch forward and two backward
(``csrc/attention_train.hip``): the core of the encoder layer's ``nn.MultiheadAttention`` over its top-300 rows
(models/bricks/salience_transformer.py:371-376) between the in- and the out-projection.

``attention_qk_v(qk, v, num_heads)``: ``qk`` [B,N,2E] = the q and k projections of a row side by side (one GEMM over the
``q = k`` input), ``v`` [B,N,E] the value projection; returns the heads' outputs concatenated [B,N,E].  fp32 HIP tensors
with 32-channel heads and at most ``sdetr_attention_train_max_rows()`` rows; ``applies`` says when.

``attention_qk_v_masked(qk, v, num_heads, attn_mask=None)`` (``csrc/attention_train_masked.hip``): the same operands at any
row count, keys walked in LDS tiles, with an optional ``torch.bool`` [N,N] mask (True = may not attend) read as it lies --
the decoder layer's self-attention over its matching + denoising queries (salience_transformer.py:566-573);
``applies_masked`` says when.
"""
import math
from typing import Optional

import torch
from torch import Tensor
from torch.autograd import Function

from . import _hip


def applies(qk: Tensor, v: Tensor, num_heads: int) -> bool:
    return (qk.is_cuda and qk.dtype == torch.float32 and v.dtype == torch.float32 and qk.dim() == 3 and v.dim() == 3
            and qk.shape[-1] == 2 * v.shape[-1] and v.shape[-1] == 32 * num_heads and qk.shape[:2] == v.shape[:2]
            and 0 < qk.shape[1] <= _hip.lib().sdetr_attention_train_max_rows())


class _AttentionQKV(Function):
    @staticmethod
    def forward(ctx, qk, v, num_heads):
        qk, v = qk.contiguous(), v.contiguous()
        B, N, E = v.shape
        out = torch.empty_like(v)
        lse = torch.empty((B, num_heads, N), dtype=torch.float32, device=v.device)
        scale = 1.0 / math.sqrt(E // num_heads)
        _hip.launch("sdetr_attention_train_forward_f32", None, v.device, qk.data_ptr(), N * 2 * E, 2 * E,
                    qk.data_ptr() + 4 * E, N * 2 * E, 2 * E, v.data_ptr(), N * E, E, B, num_heads, N, E // num_heads,
                    scale, out.data_ptr(), lse.data_ptr(), what="attention_train_forward")
        ctx.save_for_backward(qk, v, out, lse)
        ctx.num_heads = num_heads
        return out

    @staticmethod
    def backward(ctx, grad_out):
        qk, v, out, lse = ctx.saved_tensors
        B, N, E = v.shape
        H = ctx.num_heads
        go = grad_out.contiguous()
        gqk, gv = torch.empty_like(qk), torch.empty_like(v)
        _hip.launch("sdetr_attention_train_backward_f32", None, v.device, qk.data_ptr(), N * 2 * E, 2 * E,
                    qk.data_ptr() + 4 * E, N * 2 * E, 2 * E, v.data_ptr(), N * E, E, B, H, N, E // H,
                    1.0 / math.sqrt(E // H), out.data_ptr(), lse.data_ptr(), go.data_ptr(), gqk.data_ptr(),
                    gqk.data_ptr() + 4 * E, gv.data_ptr(), what="attention_train_backward")
        return gqk, gv, None


def attention_qk_v(qk: Tensor, v: Tensor, num_heads: int) -> Tensor:
    return _AttentionQKV.apply(qk, v, num_heads)


# ---- any row count, optional boolean mask (csrc/attention_train_masked.hip): the decoder layer's self-attention --------
def applies_masked(qk: Tensor, v: Tensor, num_heads: int, attn_mask: Optional[Tensor] = None) -> bool:
    """``attention_qk_v_masked`` takes these operands: fp32 HIP ``qk`` [B,N,2E] / ``v`` [B,N,E] with 32-channel heads,
    N > 0 (no row limit), and ``attn_mask`` None or a ``torch.bool`` [N,N] tensor (True = may not attend) on the same
    device.  A float (additive) mask, a per-head 3-d mask, CPU tensors and 16-bit dtypes are not served."""
    if not (qk.is_cuda and qk.dtype == torch.float32 and v.dtype == torch.float32 and qk.dim() == 3 and v.dim() == 3
            and v.device == qk.device and qk.shape[-1] == 2 * v.shape[-1] and v.shape[-1] == 32 * num_heads
            and qk.shape[:2] == v.shape[:2] and qk.shape[1] > 0):
        return False
    N = qk.shape[1]
    return attn_mask is None or (attn_mask.dtype == torch.bool and tuple(attn_mask.shape) == (N, N)
                                 and attn_mask.device == qk.device)


class _AttentionQKVMasked(Function):
    @staticmethod
    def forward(ctx, qk, v, num_heads, attn_mask):
        qk, v = qk.contiguous(), v.contiguous()
        B, N, E = v.shape
        mask = None if attn_mask is None else attn_mask.contiguous()      # torch.bool storage, read as bytes
        out = torch.empty_like(v)
        lse = torch.empty((B, num_heads, N), dtype=torch.float32, device=v.device)
        scale = 1.0 / math.sqrt(E // num_heads)
        _hip.launch("sdetr_attention_train_masked_forward_f32", None, v.device, qk.data_ptr(), N * 2 * E, 2 * E,
                    qk.data_ptr() + 4 * E, N * 2 * E, 2 * E, v.data_ptr(), N * E, E, B, num_heads, N, E // num_heads,
                    scale, _hip.ptr(mask), N, out.data_ptr(), lse.data_ptr(), what="attention_train_masked_forward")
        ctx.save_for_backward(qk, v, out, lse, mask)
        ctx.num_heads = num_heads
        return out

    @staticmethod
    def backward(ctx, grad_out):
        qk, v, out, lse, mask = ctx.saved_tensors
        B, N, E = v.shape
        H = ctx.num_heads
        go = grad_out.contiguous()
        gqk, gv = torch.empty_like(qk), torch.empty_like(v)
        _hip.launch("sdetr_attention_train_masked_backward_f32", None, v.device, qk.data_ptr(), N * 2 * E, 2 * E,
                    qk.data_ptr() + 4 * E, N * 2 * E, 2 * E, v.data_ptr(), N * E, E, B, H, N, E // H,
                    1.0 / math.sqrt(E // H), _hip.ptr(mask), N, out.data_ptr(), lse.data_ptr(), go.data_ptr(),
                    gqk.data_ptr(), gqk.data_ptr() + 4 * E, gv.data_ptr(), what="attention_train_masked_backward")
        return gqk, gv, None, None


def attention_qk_v_masked(qk: Tensor, v: Tensor, num_heads: int, attn_mask: Optional[Tensor] = None) -> Tensor:
    """``attention_qk_v`` at any row count under ``attn_mask`` (``applies_masked`` says when): a masked pair is skipped;
    a fully masked row -- NaN in torch -- gives an output row of 0 and no gradient."""
    return _AttentionQKVMasked.apply(qk, v, num_heads, attn_mask)
