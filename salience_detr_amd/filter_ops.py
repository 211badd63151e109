"""Host wrappers of the filtering / row-movement kernels (C ABI sections (4) and (5) of
include/salience_hip.h).  PyTorch only owns the memory and the stream."""
import ctypes
import math
from typing import Optional

import torch
from torch import Tensor

from . import _hip
from .derived import derived


def masked_topk_desc(score: Tensor, k: int, mask: Optional[Tensor] = None, fill_with_global_min: bool = False,
                     payload: Optional[Tensor] = None, index_offset: int = 0, want_scores: bool = True,
                     fill_value: Optional[Tensor] = None, out=None, orders_job: Optional["RowOrdersJob"] = None,
                     carry_rank: Optional["RankJob"] = None, carry_finalize: Optional["FinalizeJob"] = None):
    """Sorted-descending top-k per row with ties -> lower index first.

    ``score`` [B,N] fp32.  With ``mask`` (bool [B,N], True = masked) and ``fill_with_global_min`` the
    masked entries compete with the value ``score.min()`` taken over the WHOLE array, as the reference
    does with ``masked_fill(mask, score.min())`` before ``topk`` (salience_transformer.py:146-150).
    Returns ``(values [B,k] or None, indices [B,k] int64)``; ``indices`` are ``payload[b, pos]`` when a
    payload is given (the index gather after the global sort, :156-158), else ``pos + index_offset``.
    ``fill_value`` (one-element fp32 device tensor) supplies ``score.min()`` when the caller already has it;
    ``mask`` may be a column slice of a wider ``[B,S]`` mask.  ``out = (scores, indices)``: column slices
    ``[B,k]`` of wider buffers to write into (same row stride), instead of fresh tensors.  ``carry_rank`` /
    ``carry_finalize``: a pending ``RankJob`` / ``FinalizeJob`` that the call's merge launch takes along when it has one
    with room (the sliced form); they are marked ``done`` then, and left pending otherwise.
    """
    _hip.require_device("masked_topk_desc", score=score, payload=payload, fill_value=fill_value)
    if score.dtype != torch.float32 or score.dim() != 2:
        raise RuntimeError("masked_topk_desc: score must be a 2-d float32 tensor")
    B, N = score.shape
    k = int(k)
    if k < 0 or k > N:
        # torch.topk: "selected index k out of range"
        raise RuntimeError(f"masked_topk_desc: selected index k out of range (k={k}, row length {N})")
    if mask is not None and not fill_with_global_min:
        raise RuntimeError("masked_topk_desc: a mask requires fill_with_global_min=True")
    if mask is None and payload is None and out is None and N > _SELECT_MAX_ROW and 0 < k <= 2048 and k * 16 <= N:
        return _sliced_topk(score, k, int(index_offset), want_scores, orders_job)
    if (((N > _PREFILTER_MAX_ROW and k * 16 > N) or (N >= _SLICED_MIN_ROW and k * 5 > N)) and payload is None
            and orders_job is None and score.is_contiguous()
            and (mask is None or (fill_with_global_min and fill_value is not None))):
        return _sorted_slices_topk(score, k, mask, fill_value, int(index_offset), want_scores, out, carry_rank,
                                   carry_finalize)
    mask_stride = 0
    if mask is not None:
        if mask.shape != score.shape or not mask.is_cuda:
            raise RuntimeError("masked_topk_desc: mask shape / device mismatch")
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        if N > 1 and mask.stride(1) != 1:
            mask = mask.contiguous()
        mask_stride = mask.stride(0) if B > 1 else N
    if payload is not None and (payload.dtype != torch.int64 or payload.shape != score.shape):
        raise RuntimeError("masked_topk_desc: payload must be int64 with score's shape")
    out_stride = 0
    if out is not None:
        out_score, out_index = out
        if (tuple(out_index.shape) != (B, k) or out_index.dtype != torch.int64 or not out_index.is_cuda
                or (k > 1 and out_index.stride(1) != 1)
                or (out_score is not None and (tuple(out_score.shape) != (B, k) or out_score.dtype != torch.float32
                                               or out_score.stride() != out_index.stride()))):
            raise RuntimeError("masked_topk_desc: out must be ([B,k] fp32 | None, [B,k] int64) column slices of equal stride")
        out_stride = out_index.stride(0) if B > 1 else k
    else:
        out_score = torch.empty((B, k), dtype=torch.float32, device=score.device) if want_scores else None
        out_index = torch.empty((B, k), dtype=torch.int64, device=score.device)
    ws_bytes = _hip.lib().sdetr_topk_workspace_bytes(B, N, k)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=score.device) if ws_bytes else None
    args = (score.data_ptr(), _hip.ptr(mask), mask_stride,
            (2 if fill_value is not None else 1) if fill_with_global_min else 0, _hip.ptr(fill_value),
            _hip.ptr(payload), B, N, k, int(index_offset), _hip.ptr(out_score), out_index.data_ptr(), out_stride,
            _hip.ptr(ws), ws_bytes)
    if orders_job is not None and not orders_job.done and orders_job.device == score.device:
        # the encoder's row orders ride in this launch (or run right behind it when it is not the one-launch sort)
        _hip.launch("sdetr_masked_topk_desc_with_orders_f32", None, score.device, *args, ctypes.byref(orders_job.struct),
                    what="masked_topk_desc")
        orders_job.done = True
    else:
        _hip.launch("sdetr_masked_topk_desc_f32", None, score.device, *args, what="masked_topk_desc")
    return out_score, out_index


_SELECT_MAX_ROW = 17408      # longest row of the one-launch histogram sort (csrc/topk.hip kHsMaxN)
_SLICE = 8192


def _sliced_topk(score: Tensor, k: int, index_offset: int, want_scores: bool, orders_job):
    """Top-k (k small) of rows longer than the one-workgroup histogram sort takes, in launches of it (round 5): every
    8192-key slice of a row keeps its own sorted top-k (a workgroup per slice), then the ``slices x k`` survivors are
    sorted once more with their row positions as payload -- and, when the survivors themselves are longer than one
    workgroup's row (very long rows: ADVICE r5), they are sliced again first.  The rows' global top-k are among their
    slices' top-k; ties stay in position order (slices are concatenated in row order and each is sorted
    ties-by-position, so equal scores keep ascending positions in every candidate list -- the last sort's positional rule
    is the row's).  This is the per-layer top-300 of the reference's 5scale pyramid (salience_transformer.py:366-367 on
    45 330 rows, BASELINE configs[3]): the chip-wide rank by counting it replaces is quadratic in the row -- 80-170 us
    per layer there."""
    from . import pyramid
    B = score.shape[0]
    vals, pos = score, None                     # candidate scores and their positions in the row (None: identity)
    while vals.shape[1] > _SELECT_MAX_ROW:
        n = vals.shape[1]
        S = -(-n // _SLICE)
        pad = S * _SLICE - n
        sp = torch.nn.functional.pad(vals, (0, pad), value=float("-inf")) if pad else vals
        v1, i1 = masked_topk_desc(sp.reshape(B * S, _SLICE), k)
        base = pyramid.static_tensor(("topk_slice_base", S, str(score.device)),
                                     lambda: (torch.arange(S, dtype=torch.int64) * _SLICE).view(1, S, 1).to(score.device))
        at = (i1.view(B, S, k) + base).view(B, S * k)           # positions in `vals` (padding never survives: k <= n)
        if pad:
            at = at.clamp_(max=n - 1)                           # (-inf padding tied with real -inf scores)
        pos = at if pos is None else torch.gather(pos, 1, at)
        vals = v1.view(B, S * k)
    v2, i2 = masked_topk_desc(vals, k, payload=pos, want_scores=want_scores, orders_job=orders_job)
    if index_offset:
        i2 = i2 + index_offset
    return v2, i2


_PREFILTER_MAX_ROW = 24576   # longest row the sampled-threshold prefilter takes (csrc/topk.hip use_prefilter)
_SLICED_MIN_ROW = 8192       # rows from here on with k > N / 5 take the two chip-wide launches of the sliced form
_MERGE_SEGMENTS = 8          # csrc/topk.hip kMaxSegments


def _sorted_slices_topk(score: Tensor, k: int, mask: Optional[Tensor], fill_value: Optional[Tensor], index_offset: int,
                        want_scores: bool, out, carry_rank: Optional["RankJob"] = None,
                        carry_finalize: Optional["FinalizeJob"] = None):
    """Top-k with k a sizeable fraction of a LONG row -- the finest level of a pyramid (salience_transformer.py:146-150):
    6680 of 16 800 scores at 800 x 1333 (rounds 1-5: one histogram-sort workgroup per image, 36 us on two workgroups),
    16 700 of 67 200 on the reference's 5scale pyramid (beyond every single-workgroup form; the chip-wide rank by
    counting is quadratic in the row, ~380 us there).  ``sdetr_masked_topk_sliced_f32``: the row is cut into eight slices,
    every slice is sorted completely by the rank kernel (1/8 of the comparisons, all slices of all images in one
    launch), and the sorted slices are merged (stable in slice order, i.e. ties stay in position order); the first k are
    written straight into ``out``.  Masked entries compete with ``fill_value`` exactly as in the one-launch forms (the
    caller supplies the whole array's minimum: a per-slice minimum would be a different number)."""
    B, N = score.shape
    mask_stride = 0
    if mask is not None:
        if mask.shape != score.shape or not mask.is_cuda:
            raise RuntimeError("masked_topk_desc: mask shape / device mismatch")
        mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        if N > 1 and mask.stride(1) != 1:
            mask = mask.contiguous()
        mask_stride = mask.stride(0) if B > 1 else N
    if out is not None:
        out_score, out_index = out
        if (tuple(out_index.shape) != (B, k) or out_index.dtype != torch.int64 or not out_index.is_cuda
                or (k > 1 and out_index.stride(1) != 1)
                or (out_score is not None and (tuple(out_score.shape) != (B, k) or out_score.dtype != torch.float32
                                               or out_score.stride() != out_index.stride()))):
            raise RuntimeError("masked_topk_desc: out must be ([B,k] fp32 | None, [B,k] int64) column slices of equal stride")
        out_stride = out_index.stride(0) if B > 1 else k
    else:
        out_score = torch.empty((B, k), dtype=torch.float32, device=score.device) if want_scores else None
        out_index = torch.empty((B, k), dtype=torch.int64, device=score.device)
        out_stride = k
    ws_bytes = _hip.lib().sdetr_topk_sliced_workspace_bytes(B, N)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=score.device)
    job = carry_rank if carry_rank is not None and not carry_rank.done and carry_rank.score.device == score.device else None
    fin = (carry_finalize if carry_finalize is not None and not carry_finalize.done
           and carry_finalize.tokens.device == score.device else None)
    act = fin.tokens.dtype if fin is not None else None      # (the pass works on 16-bit activations: it picks the library)
    carried = ctypes.c_int(0)
    _hip.launch("sdetr_masked_topk_sliced_with_rank_f32", act, score.device, score.data_ptr(), _hip.ptr(mask),
                mask_stride, _hip.ptr(fill_value) if mask is not None else None, B, N, k, _MERGE_SEGMENTS,
                int(index_offset), _hip.ptr(out_score), out_index.data_ptr(), out_stride, ws.data_ptr(), ws_bytes,
                ctypes.byref(job.struct()) if job is not None else None,
                ctypes.byref(fin.struct()) if fin is not None else None, ctypes.byref(carried),
                what="masked_topk_desc (sliced)")
    if carried.value:
        if job is not None:
            job.done = True
        if fin is not None:
            fin.done = True
    return out_score, out_index


class RankJob:
    """A plain masked top-k (``masked_topk_desc`` with a given ``fill_value``, no payload, a row short enough that no
    prefilter is involved) that has not been launched yet: ``salience_head(..., rank_job=job)`` carries it in its
    stage-1 launch, ``job.run()`` launches it on its own.  The outputs are the ``out`` slices it was planned with."""

    def __init__(self, score, k, mask, fill_value, index_offset, out):
        self.score, self.k, self.mask, self.fill_value, self.index_offset, self.out = score, int(k), mask, fill_value, index_offset, out
        self.done = False

    def struct(self):
        B, N = self.score.shape
        mask = self.mask
        if mask is not None:
            mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        out_score, out_index = self.out
        st = _hip.RankJobStruct()
        st.score = self.score.data_ptr()
        st.mask = _hip.ptr(mask)
        st.mask_row_stride = (mask.stride(0) if B > 1 else N) if mask is not None else 0
        st.fill_value = _hip.ptr(self.fill_value)
        st.batch, st.n, st.k = B, N, self.k
        st.index_offset = int(self.index_offset)
        st.out_score = _hip.ptr(out_score)
        st.out_index = out_index.data_ptr()
        st.out_row_stride = out_index.stride(0) if B > 1 else self.k
        self._keep = (mask, st)
        return st

    def run(self):
        if self.done:
            return
        masked_topk_desc(self.score, self.k, mask=self.mask, fill_with_global_min=self.mask is not None,
                         index_offset=self.index_offset, fill_value=self.fill_value, out=self.out)
        self.done = True


def plan_masked_topk(score: Tensor, k: int, mask: Optional[Tensor], fill_value: Tensor, index_offset: int, out):
    """``masked_topk_desc(score, k, mask, True, index_offset=..., fill_value=..., out=out)`` as a pending ``RankJob`` when
    the launch would be the rank kernel alone (no prefilter, a contiguous fp32 ``score`` with a contiguous-row mask);
    otherwise runs it now and returns ``None``."""
    B, N = score.shape
    plain = (score.is_cuda and score.dtype == torch.float32 and score.is_contiguous() and 0 < int(k) <= N
             and fill_value is not None and not _hip.lib().sdetr_topk_uses_prefilter(N, int(k))
             and (mask is None or (mask.shape == score.shape and (N == 1 or mask.stride(1) == 1))))
    if not plain:
        masked_topk_desc(score, k, mask=mask, fill_with_global_min=mask is not None, index_offset=index_offset,
                         fill_value=fill_value, out=out)
        return None
    return RankJob(score, k, mask, fill_value, index_offset, out)


def gather_rows(src: Tensor, idx: Tensor) -> Tensor:
    """``dst[b, i] = src[b, idx[b, i]]`` for ``src`` [B,S,C], ``idx`` [B,n] int64
    (the torch.gather calls of salience_transformer.py:454-461 without the expanded index)."""
    _hip.require_device("gather_rows", idx=idx)
    if idx.dtype != torch.int64 or src.dim() < 2 or idx.dim() != 2 or idx.shape[0] != src.shape[0]:
        raise RuntimeError("gather_rows: src [B,S,...], idx [B,n] int64 expected")
    B, S = src.shape[:2]
    n = idx.shape[1]
    row_elems = src[0, 0].numel() if S > 0 else 0
    row_bytes = row_elems * src.element_size()
    if not src.is_cuda:
        raise RuntimeError("gather_rows: src must be a HIP (cuda) tensor; the hot path has no CPU fallback")
    if S > 0 and not src[0].is_contiguous():
        raise RuntimeError("gather_rows: src rows have to be contiguous")
    if B > 1 and S > 0 and row_elems > 0:
        # a row prefix [B, :S] of a longer [B, S', ...] buffer is fine: images are S' rows apart
        if src.stride(0) % row_elems or src.stride(0) < S * row_elems:
            raise RuntimeError("gather_rows: src tensor has to be contiguous (or a row prefix of one)")
        S = src.stride(0) // row_elems
    dst = torch.empty((B, n) + tuple(src.shape[2:]), dtype=src.dtype, device=src.device)
    if B * n == 0:
        return dst
    _hip.launch("sdetr_gather_rows", None, src.device, src.data_ptr(), idx.data_ptr(), B, S, n, row_bytes,
                dst.data_ptr())
    return dst


def scatter_rows_(dst: Tensor, idx: Tensor, src: Tensor, count: Optional[Tensor] = None) -> Tensor:
    """In place ``dst[b, idx[b, i]] = src[b, i]`` for ``i < count[b]`` (all rows when ``count`` is None):
    the per-image scatter of salience_transformer.py:474-485 with ``focus_token_nums`` read on-device."""
    _hip.require_device("scatter_rows_", dst=dst, idx=idx, src=src, count=count)
    if idx.dtype != torch.int64 or dst.dtype != src.dtype or idx.shape[0] != dst.shape[0]:
        raise RuntimeError("scatter_rows_: dst [B,S,...], idx [B,n] int64, src [B,n,...] expected")
    if count is not None and (count.dtype != torch.int64 or count.numel() != dst.shape[0]):
        raise RuntimeError("scatter_rows_: count must be int64 [B]")
    B, S = dst.shape[:2]
    n = idx.shape[1]
    if B * n == 0:
        return dst
    row_bytes = dst[0, 0].numel() * dst.element_size()
    _hip.launch("sdetr_scatter_rows", None, dst.device, dst.data_ptr(), idx.data_ptr(), src.data_ptr(), _hip.ptr(count),
                B, S, n, row_bytes, what="scatter_rows_")
    return dst


flatten_one_launch = True     # F0 as one launch for the whole pyramid (False: one per level; same bits)


def pyramid_flatten(multi_level_feats, multi_level_pos_embeds, multi_level_masks, level_embeds: Tensor,
                    want_bf16: bool = False, want_fp32: bool = True, one_launch: Optional[bool] = None):
    """F0 in one launch (``one_launch=False``: one per level, same bits): ``flatten_multi_level`` + ``get_lvl_pos_embed``
    (base_transformer.py:22-33) + the token validity of ``gen_encoder_output_proposals`` (:74-112).

    Returns ``(feat_flatten [B,S,C], lvl_pos_embed_flatten [B,S,C], enc_output_input [B,S,C] =
    (feat + pos) * keep, mask_flatten [B,S] bool, feat_bf16 | None, pos_bf16 | None, valid_ratios [B,L,2])``;
    ``valid_ratios`` is ``get_valid_ratios`` of every level (base_transformer.py:48-56), a by-product of the
    extents the kernel counts anyway.  ``want_fp32=False`` skips the fp32 feat / pos outputs (``None`` is returned
    for them): the bf16 encoder only reads the bf16 copies.
    """
    feats = [f.contiguous() for f in multi_level_feats]
    pos = [p.contiguous() for p in multi_level_pos_embeds]
    masks = [m.contiguous() for m in multi_level_masks]
    _hip.require_device("pyramid_flatten", level_embeds=level_embeds, **{f"feat{i}": f for i, f in enumerate(feats)})
    if feats[0].dtype != torch.float32 or pos[0].dtype != torch.float32:
        raise RuntimeError("pyramid_flatten: float32 feature / position maps expected")
    B, C = feats[0].shape[:2]
    S = sum(int(f.shape[2]) * int(f.shape[3]) for f in feats)
    dev = feats[0].device
    feat_out = torch.empty((B, S, C), dtype=torch.float32, device=dev) if want_fp32 else None
    pos_out = torch.empty((B, S, C), dtype=torch.float32, device=dev) if want_fp32 else None
    sum_out = torch.empty((B, S, C), dtype=torch.float32, device=dev)
    mask_out = torch.empty((B, S), dtype=torch.bool, device=dev)
    # (``want_bf16``: True = bfloat16 copies; a 16-bit dtype = copies in that activation type, from that library's kernel)
    act = None if not want_bf16 else (torch.bfloat16 if want_bf16 is True else want_bf16)
    if act is not None and not _hip.is_act16(act):
        raise RuntimeError("pyramid_flatten: 16-bit copies are bfloat16 or float16")
    feat_bf16 = torch.empty((B, S, C), dtype=act, device=dev) if want_bf16 else None
    pos_bf16 = torch.empty((B, S, C), dtype=act, device=dev) if want_bf16 else None
    le = level_embeds.detach().float().contiguous()
    valid_ratios = torch.empty((B, len(feats), 2), dtype=torch.float32, device=dev)
    start = 0
    L = len(feats)
    if (flatten_one_launch if one_launch is None else one_launch) and L <= 8:
        mu8s = [m.view(torch.uint8) if m.dtype == torch.bool else m for m in masks]
        ptrs = lambda ts: (ctypes.c_void_p * L)(*[t.data_ptr() for t in ts])
        ints = lambda vs: (ctypes.c_int * L)(*vs)
        _hip.launch("sdetr_pyramid_flatten", act, dev, L, ptrs(feats), ptrs(pos), ptrs(mu8s),
                    ints([int(f.shape[2]) for f in feats]), ints([int(f.shape[3]) for f in feats]), le.data_ptr(), B, C,
                    S, _hip.ptr(feat_out), _hip.ptr(pos_out), sum_out.data_ptr(), mask_out.data_ptr(),
                    _hip.ptr(feat_bf16), _hip.ptr(pos_bf16), valid_ratios.data_ptr())
        return feat_out, pos_out, sum_out, mask_out, feat_bf16, pos_bf16, valid_ratios
    for lvl, (f, p, m) in enumerate(zip(feats, pos, masks)):
        H, W = int(f.shape[2]), int(f.shape[3])
        mu8 = m.view(torch.uint8) if m.dtype == torch.bool else m
        _hip.launch("sdetr_pyramid_flatten_level", act, dev, f.data_ptr(), p.data_ptr(), mu8.data_ptr(), le[lvl].data_ptr(),
                    B, C, H, W, lvl, start, S, _hip.ptr(feat_out), _hip.ptr(pos_out), sum_out.data_ptr(),
                    mask_out.data_ptr(), _hip.ptr(feat_bf16), _hip.ptr(pos_bf16), valid_ratios.data_ptr() + lvl * 8,
                    len(feats) * 2)
        start += H * W
    return feat_out, pos_out, sum_out, mask_out, feat_bf16, pos_bf16, valid_ratios


def class_max_times(score: Tensor, scale: Tensor) -> Tensor:
    """``score.max(-1)[0] * scale`` in one pass: score ``[B,Nq,num_classes]`` (fp32 | bf16), scale ``[B,Nq]``
    fp32 (may be a row prefix of a longer ``[B,n]`` buffer) -> fp32 ``[B,Nq]`` (mc_score of
    salience_transformer.py:366)."""
    _hip.require_device("class_max_times", score=score)
    if not scale.is_cuda:
        raise RuntimeError("class_max_times: scale must be a HIP (cuda) tensor; the hot path has no CPU fallback")
    B, Nq, C = score.shape
    if scale.dtype != torch.float32 or scale.dim() != 2 or (Nq > 1 and scale.stride(1) != 1):
        scale = scale.float().contiguous()
    out = torch.empty((B, Nq), dtype=torch.float32, device=score.device)
    _hip.launch("sdetr_class_max_times", score.dtype, score.device, score.data_ptr(), _hip.dtype_code(score.dtype),
                scale.data_ptr(), scale.stride(0) if B > 1 else max(Nq, 1), B, Nq, C, out.data_ptr())
    return out


def _bn_view(t: Tensor):
    """(tensor viewed as [B, n, C] with a contiguous last dim, batch stride, row stride)."""
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3:
        t = t.reshape(-1, t.shape[-2], t.shape[-1])
    if t.stride(2) != 1:
        t = t.contiguous()
    return t, t.stride(0), t.stride(1)


def fused_layer_norm(x: Tensor, norm: torch.nn.LayerNorm, residual: Optional[Tensor] = None,
                     row_scale: Optional[Tensor] = None, alpha: Optional[Tensor] = None,
                     out_dtype: Optional[torch.dtype] = None, scatter_index: Optional[Tensor] = None,
                     scatter_into: Optional[Tensor] = None, gather_x: bool = False) -> Tensor:
    """``norm((x [+ residual]) * (1 + row_scale * alpha))`` in one launch (see include/salience_hip.h (6)).
    ``x`` may be a batch-strided view (e.g. one level's slice of ``[B,S,C]``); the result is contiguous.
    With ``scatter_index`` [B,n] int64 and ``scatter_into`` [B,m,C] (contiguous) row ``(b,i)`` of the result is
    written to ``scatter_into[b, scatter_index[b,i]]`` instead (in place; returns ``scatter_into``).  ``gather_x``:
    ``x`` is a ``[B,m,C]`` buffer whose rows ``scatter_index[b,i]`` are the inputs (``x = scatter_into`` updates the
    selected rows in place: gather + residual + norm + scatter in one launch); ``residual`` stays ``[B,n,C]``."""
    if not x.is_cuda:
        raise RuntimeError("fused_layer_norm: HIP device tensors required; there is no CPU fallback")
    shape = x.shape
    xv, xbs, xrs = _bn_view(x)
    B, n, C = xv.shape
    if gather_x:
        if scatter_index is None or scatter_index.shape[0] != B:
            raise RuntimeError("fused_layer_norm: gather_x needs scatter_index [B,n]")
        n = scatter_index.shape[1]
    rv, rbs, rrs = (None, 0, 0)
    if residual is not None:
        if residual.dtype != x.dtype or tuple(residual.shape) != (B, n, C):
            raise RuntimeError("fused_layer_norm: residual must match the normalised rows")
        rv, rbs, rrs = _bn_view(residual)
    if row_scale is not None:
        row_scale = row_scale.reshape(-1)
        if row_scale.dtype != torch.float32 or row_scale.numel() != B * n or not row_scale.is_contiguous():
            row_scale = row_scale.float().contiguous()
    w, b = norm.weight.detach(), norm.bias.detach()
    out_rows = 0
    if scatter_index is not None:
        _hip.require_device("fused_layer_norm", scatter_index=scatter_index, scatter_into=scatter_into)
        if (scatter_index.dtype != torch.int64 or tuple(scatter_index.shape) != (B, n) or scatter_into.dim() != 3
                or scatter_into.shape[0] != B or scatter_into.shape[2] != C):
            raise RuntimeError("fused_layer_norm: scatter_index [B,n] int64 and scatter_into [B,m,C] expected")
        out, out_dtype, out_rows = scatter_into, scatter_into.dtype, scatter_into.shape[1]
    else:
        out_dtype = out_dtype or x.dtype
        out = torch.empty((B, n, C), dtype=out_dtype, device=x.device)
    _hip.launch("sdetr_layernorm", x.dtype if _hip.is_act16(x.dtype) else out_dtype, x.device, xv.data_ptr(),
                _hip.ptr(rv), _hip.dtype_code(x.dtype), xbs, xrs, rbs, rrs, _hip.ptr(row_scale), _hip.ptr(alpha),
                w.data_ptr(), b.data_ptr(), _hip.dtype_code(w.dtype), float(norm.eps), B, n, C, out.data_ptr(),
                _hip.dtype_code(out_dtype), _hip.ptr(scatter_index), out_rows, 1 if gather_x else 0,
                what="fused_layer_norm")
    return out if scatter_index is not None else out.view(shape)


def column_mean(x: Tensor) -> Tensor:
    """Mean over dim 1 of a ``[B,n,C]`` fp32 tensor (may be a strided column slice) -> ``[B,1,C]``."""
    if not x.is_cuda:
        raise RuntimeError("column_mean: HIP device tensors required; there is no CPU fallback")
    if x.dtype != torch.float32 or x.dim() != 3 or x.stride(2) != 1:
        raise RuntimeError("column_mean: fp32 [B,n,C] with a contiguous last dim expected")
    B, n, C = x.shape
    out = torch.empty((B, 1, C), dtype=torch.float32, device=x.device)
    _hip.launch("sdetr_column_mean_f32", None, x.device, x.data_ptr(), x.stride(0), x.stride(1), B, n, C,
                out.data_ptr(), what="column_mean")
    return out


# Stage 1 of the salience head on the bf16 matrix cores at fp32 accuracy (three-way exact split of both operands,
# six MFMAs per product; csrc/salience_head.hip).  False = the fp32-input MFMA kernel.
salience_head_bf16x3 = True
# With the hoisted head, stage 2 of a small level takes its per-image constant in its own blocks (no const launch); False =
# the const launch everywhere.  Up to 40 rows of partial sums (1280 tokens): same-box timelines of the 800 x 1333 step,
# per level modulation + const + stage 2 -- 273 tokens 48.4 -> 44.7 us, 1050 tokens 47.9 -> 44.2, 4200 tokens (132 rows, a
# chain of nine trips to memory in every block) 25.7 -> 27.8: that level keeps the launch.  (The kernel takes up to 160.)
CONST_IN_BLOCK = True
CONST_IN_BLOCK_ROWS = 40


def packed_linear_weight(weight: Tensor, cols=None, split3: bool = False) -> Tensor:
    """``weight[:, cols[0]:cols[1]]`` ([out, in] fp32 parameter) in the operand order of the salience-head kernels
    (``sdetr_pack_linear_f32``; ``split3``: the three bf16 planes of ``sdetr_pack_linear_bf16x3``).  The packed copy
    lives on the parameter object itself and is refreshed when the parameter's storage, device or version changes
    (optimizer step, ``load_state_dict``, ``.to()``)."""
    w = weight.detach()
    if not w.is_cuda or w.dtype != torch.float32 or w.dim() != 2 or w.stride(1) != 1:
        raise RuntimeError("packed_linear_weight: fp32 [out,in] HIP tensor with a contiguous last dim expected")
    if cols is not None:
        w = w[:, cols[0]:cols[1]]

    def build():
        out = torch.empty(w.shape[0] * w.shape[1] * (3 if split3 else 1), dtype=torch.bfloat16 if split3 else torch.float32,
                          device=w.device)
        _hip.launch("sdetr_pack_linear_bf16x3" if split3 else "sdetr_pack_linear_f32", None, w.device, w.data_ptr(),
                    w.stride(0), w.shape[0], w.shape[1], out.data_ptr(), what="pack_linear")
        return out
    return derived(weight, "packed_linear_x3" if split3 else "packed_linear", (weight,), build, extra=cols)


class ValueProjectionJob:
    """A slice (``groups`` consecutive layers) of a batched value projection (``value_proj_head_major``) that has not
    been launched yet: ``salience_head(..., value_job=job)`` carries it in its stage-1 launch (the coarse levels leave
    the chip nearly empty), ``job.run()`` launches it on its own.  Either way ``job.done`` is set."""

    def __init__(self, value, packed, bias, pad, heads, groups, dst, first_group, bordered=None):
        self.value, self.packed, self.bias, self.pad = value, packed, bias, pad
        self.heads, self.groups, self.dst, self.first_group = heads, groups, dst, first_group
        self.bordered = bordered      # (struct, its device tensors) of a bordered destination, or None
        self.done = False

    def pointers(self):
        """(x, packed weight, padded bias, pad mask, B, Nv, heads, groups, dst, dtype code, bordered layout | None) of
        the slice."""
        B, Nv, _ = self.value.shape
        tiles = self.first_group * self.heads        # 32-feature tiles in front of the slice (32 channels per head)
        d = self.dst[self.first_group]
        return (self.value.data_ptr(), self.packed.data_ptr() + tiles * 16384, self.bias.data_ptr() + tiles * 32 * 4,
                _hip.ptr(self.pad), B, Nv, self.heads, self.groups, d.data_ptr(), _hip.dtype_code(self.dst.dtype),
                None if self.bordered is None else ctypes.byref(self.bordered[0]))

    def run(self):
        if self.done:
            return
        x, pw, b, pad, B, Nv, heads, groups, dst, code_, lay = self.pointers()
        _hip.launch("sdetr_value_proj_head_major", self.value.dtype, self.value.device, x, pw, b, pad, B, Nv, 256,
                    heads, 32, groups, dst, code_, lay)
        self.done = True


def bordered_struct(level_shapes, device):
    """``(sdetr_bordered_layout, keep-alive tensors)`` of a pyramid's bordered map layout on ``device`` (cached)."""
    from .ms_deform_attn import bordered_layout
    lay = bordered_layout(level_shapes)
    key = "struct:" + str(device)
    hit = lay._dev.get(key)
    if hit is None:
        pix, border = lay.on(device)
        hit = (_hip.BorderedLayoutStruct(pix.data_ptr(), border.data_ptr(), int(border.numel()), int(lay.records)), pix, border)
        lay._dev[key] = hit
    return hit


def plan_value_projection(value: Tensor, weight: Tensor, bias: Optional[Tensor], padding_mask: Optional[Tensor],
                          num_heads: int, num_groups: int, dtype: torch.dtype, parts=2, bordered_levels=None):
    """``value_proj_head_major`` split into jobs over consecutive layer groups that share one destination
    ``[groups,B,heads,Nv,32]``: returns ``(dst, [ValueProjectionJob, ...])``.  ``parts``: a number of (nearly) equal
    parts, or a sequence of layer counts per job (they must add up to ``num_groups``).  ``bordered_levels``: the
    pyramid's level shapes -> the maps are written in the bordered layout ``[groups,B,heads,Np,32]``
    (``ms_deform_attn.BorderedLayout``; the jobs zero the borders themselves)."""
    if not token_linear_applies(value, weight) or weight.shape[0] != num_groups * num_heads * 32:
        raise RuntimeError("plan_value_projection: bf16 [B,Nv,256] tokens and 32-channel heads expected")
    _hip.require_device("plan_value_projection", value=value, padding_mask=padding_mask)
    B, Nv, _ = value.shape
    packed, b = _packed_linear_bf16(weight, bias)
    pad = None if padding_mask is None else (padding_mask.view(torch.uint8) if padding_mask.dtype == torch.bool
                                             else padding_mask)
    bordered = None
    records = Nv
    if bordered_levels is not None:
        bordered = bordered_struct(bordered_levels, value.device)
        records = bordered[0].records
        if sum(int(h) * int(w) for h, w in bordered_levels) != Nv:
            raise RuntimeError("plan_value_projection: the level shapes do not add up to the token count")
    dst = torch.empty((num_groups, B, num_heads, records, 32), dtype=dtype, device=value.device)
    if isinstance(parts, int):
        k = max(1, min(int(parts), num_groups))
        sizes = [(num_groups * (i + 1)) // k - (num_groups * i) // k for i in range(k)]
    else:
        sizes = [int(v) for v in parts]
        if sum(sizes) != num_groups or any(v < 0 for v in sizes):
            raise RuntimeError("plan_value_projection: the parts must add up to num_groups")
    jobs, g0 = [], 0
    for n in sizes:
        if n > 0:
            jobs.append(ValueProjectionJob(value, packed, b, pad, num_heads, n, dst, g0, bordered))
        g0 += n
    return dst, jobs


class HoistedHead:
    """``salience_head_hoist``'s result: ``g`` [B,S,256] and ``sigma`` [B,S] of all levels' tokens plus the constant row
    ``c0`` [256] -- ``salience_head(..., hoisted=h.level(start, n))`` then runs a level without its stage 1."""

    def __init__(self, g: Tensor, sigma: Tensor, c0: Tensor):
        self.g, self.sigma, self.c0 = g, sigma, c0

    def level(self, start: int, n: int) -> "HoistedHead":
        return HoistedHead(self.g[:, start:start + n], self.sigma[:, start:start + n], self.c0)


def _layer1_constant(predictor) -> Tensor:
    """``c0 = layer1.Linear.weight @ layer1.LayerNorm.bias + layer1.Linear.bias`` (fp32 [256]), cached on the weight and
    refreshed when any of the three parameters changes."""
    l1n, l1 = predictor.layer1[0], predictor.layer1[1]

    def build():
        with torch.no_grad():
            # (elementwise product + a sum per row: no library GEMV -- its accumulation order varies with the handle's state)
            return ((l1.weight.detach().double() * l1n.bias.detach().double()).sum(1)
                    + l1.bias.detach().double()).float().contiguous()
    return derived(l1.weight, "layer1_constant", (l1.weight, l1.bias, l1n.bias), build)


def salience_head_hoist(x: Tensor, predictor, enc_output=None, enc_output_norm=None, memory_out: Optional[Tensor] = None,
                        value_job: Optional[ValueProjectionJob] = None,
                        finalize_job: Optional["FinalizeJob"] = None) -> HoistedHead:
    """Everything of the salience head's stage 1 that does not depend on the coarser level's score, for ALL levels' tokens
    in one launch (include/salience_hip.h, sdetr_salience_head_hoist_x3): ``x`` [B,S,256] fp32 -> ``HoistedHead``.  With
    ``enc_output`` / ``enc_output_norm`` they are applied first (``memory_out`` [B,S,256] optionally receives their
    result).  ``value_job`` / ``finalize_job``: pending jobs the launch carries (the latter only next to no value job)."""
    if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 3 or x.stride(2) != 1 or x.shape[2] != 256:
        raise RuntimeError("salience_head_hoist: fp32 [B,S,256] HIP tensor with a contiguous last dim expected; no CPU fallback")
    B, S, C = x.shape
    job_act = value_job.value.dtype if value_job is not None else (finalize_job.tokens.dtype if finalize_job is not None else None)
    lib = _hip.lib(job_act)
    l1n, l1 = predictor.layer1[0], predictor.layer1[1]
    w_enc = b_enc = g_enc = be_enc = None
    eps_enc, mbs = 0.0, 0
    if enc_output is not None:
        w_enc = packed_linear_weight(enc_output.weight, split3=True)
        b_enc, g_enc, be_enc = enc_output.bias.detach(), enc_output_norm.weight.detach(), enc_output_norm.bias.detach()
        eps_enc = float(enc_output_norm.eps)
        if memory_out is not None:
            if memory_out.shape != x.shape or memory_out.stride(2) != 1 or memory_out.stride(1) != C:
                raise RuntimeError("salience_head_hoist: memory_out must be [B,S,C] with contiguous rows")
            mbs = memory_out.stride(0)
    g = torch.empty((B, S, C), dtype=torch.float32, device=x.device)
    sigma = torch.empty((B, S), dtype=torch.float32, device=x.device)
    c0 = _layer1_constant(predictor)
    carry_value = value_job is not None and not value_job.done and value_job.value.device == x.device
    carry_fin = (finalize_job is not None and not finalize_job.done and not carry_value
                 and finalize_job.tokens.device == x.device)
    vp = value_job.pointers() if carry_value else (None, None, None, None, 0, 0, 0, 0, None, 0, None)
    fj = ctypes.byref(finalize_job.struct()) if carry_fin else None
    _hip.launch("sdetr_salience_head_hoist_x3", lib, x.device, x.data_ptr(), x.stride(0), x.stride(1), B, S, C,
                _hip.ptr(w_enc), _hip.ptr(b_enc), _hip.ptr(g_enc), _hip.ptr(be_enc), eps_enc, l1n.weight.data_ptr(),
                packed_linear_weight(l1.weight, split3=True).data_ptr(), _hip.ptr(memory_out), mbs, g.data_ptr(),
                g.stride(0), sigma.data_ptr(), sigma.stride(0), *vp, fj, what="salience_head_hoist")
    if carry_value:
        value_job.done = True
    if carry_fin:
        finalize_job.done = True
    return HoistedHead(g, sigma, c0)


# The pyramid flatten inside the hoisted stage-1 launch (csrc/salience_head_core.h, PYR form) where nothing but that launch
# would read the flatten's fp32 ``enc_output`` input: 16-bit encoder, no fp32 / aux outputs wanted.  False = the flatten's
# own launch followed by ``salience_head_hoist`` (same bits; the reference of tests/test_stage1_flatten_fused_gpu.py).
FLATTEN_IN_STAGE1 = True
_PYR_TILE_LEVELS = 4     # levels that may meet inside one 32-token tile (csrc/salience_head_core.h kPyrTileLevels)


def hoist_pyramid_applies(multi_level_feats, multi_level_pos_embeds, multi_level_masks, predictor, enc_output, act) -> bool:
    """Does ``salience_head_hoist_pyramid`` take this pyramid?  fp32 NCHW maps with 256 channels on one HIP device, a 16-bit
    activation type, the fp32 256-wide head on the bf16x3 kernels, at most 8 levels of which at most 4 meet in a tile."""
    feats, L = list(multi_level_feats), len(multi_level_feats)
    if not (FLATTEN_IN_STAGE1 and salience_head_bf16x3 and _hip.is_act16(act) and 1 <= L <= 8):
        return False
    if any((not t.is_cuda) or t.dtype != torch.float32 or t.dim() != 4 or t.shape[1] != 256
           for t in feats + list(multi_level_pos_embeds)):
        return False
    if any(m.dtype not in (torch.bool, torch.uint8) for m in multi_level_masks):
        return False
    if not (getattr(predictor, "h_dim", 0) == 256 and predictor.layer1[1].weight.dtype == torch.float32
            and enc_output is not None and enc_output.weight.dtype == torch.float32 and enc_output.weight.is_cuda):
        return False
    starts = [0]
    for f in feats:
        starts.append(starts[-1] + int(f.shape[2]) * int(f.shape[3]))
    return all(starts[l + _PYR_TILE_LEVELS] // 32 != (starts[l + 1] - 1) // 32 for l in range(L - _PYR_TILE_LEVELS))


def salience_head_hoist_pyramid(multi_level_feats, multi_level_pos_embeds, multi_level_masks, level_embeds: Tensor, predictor,
                                enc_output, enc_output_norm, act: torch.dtype, memory_out: Optional[Tensor] = None):
    """``pyramid_flatten(want_bf16=act, want_fp32=False)`` and ``salience_head_hoist`` of its ``enc_output`` input in ONE launch
    (include/salience_hip.h, sdetr_salience_head_hoist_pyramid_x3): the stage-1 tiles read the fp32 NCHW maps themselves.
    Returns ``(HoistedHead, mask_flatten [B,S] bool, feat_act [B,S,256], pos_act [B,S,256], valid_ratios [B,L,2])`` -- the
    same bits as the two launches.  No job rides on this launch: the pending ones read ``feat_act``."""
    feats = [f.contiguous() for f in multi_level_feats]
    pos = [p.contiguous() for p in multi_level_pos_embeds]
    masks = [m.contiguous() for m in multi_level_masks]
    _hip.require_device("salience_head_hoist_pyramid", level_embeds=level_embeds, **{f"feat{i}": f for i, f in enumerate(feats)},
                        **{f"pos{i}": t for i, t in enumerate(pos)}, **{f"mask{i}": m for i, m in enumerate(masks)})
    if not hoist_pyramid_applies(feats, pos, masks, predictor, enc_output, act):
        raise RuntimeError("salience_head_hoist_pyramid: fp32 [B,256,H,W] maps, a 16-bit activation type and the fp32 256-wide "
                           "head on the bf16x3 kernels expected (at most 8 levels, at most 4 inside one 32-token tile)")
    L = len(feats)
    B, C = feats[0].shape[:2]
    for f, q, m in zip(feats, pos, masks):
        if q.shape != f.shape or tuple(m.shape) != (B, f.shape[2], f.shape[3]) or f.shape[:2] != (B, C):
            raise RuntimeError("salience_head_hoist_pyramid: feature / position / mask shapes of a level disagree")
    S = sum(int(f.shape[2]) * int(f.shape[3]) for f in feats)
    dev = feats[0].device
    mask_out = torch.empty((B, S), dtype=torch.bool, device=dev)
    feat_act = torch.empty((B, S, C), dtype=act, device=dev)
    pos_act = torch.empty((B, S, C), dtype=act, device=dev)
    valid_ratios = torch.empty((B, L, 2), dtype=torch.float32, device=dev)
    le = level_embeds.detach().float().contiguous()
    g = torch.empty((B, S, C), dtype=torch.float32, device=dev)
    sigma = torch.empty((B, S), dtype=torch.float32, device=dev)
    mbs = 0
    if memory_out is not None:
        if memory_out.shape != g.shape or memory_out.stride(2) != 1 or memory_out.stride(1) != C or memory_out.dtype != torch.float32:
            raise RuntimeError("salience_head_hoist_pyramid: memory_out must be fp32 [B,S,C] with contiguous rows")
        mbs = memory_out.stride(0)
    l1n, l1 = predictor.layer1[0], predictor.layer1[1]
    c0 = _layer1_constant(predictor)
    mu8s = [m.view(torch.uint8) if m.dtype == torch.bool else m for m in masks]
    ptrs = lambda ts: (ctypes.c_void_p * L)(*[t.data_ptr() for t in ts])
    ints = lambda vs: (ctypes.c_int * L)(*vs)
    lib = _hip.lib(act)
    _hip.launch("sdetr_salience_head_hoist_pyramid_x3", lib, dev, L, ptrs(feats), ptrs(pos), ptrs(mu8s),
                ints([int(f.shape[2]) for f in feats]), ints([int(f.shape[3]) for f in feats]), le.data_ptr(), B, C, S,
                mask_out.data_ptr(), feat_act.data_ptr(), pos_act.data_ptr(), valid_ratios.data_ptr(),
                packed_linear_weight(enc_output.weight, split3=True).data_ptr(), enc_output.bias.detach().data_ptr(),
                enc_output_norm.weight.detach().data_ptr(), enc_output_norm.bias.detach().data_ptr(),
                float(enc_output_norm.eps), l1n.weight.data_ptr(),
                packed_linear_weight(l1.weight, split3=True).data_ptr(), _hip.ptr(memory_out), mbs, g.data_ptr(),
                g.stride(0), sigma.data_ptr(), sigma.stride(0), what="salience_head_hoist_pyramid")
    return HoistedHead(g, sigma, c0), mask_out, feat_act, pos_act, valid_ratios


def salience_head(x: Tensor, predictor, row_scale: Optional[Tensor] = None, coarse_score: Optional[Tensor] = None,
                  level_hw=None, alpha: Optional[Tensor] = None, enc_output=None, enc_output_norm=None,
                  memory_out: Optional[Tensor] = None, score_flat: Optional[Tensor] = None,
                  score_min: Optional[Tensor] = None, value_job: Optional[ValueProjectionJob] = None,
                  value_job2: Optional[ValueProjectionJob] = None, rank_job: Optional["RankJob"] = None,
                  finalize_job: Optional["FinalizeJob"] = None, hoisted: Optional["HoistedHead"] = None) -> Tensor:
    """The salience head on one level in three launches (include/salience_hip.h (6)).

    ``x`` [B,n,256] fp32 (may be one level's slice of ``[B,S,256]``); ``predictor`` a ``MaskPredictor`` with
    ``in_dim == h_dim == 256``.  With ``enc_output`` / ``enc_output_norm`` (``nn.Linear`` / ``nn.LayerNorm``) they
    are applied first and ``memory_out`` (a ``[B,n,256]`` slice, optional) receives their result.  The
    coarse-to-fine modulation takes either ``row_scale`` [B,n] or the coarser level's ``coarse_score``
    [B,1,h',w'] (resized in-kernel to ``level_hw``), times the device scalar ``alpha``.  ``score_flat``
    (a ``[B,n]`` slice of the flattened score buffer) optionally receives a second copy; ``score_min`` (one-element
    fp32 tensor) the minimum over all ``B*n`` scores.  ``value_job``: a pending slice of the encoder's value projection
    that stage 1's launch carries along (bf16x3 kernel only; otherwise it is left pending), ``value_job2`` one for
    stage 2's launch; ``rank_job``: a pending top-k of the next coarser level, ``finalize_job``: the token-space
    pass of the encoder's output -- also for stage 1's launch (the latter only next to no value job).
    ``hoisted``: the level's rows of ``salience_head_hoist``'s result -- stage 1 then shrinks to the modulation step
    (``sdetr_salience_head_modulate``: ``x`` is only looked at for its shape, ``enc_output`` / ``memory_out`` have been
    dealt with by the hoisted launch, a ``value_job`` is left pending).
    Returns ``[B,n]``."""
    if not x.is_cuda:
        raise RuntimeError("salience_head: HIP device tensors required; there is no CPU fallback")
    if x.dtype != torch.float32 or x.dim() != 3 or x.stride(2) != 1:
        raise RuntimeError("salience_head: fp32 [B,n,C] with a contiguous last dim expected")
    B, n, C = x.shape
    # (the head itself is fp32 arithmetic, the same in both libraries; the jobs its launches carry work on 16-bit
    # activations: they pick the library)
    job_act = next((j.value.dtype for j in (value_job, value_job2) if j is not None), None)
    if job_act is None and finalize_job is not None:
        job_act = finalize_job.tokens.dtype
    lib = _hip.lib(job_act)
    l1n, l1 = predictor.layer1[0], predictor.layer1[1]
    l2a, l2b, l2c = predictor.layer2[0], predictor.layer2[2], predictor.layer2[4]
    half = predictor.h_dim // 2
    if row_scale is not None:
        row_scale = row_scale.reshape(B, n)
        if row_scale.dtype != torch.float32 or not row_scale.is_contiguous():
            row_scale = row_scale.float().contiguous()
    ch = cw = lh = lw = 0
    if coarse_score is not None:
        ch, cw = coarse_score.shape[-2:]
        lh, lw = level_hw
        _hip.require_device("salience_head", coarse_score=coarse_score)
    x3 = bool(salience_head_bf16x3)
    w_enc = b_enc = g_enc = be_enc = None
    eps_enc = 0.0
    mbs = 0
    if enc_output is not None:
        w_enc = packed_linear_weight(enc_output.weight, split3=x3)
        b_enc, g_enc, be_enc = enc_output.bias.detach(), enc_output_norm.weight.detach(), enc_output_norm.bias.detach()
        eps_enc = float(enc_output_norm.eps)
        if memory_out is not None:
            if memory_out.shape != x.shape or memory_out.stride(2) != 1 or memory_out.stride(1) != C:
                raise RuntimeError("salience_head: memory_out must be a [B,n,C] slice with contiguous rows")
            mbs = memory_out.stride(0)
    nblk = lib.sdetr_salience_head_blocks(B, n)
    z_local = torch.empty((B, n, half), dtype=torch.float32, device=x.device)
    partial = torch.empty((B, max(nblk, 1), half), dtype=torch.float32, device=x.device)
    cst = torch.empty((B, half), dtype=torch.float32, device=x.device)
    score = torch.empty((B, n), dtype=torch.float32, device=x.device)
    sfs = 0
    if score_flat is not None:
        if score_flat.shape != score.shape or score_flat.stride(1) != 1 or score_flat.dtype != torch.float32:
            raise RuntimeError("salience_head: score_flat must be a fp32 [B,n] slice with a contiguous last dim")
        sfs = score_flat.stride(0)
    dev = x.device
    stage1_args = (
        x.data_ptr(), x.stride(0), x.stride(1), B, n, C, _hip.ptr(w_enc), _hip.ptr(b_enc), _hip.ptr(g_enc),
        _hip.ptr(be_enc), eps_enc, _hip.ptr(row_scale), _hip.ptr(coarse_score), ch, cw, lh, lw, _hip.ptr(alpha),
        l1n.weight.data_ptr(), l1n.bias.data_ptr(), float(l1n.eps),
        packed_linear_weight(l1.weight, split3=x3).data_ptr(),
        l1.bias.data_ptr(), _hip.ptr(memory_out), mbs, z_local.data_ptr(), partial.data_ptr())
    # a coarse level of the hoisted head takes stage 2's per-image constant in stage 2's own blocks (no const launch)
    const_in_block = hoisted is not None and x3 and CONST_IN_BLOCK and nblk <= CONST_IN_BLOCK_ROWS
    if hoisted is not None:
        if hoisted.g.shape != x.shape or hoisted.g.stride(2) != 1 or hoisted.g.stride(1) != C or hoisted.sigma.stride(1) != 1:
            raise RuntimeError("salience_head: hoisted rows must be [B,n,256] / [B,n] slices with contiguous rows")
        value_job = None
    carry_value = x3 and value_job is not None and not value_job.done and value_job.value.device == dev
    carry_rank = x3 and rank_job is not None and not rank_job.done and rank_job.score.device == dev
    carry_fin = (x3 and finalize_job is not None and not finalize_job.done and not carry_value
                 and finalize_job.tokens.device == dev)
    rk = ctypes.byref(rank_job.struct()) if carry_rank else None
    fj = ctypes.byref(finalize_job.struct()) if carry_fin else None
    if hoisted is not None:
        _hip.launch("sdetr_salience_head_modulate", lib, dev, hoisted.g.data_ptr(), hoisted.g.stride(0),
                    hoisted.sigma.data_ptr(), hoisted.sigma.stride(0), B, n, _hip.ptr(row_scale), _hip.ptr(coarse_score),
                    ch, cw, lh, lw, _hip.ptr(alpha), float(l1n.eps), hoisted.c0.data_ptr(), z_local.data_ptr(),
                    partial.data_ptr(), rk, fj, _hip.ptr(score_min) if const_in_block else None,
                    what="salience_head_stage1")
    elif carry_value or carry_rank or carry_fin:
        vp = value_job.pointers() if carry_value else (None, None, None, None, 0, 0, 0, 0, None, 0, None)
        _hip.launch("sdetr_stage1_x3_with_jobs", lib, dev, *stage1_args, *vp, rk, fj, what="salience_head_stage1")
    else:
        _hip.launch("sdetr_salience_head_stage1_x3" if x3 else "sdetr_salience_head_stage1", lib, dev, *stage1_args,
                    what="salience_head_stage1")
    if carry_value:
        value_job.done = True
    if carry_rank:
        rank_job.done = True
    if carry_fin:
        finalize_job.done = True
    # (with the bf16x3 kernels stage 2's first product takes the three-plane packing too: no f32 MFMA in front of GELU)
    w2_local = None if x3 else packed_linear_weight(l2a.weight, cols=(0, half)).data_ptr()
    w2_x3 = packed_linear_weight(l2a.weight, cols=(0, half), split3=True).data_ptr() if x3 else None
    w3 = packed_linear_weight(l2b.weight).data_ptr()
    if value_job2 is not None and not value_job2.done and value_job2.value.device == dev:
        if not const_in_block:
            _hip.launch("sdetr_salience_head_const", lib, dev, partial.data_ptr(), B, n, l2a.weight.data_ptr(),
                        l2a.bias.data_ptr(), cst.data_ptr(), _hip.ptr(score_min))
        _hip.launch("sdetr_stage2_with_value_proj", lib, dev, z_local.data_ptr(), B, n, w2_local, w3, l2b.bias.data_ptr(),
                    l2c.weight.data_ptr(), l2c.bias.data_ptr(), cst.data_ptr(), score.data_ptr(), _hip.ptr(score_flat), sfs,
                    _hip.ptr(score_min), *value_job2.pointers(), w2_x3, partial.data_ptr() if const_in_block else None,
                    l2a.weight.data_ptr() if const_in_block else None, l2a.bias.data_ptr() if const_in_block else None,
                    what="salience_head_stage2")
        value_job2.done = True
    else:
        _hip.launch("sdetr_salience_head_stage2", lib, dev, z_local.data_ptr(), partial.data_ptr(), B, n,
                    l2a.weight.data_ptr(), l2a.bias.data_ptr(), w2_local, w3, l2b.bias.data_ptr(), l2c.weight.data_ptr(),
                    l2c.bias.data_ptr(), cst.data_ptr(), score.data_ptr(), _hip.ptr(score_flat), sfs, _hip.ptr(score_min),
                    w2_x3, 1 if const_in_block else 0)
    return score


def advance_rows(layer_out: Tensor, sorted_result: Tensor, next_rows: int, tokens: Tensor, sorted_index: Tensor,
                 count: Optional[Tensor] = None) -> Optional[Tensor]:
    """End of an encoder layer whose index set is ``sorted_index[:, :rows]`` (include/salience_hip.h (5)):
    records the live rows (``i < count[b]``) of ``layer_out`` [B,rows,C] in ``sorted_result`` [B,n0,C] (in place)
    and returns the next layer's queries [B,next_rows,C] -- live rows from ``layer_out``, the others straight
    from ``tokens`` [B,S,C] (never-updated originals); ``None`` when ``next_rows == 0``."""
    _hip.require_device("advance_rows", layer_out=layer_out, sorted_result=sorted_result, tokens=tokens, count=count)
    B, rows, C = layer_out.shape
    if (sorted_result.dtype != layer_out.dtype or tokens.dtype != layer_out.dtype or sorted_index.dtype != torch.int64
            or sorted_index.dim() != 2 or sorted_index.stride(1) != 1 or not sorted_index.is_cuda):
        raise RuntimeError("advance_rows: dtype / layout mismatch")
    if count is not None and (count.dtype != torch.int64 or count.numel() != B):
        raise RuntimeError("advance_rows: count must be int64 [B]")
    nxt = torch.empty((B, next_rows, C), dtype=layer_out.dtype, device=layer_out.device) if next_rows > 0 else None
    _hip.launch("sdetr_advance_rows", layer_out.dtype, layer_out.device, layer_out.data_ptr(), sorted_result.data_ptr(),
                _hip.ptr(nxt), tokens.data_ptr(), sorted_index.data_ptr(), sorted_index.stride(0), _hip.ptr(count), B,
                rows, sorted_result.shape[1], int(next_rows), tokens.shape[1], C * layer_out.element_size())
    return nxt


def _batch_stride(t: Tensor, what: str) -> int:
    """Element stride between images of a [B,n,C] tensor whose rows are contiguous (a row prefix is fine)."""
    if not t.is_cuda or t.dim() != 3 or t.stride(2) != 1 or t.stride(1) != t.shape[2]:
        raise RuntimeError(f"{what}: [B,n,C] HIP tensor with contiguous rows expected")
    return t.stride(0) if t.shape[0] > 1 else t.shape[1] * t.shape[2]


def select_stack(query: Tensor, pos: Tensor, index: Tensor) -> Tensor:
    """``cat([query[index] + pos[index], query[index]], 1)`` -> [B, 2N, C]: the q/k rows and the value rows of the
    top-k dense self-attention (salience_transformer.py:366-376) in one launch."""
    _hip.require_device("select_stack", index=index)
    if query.dtype != pos.dtype or index.dtype != torch.int64 or index.dim() != 2:
        raise RuntimeError("select_stack: query / pos of one dtype and an int64 [B,N] index expected")
    B, _, C = query.shape
    N = index.shape[1]
    out = torch.empty((B, 2 * N, C), dtype=query.dtype, device=query.device)
    _hip.launch("sdetr_select_stack", query.dtype, query.device, query.data_ptr(), _batch_stride(query, "select_stack"),
                pos.data_ptr(), _batch_stride(pos, "select_stack"), index.data_ptr(), B, N, C,
                _hip.dtype_code(query.dtype), out.data_ptr())
    return out


class FinalizeJob:
    """The token-space pass of ``encoder_finalize`` (``out = tokens + (padding ? 0 : background)``) as a pending job:
    it depends on nothing the filtering or the encoder compute, so ``salience_head(..., finalize_job=job)`` carries it
    in a stage-1 launch; ``run()`` launches it on its own.  ``encoder_finalize(..., finalize_job=job)`` then only
    overwrites the sorted rows."""

    def __init__(self, tokens: Tensor, background: Tensor, padding_mask: Optional[Tensor]):
        _hip.require_device("FinalizeJob", tokens=tokens, background=background, padding_mask=padding_mask)
        B, S, C = tokens.shape
        if (not _hip.is_act16(tokens.dtype) or C != 256 or not tokens.is_contiguous() or background.dtype != tokens.dtype
                or tuple(background.shape) != (S, C) or not background.is_contiguous()):
            raise RuntimeError("FinalizeJob: contiguous 16-bit [B,S,256] tokens and [S,256] background expected")
        self.tokens, self.background = tokens, background
        self.pad = None if padding_mask is None else (padding_mask.view(torch.uint8) if padding_mask.dtype == torch.bool
                                                      else padding_mask).contiguous()
        self.out = torch.empty_like(tokens)
        self.done = False

    def struct(self):
        st = _hip.FinalizeJobStruct()
        st.tokens, st.background, st.padding_mask = self.tokens.data_ptr(), self.background.data_ptr(), _hip.ptr(self.pad)
        st.batch, st.spatial_size, st.out = self.tokens.shape[0], self.tokens.shape[1], self.out.data_ptr()
        self._keep = st
        return st

    def run(self):
        if self.done:
            return
        self.out = self.tokens + torch.where(self.pad.bool()[..., None], torch.zeros_like(self.background[None]),
                                             self.background[None]) if self.pad is not None else self.tokens + self.background
        self.done = True


def encoder_finalize(tokens: Tensor, sorted_result: Tensor, sorted_index: Tensor, count: Optional[Tensor],
                     background: Tensor, padding_mask: Optional[Tensor], last_rows: int,
                     finalize_job: Optional[FinalizeJob] = None) -> Tensor:
    """Encoder output in token space (include/salience_hip.h (5), salience_transformer.py:474-495): live sorted
    rows replace their tokens, and every token that is neither padding nor among the first ``last_rows`` sorted
    rows (the last layer's set) receives its background embedding."""
    _hip.require_device("encoder_finalize", tokens=tokens, sorted_result=sorted_result, sorted_index=sorted_index,
                        count=count, background=background, padding_mask=padding_mask)
    B, S, C = tokens.shape
    if background.dtype != tokens.dtype or sorted_result.dtype != tokens.dtype or tuple(background.shape) != (S, C):
        raise RuntimeError("encoder_finalize: background [S,C] / sorted_result of the tokens' dtype expected")
    pad = None if padding_mask is None else (padding_mask.view(torch.uint8) if padding_mask.dtype == torch.bool
                                             else padding_mask)
    if finalize_job is not None and finalize_job.done and finalize_job.tokens is tokens:
        out = finalize_job.out      # the token-space pass has run (carried by a filtering launch): sorted rows only
        _hip.launch("sdetr_encoder_finalize_sorted", tokens.dtype, tokens.device, tokens.data_ptr(),
                    sorted_result.data_ptr(), sorted_index.data_ptr(), _hip.ptr(count), background.data_ptr(),
                    _hip.ptr(pad), B, S, sorted_result.shape[1], int(last_rows), C, _hip.dtype_code(tokens.dtype),
                    out.data_ptr(), what="encoder_finalize")
        return out
    out = torch.empty_like(tokens)
    _hip.launch("sdetr_encoder_finalize", tokens.dtype, tokens.device, tokens.data_ptr(), sorted_result.data_ptr(),
                sorted_index.data_ptr(), _hip.ptr(count), background.data_ptr(), _hip.ptr(pad), B, S,
                sorted_result.shape[1], int(last_rows), C, _hip.dtype_code(tokens.dtype), out.data_ptr())
    return out


def fused_ffn_applies(x: Tensor, linear1, linear2, norm, activation) -> bool:
    """The one-launch MFMA feed-forward (csrc/ffn.hip) covers the released configuration: bf16, embed_dim 256, ReLU,
    hidden a multiple of 32 that fits its LDS budget.  A 128-token block keeps a CU for ~55 us at hidden 2048; smaller
    token counts are spread over the chip by splitting the hidden dimension (``sdetr_ffn_auto_splits``) -- measured
    against the two library GEMMs + LayerNorm on MI355X: 23 vs 67 us at 1800 tokens, 27 vs 67 at 4544, 36 vs 68 at 9090,
    44 vs 74 at 13 634, 66 vs 116 at 18 180."""
    return (x.numel() >= 1000 * 256 and x.is_cuda and _hip.is_act16(x.dtype) and x.shape[-1] == 256 and isinstance(activation, torch.nn.ReLU)
            and linear1.weight.dtype == x.dtype and linear2.weight.dtype == x.dtype
            and linear1.in_features == 256 and linear2.out_features == 256
            and linear1.out_features == linear2.in_features and linear1.out_features % 32 == 0
            and linear1.out_features <= 8192 and linear1.bias is not None and linear2.bias is not None)


def _ffn_operands(linear1, linear2, norm):
    """(packed weights, fp32 bias1, bias2, norm weight, norm bias) of the fused feed-forward, cached on
    ``linear1.weight`` and refreshed when any parameter changes."""
    def build():
        lib = _hip.lib(linear1.weight.dtype)
        F, dev = linear1.out_features, linear1.weight.device
        with torch.no_grad(), torch.cuda.device(dev):
            packed = torch.empty(lib.sdetr_ffn_packed_bytes(F), dtype=torch.uint8, device=dev)
            w1, w2 = linear1.weight.detach().contiguous(), linear2.weight.detach().contiguous()
            _hip.launch("sdetr_ffn_pack_bf16", lib, dev, w1.data_ptr(), w2.data_ptr(), 256, F, packed.data_ptr(),
                        what="ffn_pack")
            small = [t.detach().float().contiguous() for t in (linear1.bias, linear2.bias, norm.weight, norm.bias)]
        return packed, small
    return derived(linear1.weight, "ffn", (linear1.weight, linear1.bias, linear2.weight, linear2.bias, norm.weight,
                                           norm.bias), build)


def fused_ffn(x: Tensor, linear1, linear2, norm, hidden_splits: Optional[int] = None) -> Tensor:
    """``norm(x + linear2(relu(linear1(x))))`` in one launch (include/salience_hip.h (7)).  The packed weights and
    fp32 copies of the small vectors live on ``linear1.weight`` and are refreshed when any parameter changes.
    ``hidden_splits``: pieces of the hidden dimension per 128-token block (default: chosen for the device so that
    small token counts still fill it; > 1 adds a reduce + LayerNorm launch)."""
    if not x.is_cuda:
        raise RuntimeError("fused_ffn: HIP device tensors required; there is no CPU fallback")
    lib = _hip.lib(x.dtype)
    F = linear1.out_features
    packed, (b1, b2, g, be) = _ffn_operands(linear1, linear2, norm)
    x2 = x.reshape(-1, 256)
    if not x2.is_contiguous():
        x2 = x2.contiguous()
    out = torch.empty_like(x2)
    T = x2.shape[0]
    with torch.cuda.device(x.device):      # (the choice reads the current device's CU count)
        splits = int(hidden_splits) if hidden_splits else lib.sdetr_ffn_auto_splits(T, F)
    ws_bytes = lib.sdetr_ffn_workspace_bytes(T, splits)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device) if ws_bytes else None
    _hip.launch("sdetr_ffn_fused_bf16", lib, x.device, x2.data_ptr(), packed.data_ptr(), b1.data_ptr(), b2.data_ptr(),
                g.data_ptr(), be.data_ptr(), float(norm.eps), T, 256, F, out.data_ptr(), splits, _hip.ptr(ws), ws_bytes,
                what="ffn_fused")
    return out.view(x.shape)


def fused_ffn_advance(x: Tensor, linear1, linear2, norm, sorted_result: Tensor, next_rows: int, tokens: Tensor,
                      sorted_index: Tensor, count: Optional[Tensor] = None,
                      hidden_splits: Optional[int] = None) -> Optional[Tensor]:
    """``advance_rows(fused_ffn(x, ...), sorted_result, next_rows, tokens, sorted_index, count)`` as one operator
    (``sdetr_ffn_fused_advance_bf16``): the end of an encoder layer.  With a split hidden dimension the reduce +
    LayerNorm pass writes the live rows straight into ``sorted_result`` and the next layer's queries -- the layer
    output is never materialised and ``advance_rows`` is no launch of its own."""
    _hip.require_device("fused_ffn_advance", x=x, sorted_result=sorted_result, tokens=tokens, count=count)
    if x.dim() != 3 or not x.is_contiguous() or x.shape[2] != 256:
        raise RuntimeError("fused_ffn_advance: contiguous [B, rows, 256] queries expected")
    B, rows, C = x.shape
    if (sorted_result.dtype != x.dtype or tokens.dtype != x.dtype or sorted_index.dtype != torch.int64
            or sorted_index.dim() != 2 or sorted_index.stride(1) != 1 or not sorted_index.is_cuda
            or not sorted_result.is_contiguous() or not tokens.is_contiguous()):
        raise RuntimeError("fused_ffn_advance: dtype / layout mismatch")
    if count is not None and (count.dtype != torch.int64 or count.numel() != B):
        raise RuntimeError("fused_ffn_advance: count must be int64 [B]")
    lib = _hip.lib(x.dtype)
    F = linear1.out_features
    packed, (b1, b2, g, be) = _ffn_operands(linear1, linear2, norm)
    nxt = torch.empty((B, next_rows, C), dtype=x.dtype, device=x.device) if next_rows > 0 else None
    with torch.cuda.device(x.device):      # (the choice reads the current device's CU count)
        splits = int(hidden_splits) if hidden_splits else lib.sdetr_ffn_auto_splits(B * rows, F)
    ws_bytes = lib.sdetr_ffn_workspace_bytes(B * rows, splits) + (B * rows * 512 if splits == 1 else 0)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=x.device)
    _hip.launch("sdetr_ffn_fused_advance_bf16", lib, x.device, x.data_ptr(), packed.data_ptr(), b1.data_ptr(),
                b2.data_ptr(), g.data_ptr(), be.data_ptr(), float(norm.eps), B, rows, 256, F, splits, ws.data_ptr(),
                ws_bytes, sorted_result.data_ptr(), _hip.ptr(nxt), tokens.data_ptr(), sorted_index.data_ptr(),
                sorted_index.stride(0), _hip.ptr(count), sorted_result.shape[1], int(next_rows), tokens.shape[1],
                what="ffn_fused_advance")
    return nxt


def attn_tail_ffn_applies(sampled: Tensor, residual: Tensor, output_proj, norm1, linear1, linear2, norm2, activation) -> bool:
    """The layer-end operator (``attn_tail_ffn_advance``) covers the bf16 benchmark configuration."""
    return (sampled.dim() == 3 and sampled.shape == residual.shape and sampled.is_contiguous() and residual.is_contiguous()
            and _hip.is_act16(residual.dtype) and sampled.dtype == residual.dtype
            and fused_ffn_applies(residual, linear1, linear2, norm2, activation)
            and output_proj.weight.dtype == residual.dtype and tuple(output_proj.weight.shape) == (256, 256)
            and output_proj.bias is not None and norm1.weight is not None and norm1.bias is not None
            and norm1.normalized_shape == (256,))


def _tail_ffn_operands(output_proj, norm1, linear1, linear2, norm2, class_head=None):
    """``(packed [Wo tail | feed-forward | class head], fp32 (bo, gamma1, beta1, b1, b2, gamma2, beta2, class bias padded
    to 96 with -inf))``, cached on ``output_proj.weight`` (one entry with, one without the class head) and refreshed when
    any of the parameters changes."""
    params = (output_proj.weight, output_proj.bias, norm1.weight, norm1.bias, linear1.weight, linear1.bias, linear2.weight,
              linear2.bias, norm2.weight, norm2.bias)
    if class_head is not None:
        params = params + (class_head.weight, class_head.bias)

    def build():
        lib = _hip.lib(output_proj.weight.dtype)
        F, dev = linear1.out_features, output_proj.weight.device
        with torch.no_grad(), torch.cuda.device(dev):
            tail_bytes, ffn_bytes = lib.sdetr_attn_tail_packed_bytes(), lib.sdetr_ffn_packed_bytes(F)
            cls_bytes = lib.sdetr_class_head_packed_bytes() if class_head is not None else 0
            packed = torch.empty(tail_bytes + ffn_bytes + cls_bytes, dtype=torch.uint8, device=dev)
            wo = output_proj.weight.detach().contiguous()
            _hip.launch("sdetr_attn_tail_pack_bf16", lib, dev, wo.data_ptr(), 256, packed.data_ptr(),
                        what="attn_tail_pack")
            w1, w2 = linear1.weight.detach().contiguous(), linear2.weight.detach().contiguous()
            _hip.launch("sdetr_ffn_pack_bf16", lib, dev, w1.data_ptr(), w2.data_ptr(), 256, F,
                        packed.data_ptr() + tail_bytes, what="ffn_pack")
            small = [t.detach().float().contiguous() for t in (output_proj.bias, norm1.weight, norm1.bias, linear1.bias,
                                                               linear2.bias, norm2.weight, norm2.bias)]
            if class_head is not None:
                wc = class_head.weight.detach().contiguous()
                _hip.launch("sdetr_class_head_pack_bf16", lib, dev, wc.data_ptr(), wc.shape[0], 256,
                            packed.data_ptr() + tail_bytes + ffn_bytes, what="class_head_pack")
                cb = torch.full((96,), float("-inf"), dtype=torch.float32, device=dev)
                cb[:wc.shape[0]] = class_head.bias.detach().float()
                small.append(cb)
        return packed, small
    return derived(output_proj.weight, "tail_ffn" if class_head is None else "tail_ffn_cls", params, build)


# The second pass of a split hidden dimension computes the next layer's class score (csrc/ffn.hip,
# ffn_reduce_ln_advance_cls_kernel); False = the caller launches the class head (the form up to round 6, for A/B runs).
SPLIT_PASS_CLASS_SCORE = True


def attn_tail_ffn_advance(sampled: Tensor, residual: Tensor, output_proj, norm1, linear1, linear2, norm2,
                          sorted_result: Tensor, next_rows: int, tokens: Tensor, sorted_index: Tensor,
                          count: Optional[Tensor] = None, hidden_splits: Optional[int] = None, next_class_head=None,
                          foreground: Optional[Tensor] = None):
    """The end of an encoder layer as ONE operator (``sdetr_attn_tail_ffn_advance_bf16``):
    ``x = norm1(residual + output_proj(sampled))``, ``y = norm2(x + linear2(relu(linear1(x))))``, then
    ``advance_rows(y, ...)`` -- i.e. ``fused_ffn_advance(token_linear_ln(sampled, output_proj, norm1, residual), ...)``
    without the launch, the weight pipeline start-up and the [rows, 256] round trip of the first half.

    ``next_class_head`` + ``foreground`` ([B, >= next_rows] fp32): returns ``(next_query, score)`` where ``score``
    [B, next_rows] is the NEXT layer's selection score ``class_head_max_times(next_query, next_class_head, foreground)`` --
    computed in the feed-forward launch's epilogue (one hidden piece) or by the second pass of a split hidden dimension;
    ``None`` when the class head does not fit the kernels (the caller launches it)."""
    _hip.require_device("attn_tail_ffn_advance", sampled=sampled, residual=residual, sorted_result=sorted_result, tokens=tokens,
                        count=count, foreground=foreground)
    if sampled.dim() != 3 or sampled.shape != residual.shape or sampled.shape[2] != 256 or not sampled.is_contiguous() \
            or not residual.is_contiguous() or not _hip.is_act16(residual.dtype) or sampled.dtype != residual.dtype:
        raise RuntimeError("attn_tail_ffn_advance: contiguous 16-bit [B, rows, 256] sampled heads and queries expected")
    B, rows, C = residual.shape
    if (sorted_result.dtype != residual.dtype or tokens.dtype != residual.dtype or sorted_index.dtype != torch.int64
            or sorted_index.dim() != 2 or sorted_index.stride(1) != 1 or not sorted_index.is_cuda
            or not sorted_result.is_contiguous() or not tokens.is_contiguous()):
        raise RuntimeError("attn_tail_ffn_advance: dtype / layout mismatch")
    if count is not None and (count.dtype != torch.int64 or count.numel() != B):
        raise RuntimeError("attn_tail_ffn_advance: count must be int64 [B]")
    lib = _hip.lib(residual.dtype)
    F = linear1.out_features
    with torch.cuda.device(residual.device):
        splits = int(hidden_splits) if hidden_splits else lib.sdetr_ffn_auto_splits(B * rows, F)
    want_score = next_class_head is not None
    with_score = (want_score and (splits == 1 or SPLIT_PASS_CLASS_SCORE) and next_rows > 0 and foreground is not None
                  and next_class_head.weight.dtype == residual.dtype and next_class_head.weight.shape[0] <= 96
                  and next_class_head.weight.shape[1] == 256 and next_class_head.bias is not None)
    if with_score and (foreground.dtype != torch.float32 or foreground.dim() != 2 or foreground.shape[0] != B
                       or foreground.shape[1] < next_rows or foreground.stride(1) != 1):
        raise RuntimeError("attn_tail_ffn_advance: foreground must be fp32 [B, >= next_rows] rows")
    ops = _tail_ffn_operands(output_proj, norm1, linear1, linear2, norm2, next_class_head if with_score else None)
    packed, (bo, g1, be1, b1, b2, g2, be2) = ops[0], ops[1][:7]
    cls_bias = ops[1][7] if with_score else None
    nxt = torch.empty((B, next_rows, C), dtype=residual.dtype, device=residual.device) if next_rows > 0 else None
    score = torch.empty((B, next_rows), dtype=torch.float32, device=residual.device) if with_score else None
    ws_bytes = lib.sdetr_ffn_workspace_bytes(B * rows, splits) + (B * rows * 512 if splits == 1 else 0)
    ws = torch.empty(max(ws_bytes, 16), dtype=torch.uint8, device=residual.device)
    _hip.launch("sdetr_attn_tail_ffn_advance_bf16", lib, residual.device, sampled.data_ptr(), residual.data_ptr(),
                packed.data_ptr(), bo.data_ptr(), g1.data_ptr(), be1.data_ptr(), float(norm1.eps), b1.data_ptr(),
                b2.data_ptr(), g2.data_ptr(), be2.data_ptr(), float(norm2.eps), B, rows, 256, F, splits, ws.data_ptr(),
                ws_bytes, sorted_result.data_ptr(), _hip.ptr(nxt), tokens.data_ptr(), sorted_index.data_ptr(),
                sorted_index.stride(0), _hip.ptr(count), sorted_result.shape[1], int(next_rows), tokens.shape[1],
                _hip.ptr(cls_bias), _hip.ptr(foreground) if with_score else None,
                (foreground.stride(0) if B > 1 else foreground.shape[1]) if with_score else 0, _hip.ptr(score),
                what="attn_tail_ffn_advance")
    return (nxt, score) if want_score else nxt


def _packed_linear_bf16(weight: Tensor, bias: Optional[Tensor]):
    """(packed weight, zero-padded fp32 bias) of a ``[N,256]`` bf16 Linear for the token-resident kernels, cached on
    the weight tensor object and refreshed when weight / bias storage or version change."""
    def build():
        lib = _hip.lib(weight.dtype)
        w = weight.detach()
        N = w.shape[0]
        npad = (N + 127) // 128 * 128
        with torch.no_grad(), torch.cuda.device(w.device):
            packed = torch.empty(lib.sdetr_linear_packed_bytes(N), dtype=torch.uint8, device=w.device)
            _hip.launch("sdetr_linear_pack_bf16", lib, w.device, w.data_ptr(), w.stride(0), N, w.shape[1],
                        packed.data_ptr(), what="linear_pack")
            b = torch.zeros(npad, dtype=torch.float32, device=w.device)
            if bias is not None:
                b[:N] = bias.detach().float()
        return packed, b
    return derived(weight, "token_linear", (weight, bias), build)


def _fragment_order(weight: Tensor, rows_per_head: int) -> Tensor:
    """``weight`` ([8 * rows_per_head, 256] 16-bit, rows grouped by head) in the fragment order of the top-300 attention's
    16x16x32 products: ``[head][16-row tile][k-step of 32][lane][8]`` with lane = (row & 15) + 16 * (k / 8 & 3) -- a wave's
    operand fragment is one contiguous KB (include/salience_hip.h, sdetr_topk_attention_with_projection_bf16).  Cached on
    the weight object, refreshed when its storage or version changes."""
    def build():
        tiles = rows_per_head // 16
        with torch.no_grad():
            # [head, tile c, row t, k-step j, quarter g, element e] -> [head, c, j, g, t, e]
            return weight.detach().view(8, tiles, 16, 8, 4, 8).permute(0, 1, 3, 4, 2, 5).contiguous()
    return derived(weight, "fragment_order", (weight,), build, extra=rows_per_head)


def token_linear_applies(x: Tensor, weight: Tensor) -> bool:
    return (x.is_cuda and _hip.is_act16(x.dtype) and weight.dtype == x.dtype and x.shape[-1] == 256
            and weight.dim() == 2 and weight.shape[1] == 256 and weight.stride(1) == 1)


def token_linear(x: Tensor, weight: Tensor, bias: Optional[Tensor], x_add: Optional[Tensor] = None,
                 group_features: int = 0) -> Tensor:
    """``F.linear(x (+ x_add), weight, bias)`` for bf16 ``[B,n,256]`` tokens with the activations resident in
    registers (include/salience_hip.h (8)); ``x_add`` may be a row prefix of a longer ``[B,n',256]`` buffer.
    ``group_features = g`` returns the result feature-group-major, ``[B, N/g, n, g]``."""
    if not token_linear_applies(x, weight):
        raise RuntimeError("token_linear: bf16 HIP tensors with 256 input features expected; no CPU fallback")
    shape = x.shape
    x3 = x if x.dim() == 3 else x.reshape(1, -1, 256)
    if not x3.is_contiguous():
        x3 = x3.contiguous()
    B, n, _ = x3.shape
    N = weight.shape[0]
    if N % 4:
        raise RuntimeError("token_linear: out_features must be a multiple of 4")
    packed, b = _packed_linear_bf16(weight, bias)
    if group_features and (N % group_features or group_features % 4):
        raise RuntimeError("token_linear: group_features must divide out_features and be a multiple of 4")
    out = torch.empty((B, N // group_features, n, group_features) if group_features else (B, n, N),
                      dtype=x.dtype, device=x.device)
    abs_ = 0
    if x_add is not None:
        if x_add.dtype != x.dtype or tuple(x_add.shape) != (B, n, 256):
            raise RuntimeError("token_linear: x_add must match x")
        abs_ = _batch_stride(x_add, "token_linear")
    _hip.launch("sdetr_token_linear_bf16", x.dtype, x.device, x3.data_ptr(), _hip.ptr(x_add), abs_, n, B * n, 256,
                packed.data_ptr(), b.data_ptr(), N, out.data_ptr(), N, int(group_features), what="token_linear")
    return out if group_features else out.view(tuple(shape[:-1]) + (N,))


class RowOrdersJob:
    """``layer_row_orders`` not launched yet: ``masked_topk_desc(..., orders_job=job)`` lets the layer-0 selection's launch
    carry it, ``job.run()`` launches it on its own.  ``job.orders``: the per-layer ``[B,c_k]`` int32 views it fills."""

    def __init__(self, sorted_index, tile_pos, counts_dev, counts, S, order):
        B, n0 = sorted_index.shape
        self.device = sorted_index.device
        self._keep = (sorted_index, tile_pos, counts_dev, order)
        self.struct = _hip.RowOrdersJobStruct(sorted_index.data_ptr(), sorted_index.stride(0), tile_pos.data_ptr(), B, S, n0,
                                              len(counts), counts_dev.data_ptr(), order.data_ptr(), n0)
        self.orders = [order[k, :, :c] for k, c in enumerate(counts)]
        self.done = False

    def run(self):
        if self.done:
            return
        j = self.struct
        _hip.launch("sdetr_layer_row_orders", None, self.device, j.sorted_index, j.index_batch_stride, j.tile_pos,
                    j.batch, j.spatial_size, j.num_rows, j.num_layers, j.counts, j.order, j.order_batch_stride)
        self.done = True


def layer_row_orders(sorted_index: Tensor, counts, level_shapes, tile: int = 16, as_job: bool = False):
    """Per-layer row orders for the bordered MSDA kernel (include/salience_hip.h ``sdetr_layer_row_orders``):
    ``sorted_index`` int64 ``[B,n0]`` (the token of every row of the sorted list), ``counts`` the layers' row counts
    (non-increasing, ``counts[0] <= n0``) -> list of int32 ``[B,c_k]`` views (rows ``n0`` apart), each a permutation of
    ``0..c_k-1`` that walks the layer's rows tile by tile of the finest level.  ``None`` when the list is too long for
    the kernel's 16-bit row slots (65 534 rows per image; the caller then runs the rows in list order) -- pyramids whose
    tile positions do not fit one workgroup's LDS take several passes (round 5: the 5scale pyramid's 89 250 in two).  ``as_job``: return the pending
    ``RowOrdersJob`` instead of launching it."""
    from .ms_deform_attn import tile_major_positions
    _hip.require_device("layer_row_orders", sorted_index=sorted_index)
    B, n0 = sorted_index.shape
    S = sum(int(h) * int(w) for h, w in level_shapes)
    counts = [int(c) for c in counts]
    if S > (1 << 20) or n0 >= 0xffff or len(counts) > 8 or sorted_index.dtype != torch.int64 or max(counts) > n0:
        return None
    dev = sorted_index.device
    key = ("row_orders", tuple(map(tuple, level_shapes)), int(tile), tuple(counts), str(dev))

    def build():
        return (tile_major_positions(level_shapes, tile).to(dev), torch.tensor(counts, dtype=torch.int32).to(dev))
    from . import pyramid
    tile_pos, counts_dev = pyramid.static_tensor(key, build)
    order = torch.empty((len(counts), B, n0), dtype=torch.int32, device=dev)
    job = RowOrdersJob(sorted_index, tile_pos, counts_dev, counts, S, order)
    if as_job:
        return job            # (``as_job``: the pending job; None above still means "no orders for this pyramid")
    job.run()
    return job.orders


def value_proj_head_major(value: Tensor, weight: Tensor, bias: Optional[Tensor], padding_mask: Optional[Tensor],
                          num_heads: int, num_groups: int, dtype: torch.dtype, bordered_levels=None) -> Tensor:
    """``value_proj`` of ``num_groups`` stacked layers + ``masked_fill`` + head-major re-layout in one launch:
    value ``[B,Nv,256]`` bf16, weight ``[groups*heads*32, 256]`` -> ``[groups,B,heads,Nv,32]`` fp16 | bf16
    (``bordered_levels``: ``[groups,B,heads,Np,32]`` in the bordered layout of that pyramid)."""
    if not token_linear_applies(value, weight) or weight.shape[0] != num_groups * num_heads * 32:
        raise RuntimeError("value_proj_head_major: bf16 [B,Nv,256] tokens and 32-channel heads expected")
    _hip.require_device("value_proj_head_major", value=value, padding_mask=padding_mask)
    B, Nv, _ = value.shape
    packed, b = _packed_linear_bf16(weight, bias)
    pad = None if padding_mask is None else (padding_mask.view(torch.uint8) if padding_mask.dtype == torch.bool
                                             else padding_mask)
    bordered = None if bordered_levels is None else bordered_struct(bordered_levels, value.device)
    records = Nv if bordered is None else bordered[0].records
    dst = torch.empty((num_groups, B, num_heads, records, 32), dtype=dtype, device=value.device)
    _hip.launch("sdetr_value_proj_head_major", value.dtype, value.device, value.data_ptr(), packed.data_ptr(),
                b.data_ptr(), _hip.ptr(pad), B, Nv, 256, num_heads, 32, num_groups, dst.data_ptr(),
                _hip.dtype_code(dtype), None if bordered is None else ctypes.byref(bordered[0]))
    return dst


def class_head_max_times(x: Tensor, class_head, scale: Tensor) -> Tensor:
    """``class_head(x).max(-1)[0] * scale`` (mc_score, salience_transformer.py:365-366) without the logits:
    x ``[B,n,256]`` bf16, scale ``[B,n]`` fp32 (may be a row prefix of a longer buffer) -> fp32 ``[B,n]``."""
    if not token_linear_applies(x, class_head.weight) or x.dim() != 3:
        raise RuntimeError("class_head_max_times: bf16 [B,n,256] HIP tokens expected; no CPU fallback")
    _hip.require_device("class_head_max_times", x=x)
    B, n, _ = x.shape
    if scale.dtype != torch.float32 or scale.dim() != 2 or (n > 1 and scale.stride(1) != 1) or not scale.is_cuda:
        scale = scale.float().contiguous()
    packed, b = _packed_linear_bf16(class_head.weight, class_head.bias)
    out = torch.empty((B, n), dtype=torch.float32, device=x.device)
    _hip.launch("sdetr_class_head_max_times", x.dtype, x.device, x.data_ptr(), packed.data_ptr(), b.data_ptr(), 256,
                class_head.out_features, scale.data_ptr(), scale.stride(0) if B > 1 else max(n, 1), B, n,
                out.data_ptr())
    return out


def masked_fill_min(score: Tensor, mask: Tensor, mins: Tensor) -> Tensor:
    """``torch.where(mask, mins.min(), score)`` in one launch (foreground_score, salience_transformer.py:164-168,
    from the per-level minima that are already on the device)."""
    _hip.require_device("masked_fill_min", score=score, mask=mask, mins=mins)
    if score.dtype != torch.float32 or mins.dtype != torch.float32 or mask.shape != score.shape:
        raise RuntimeError("masked_fill_min: fp32 score / mins and a mask of score's shape expected")
    m = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    out = torch.empty_like(score)
    _hip.launch("sdetr_masked_fill_min", None, score.device, score.data_ptr(), m.data_ptr(), mins.data_ptr(),
                mins.numel(), score.numel(), out.data_ptr())
    return out


def encoder_reference_points(valid_ratios: Tensor, spatial_shapes: Tensor, level_start_index: Tensor, rows: int,
                             index: Optional[Tensor] = None) -> Tensor:
    """``get_reference_points`` (salience_transformer.py:418-432) evaluated only for the tokens ``index[b,i]``
    (all ``rows`` tokens in order when ``index`` is None) -> ``[B,rows,L,2]`` fp32."""
    _hip.require_device("encoder_reference_points", valid_ratios=valid_ratios, spatial_shapes=spatial_shapes,
                        level_start_index=level_start_index)
    B, L, _ = valid_ratios.shape
    if valid_ratios.dtype != torch.float32 or spatial_shapes.dtype != torch.int64:
        raise RuntimeError("encoder_reference_points: fp32 valid ratios and int64 shapes expected")
    ibs = 0
    if index is not None:
        if index.dtype != torch.int64 or index.dim() != 2 or not index.is_cuda or (index.shape[1] > 1 and index.stride(1) != 1):
            raise RuntimeError("encoder_reference_points: int64 [B,n] index with a contiguous last dim expected")
        rows = index.shape[1]
        ibs = index.stride(0) if B > 1 else rows
    out = torch.empty((B, rows, L, 2), dtype=torch.float32, device=valid_ratios.device)
    _hip.launch("sdetr_encoder_reference_points", None, valid_ratios.device, valid_ratios.data_ptr(),
                spatial_shapes.data_ptr(), level_start_index.data_ptr(), _hip.ptr(index), ibs, B, int(rows), L,
                out.data_ptr())
    return out


def _host_level_shapes(level_shapes):
    import ctypes
    flat = [int(v) for hw in level_shapes for v in hw]
    return (ctypes.c_int64 * len(flat))(*flat)


def encoder_output_proposals(padding_mask: Tensor, level_shapes, want_logit: bool = True):
    """The geometry half of ``gen_encoder_output_proposals`` (base_transformer.py:74-112): ``keep`` ``[B,S]`` bool
    (token not padding and its proposal inside (0.01, 0.99)) and the proposal logits ``[B,S,4]`` fp32 (+inf where
    ``keep`` is False).  ``level_shapes``: host list of (h, w)."""
    _hip.require_device("encoder_output_proposals", padding_mask=padding_mask)
    B, S = padding_mask.shape
    m = padding_mask.contiguous()
    m = m.view(torch.uint8) if m.dtype == torch.bool else m
    keep = torch.empty((B, S), dtype=torch.uint8, device=m.device)
    logit = torch.empty((B, S, 4), dtype=torch.float32, device=m.device) if want_logit else None
    shapes = _host_level_shapes(level_shapes)
    _hip.launch("sdetr_encoder_output_proposals", None, m.device, m.data_ptr(), shapes, len(level_shapes), B, S,
                keep.data_ptr(), _hip.ptr(logit))
    return keep.view(torch.bool), logit


def nms_neighbourhood(iou_threshold: float) -> int:
    """Which grid neighbours the reference's unit boxes suppress at ``iou_threshold``: the IoU of two 2x2 boxes one
    cell apart is 2/6 (edge) or 1/7 (corner), compared in fp32 like torchvision's kernel does."""
    import numpy as np
    thr = np.float32(iou_threshold)
    edge = np.float32(2) / np.float32(6) > thr
    corner = np.float32(1) / np.float32(7) > thr
    return 8 if corner else (4 if edge else 0)


def grid_nms_topk(topk_index: Tensor, level_shapes, spatial_size: int, iou_threshold: float, max_keep: int):
    """``nms_on_topk_index`` (salience_transformer.py:249-295) up to the final truncation: ``topk_index`` ``[B,K]``
    int64 token ids in descending score order -> (kept ids ``[B,max_keep]`` in score order, kept count ``[B]`` int32,
    device; entries of a row beyond its count are undefined)."""
    _hip.require_device("grid_nms_topk", topk_index=topk_index)
    if topk_index.dtype != torch.int64 or topk_index.dim() != 2 or (topk_index.shape[1] > 1 and topk_index.stride(1) != 1):
        raise RuntimeError("grid_nms_topk: int64 [B,K] index with a contiguous last dim expected")
    B, K = topk_index.shape
    out = torch.empty((B, max_keep), dtype=torch.int64, device=topk_index.device)
    count = torch.empty((B,), dtype=torch.int32, device=topk_index.device)
    shapes = _host_level_shapes(level_shapes)
    _hip.launch("sdetr_grid_nms_topk", None, topk_index.device, topk_index.data_ptr(),
                topk_index.stride(0) if B > 1 else K, shapes, len(level_shapes), B, K, int(spatial_size),
                nms_neighbourhood(iou_threshold), int(max_keep), out.data_ptr(), count.data_ptr())
    return out, count


def proposal_refine(delta: Tensor, proposal_logit: Tensor, index: Tensor) -> Tensor:
    """``sigmoid(delta + proposal_logit.gather(index))``: enc_outputs_coord of the selected tokens
    (salience_transformer.py:198-199, 209).  delta ``[B,n,4]`` fp32 | bf16, logits ``[B,S,4]`` fp32, index ``[B,n]``."""
    _hip.require_device("proposal_refine", delta=delta, proposal_logit=proposal_logit, index=index)
    B, n, _ = delta.shape
    if (delta.dtype not in (torch.float32,) + _hip.ACT16 or proposal_logit.dtype != torch.float32
            or index.dtype != torch.int64 or tuple(index.shape) != (B, n) or (n > 1 and index.stride(1) != 1)):
        raise RuntimeError("proposal_refine: delta [B,n,4] fp32 | bf16, logits fp32 [B,S,4], index int64 [B,n] expected")
    d = delta.contiguous()
    lg = proposal_logit.contiguous()
    out = torch.empty((B, n, 4), dtype=torch.float32, device=d.device)
    _hip.launch("sdetr_proposal_refine", d.dtype, d.device, d.data_ptr(), _hip.dtype_code(d.dtype), lg.data_ptr(),
                index.data_ptr(), index.stride(0) if B > 1 else n, B, lg.shape[1], n, out.data_ptr())
    return out


def attention_heads_applies(q: Tensor, k: Tensor, v: Tensor, num_heads: int) -> bool:
    return (q.is_cuda and q.dtype == k.dtype == v.dtype and _hip.is_act16(q.dtype) and q.dim() == 3 and q.shape == k.shape == v.shape
            and q.shape[-1] == 32 * num_heads and 0 < q.shape[1] <= 1152
            and all(t.stride(2) == 1 and t.stride(1) % 8 == 0 and t.stride(0) % 8 == 0 for t in (q, k, v)))


def attention_heads(q: Tensor, k: Tensor, v: Tensor, num_heads: int) -> Tensor:
    """``softmax(Q_h K_h^T / sqrt(32)) V_h`` per head, heads concatenated: q, k, v ``[B,n,32*heads]`` bf16 (column slices
    of a wider projection output are fine) -> ``[B,n,32*heads]`` (the input of ``out_proj``).  No mask, n <= 1152."""
    if not attention_heads_applies(q, k, v, num_heads):
        raise RuntimeError("attention_heads: bf16 HIP tensors [B,n,32*heads] with n <= 1152 expected; no CPU fallback")
    B, n, E = q.shape
    out = torch.empty((B, n, E), dtype=q.dtype, device=q.device)
    _hip.launch("sdetr_attention_heads_bf16", q.dtype, q.device, q.data_ptr(), q.stride(0), q.stride(1), k.data_ptr(),
                k.stride(0), k.stride(1), v.data_ptr(), v.stride(0), v.stride(1), B, n, num_heads, 32,
                1.0 / math.sqrt(32.0), out.data_ptr(), what="attention_heads")
    return out


def decoder_query_sine_embed(reference_points: Tensor, valid_ratios: Tensor, num_pos_feats: int,
                             dtype: torch.dtype, temperature: float = 10000.0):
    """``reference_points_input`` and its sine embedding for one decoder layer (salience_transformer.py:642-643):
    boxes ``[B,Nq,4]`` fp32, ``valid_ratios`` ``[B,L,2]`` -> (``[B,Nq,L,4]`` fp32, ``[B,Nq,4*num_pos_feats]``)."""
    _hip.require_device("decoder_query_sine_embed", reference_points=reference_points, valid_ratios=valid_ratios)
    if reference_points.dim() != 3 or reference_points.shape[-1] != 4 or dtype not in (torch.float32,) + _hip.ACT16:
        raise RuntimeError("decoder_query_sine_embed: [B,Nq,4] boxes and an fp32 | bf16 embedding expected")
    ref = reference_points.detach().float().contiguous()
    vr = valid_ratios.float().contiguous()
    B, Nq, _ = ref.shape
    L = vr.shape[1]
    embed = torch.empty((B, Nq, 4 * num_pos_feats), dtype=dtype, device=ref.device)
    ref_in = torch.empty((B, Nq, L, 4), dtype=torch.float32, device=ref.device)
    _hip.launch("sdetr_decoder_query_sine_embed", dtype, ref.device, ref.data_ptr(), vr.data_ptr(), B, Nq, L,
                int(num_pos_feats), float(temperature), embed.data_ptr(), _hip.dtype_code(dtype), ref_in.data_ptr())
    return ref_in, embed


def rows_linear_ln_applies(x: Tensor, linear, norm) -> bool:
    """``rows_linear_ln`` takes this tail: 16-bit HIP rows of 256 features, a 256 -> 256 Linear and an affine
    LayerNorm(256), no autograd."""
    return (x.is_cuda and _hip.is_act16(x.dtype) and x.shape[-1] == 256 and not torch.is_grad_enabled()
            and linear.in_features == 256 and linear.out_features == 256 and linear.bias is not None
            and linear.weight.dtype == x.dtype and linear.weight.stride(1) == 1
            and isinstance(norm, torch.nn.LayerNorm) and tuple(norm.normalized_shape) == (256,)
            and norm.weight is not None and norm.bias is not None)


def rows_linear_ln(x: Tensor, linear, norm, residual: Tensor) -> Tensor:
    """``norm(residual + linear(x))`` in one launch for a few thousand rows (include/salience_hip.h,
    ``sdetr_rows_linear_ln_bf16``)."""
    if not rows_linear_ln_applies(x, linear, norm):
        raise RuntimeError("rows_linear_ln: 16-bit HIP rows, a 256 -> 256 Linear and LayerNorm(256) expected; no CPU fallback")
    if residual.shape != x.shape or residual.dtype != x.dtype or residual.device != x.device:
        raise RuntimeError("rows_linear_ln: residual must match x")
    xa = x if x.is_contiguous() else x.contiguous()
    ra = residual if residual.is_contiguous() else residual.contiguous()
    packed, b = _packed_linear_bf16(linear.weight, linear.bias)
    g, be = _norm_f32(norm)
    out = torch.empty(x.shape, dtype=x.dtype, device=x.device)
    _hip.launch("sdetr_rows_linear_ln_bf16", x.dtype, x.device, xa.data_ptr(), ra.data_ptr(), xa.numel() // 256,
                packed.data_ptr(), b.data_ptr(), g.data_ptr(), be.data_ptr(), float(norm.eps), out.data_ptr(),
                what="rows_linear_ln")
    return out


def ref_point_head_applies(layers, dtype: torch.dtype, num_pos_feats: int) -> bool:
    """``ref_point_head`` (sine embedding + 512 -> 256 -> 256 chain in one launch) takes these layers."""
    layers = list(layers)
    return (_hip.is_act16(dtype) and num_pos_feats == 128 and len(layers) == 2 and not torch.is_grad_enabled()
            and [(l.in_features, l.out_features) for l in layers] == [(512, 256), (256, 256)]
            and all(l.bias is not None and l.weight.is_cuda and l.weight.dtype == dtype and l.weight.stride(1) == 1
                    for l in layers))


def ref_point_head(reference_points: Tensor, valid_ratios: Tensor, layers, dtype: torch.dtype,
                   temperature: float = 10000.0):
    """``(reference_points_input [B,Nq,L,4] fp32, query_pos [B,Nq,256])`` of one decoder layer
    (salience_transformer.py:642-644) in one launch (include/salience_hip.h, ``sdetr_ref_point_head_bf16``)."""
    layers = list(layers)
    if not ref_point_head_applies(layers, dtype, 128):
        raise RuntimeError("ref_point_head: a 512 -> 256 -> 256 chain in a 16-bit type expected; no CPU fallback")
    _hip.require_device("ref_point_head", reference_points=reference_points, valid_ratios=valid_ratios)
    if reference_points.dim() != 3 or reference_points.shape[-1] != 4:
        raise RuntimeError("ref_point_head: [B,Nq,4] boxes expected")
    ref = reference_points.detach().float().contiguous()
    vr = valid_ratios.float().contiguous()
    B, Nq, _ = ref.shape
    L = vr.shape[1]
    p1, b1 = _packed_linear_512(layers[0].weight, layers[0].bias)
    p2, b2 = _packed_linear_bf16(layers[1].weight, layers[1].bias)
    pos = torch.empty((B, Nq, 256), dtype=dtype, device=ref.device)
    ref_in = torch.empty((B, Nq, L, 4), dtype=torch.float32, device=ref.device)
    _hip.launch("sdetr_ref_point_head_bf16", dtype, ref.device, ref.data_ptr(), vr.data_ptr(), B, Nq, L,
                float(temperature), p1.data_ptr(), b1.data_ptr(), p2.data_ptr(), b2.data_ptr(), pos.data_ptr(),
                ref_in.data_ptr(), what="ref_point_head")
    return ref_in, pos


def rows_linear_applies(x: Tensor, weight: Tensor, bias: Optional[Tensor]) -> bool:
    """``rows_linear`` takes this Linear on these rows: 16-bit HIP rows of 256 features, at most 768 outputs, no autograd."""
    return (x.is_cuda and _hip.is_act16(x.dtype) and x.shape[-1] == 256 and weight.dim() == 2 and weight.shape[1] == 256
            and weight.dtype == x.dtype and weight.stride(1) == 1 and 1 <= weight.shape[0] <= 768 and bias is not None
            and not torch.is_grad_enabled())


def rows_linear(x: Tensor, weight: Tensor, bias: Tensor, pos: Optional[Tensor] = None, pos_features: int = 0) -> Tensor:
    """``F.linear(x, weight, bias)`` where the first ``pos_features`` outputs see ``x + pos`` instead of ``x`` -- one launch
    for a few thousand rows (include/salience_hip.h, ``sdetr_rows_linear_bf16``)."""
    if not rows_linear_applies(x, weight, bias):
        raise RuntimeError("rows_linear: 16-bit HIP rows of 256 features and a Linear with at most 768 outputs expected; "
                           "no CPU fallback")
    N = weight.shape[0]
    xa = x if x.is_contiguous() else x.contiguous()
    pa = None
    if pos_features:
        if pos is None or pos.shape != x.shape or pos.dtype != x.dtype or pos.device != x.device:
            raise RuntimeError("rows_linear: pos must match x")
        pa = pos if pos.is_contiguous() else pos.contiguous()
    packed, b = _packed_linear_bf16(weight, bias)
    out = torch.empty(tuple(x.shape[:-1]) + (N,), dtype=x.dtype, device=x.device)
    _hip.launch("sdetr_rows_linear_bf16", x.dtype, x.device, xa.data_ptr(), _hip.ptr(pa), xa.numel() // 256,
                int(pos_features), packed.data_ptr(), b.data_ptr(), N, out.data_ptr(), N, what="rows_linear")
    return out


def _norm_f32(norm):
    """fp32 copies of a LayerNorm's weight and bias, cached on the weight tensor (refreshed when the parameters change)."""
    return derived(norm.weight, "norm_f32", (norm.weight, norm.bias),
                   lambda: (norm.weight.detach().float().contiguous(), norm.bias.detach().float().contiguous()))


def decoder_head_applies(query: Tensor, norm, class_head, bbox_layers) -> bool:
    """``decoder_head`` takes this layer head: 16-bit HIP queries of 256 features, an affine LayerNorm(256), a Linear class
    head with at most 224 classes and a 256 -> 256 -> 256 -> 4 bbox chain, parameters in the queries' type, no autograd."""
    layers = list(bbox_layers)
    if not (query.is_cuda and _hip.is_act16(query.dtype) and query.shape[-1] == 256 and not torch.is_grad_enabled()):
        return False
    if not (isinstance(norm, torch.nn.LayerNorm) and tuple(norm.normalized_shape) == (256,) and norm.weight is not None
            and norm.bias is not None):
        return False
    if not (class_head.in_features == 256 and 1 <= class_head.out_features <= 224 and class_head.bias is not None
            and class_head.weight.dtype == query.dtype and class_head.weight.stride(1) == 1):
        return False
    return (len(layers) == 3 and [(l.in_features, l.out_features) for l in layers] == [(256, 256), (256, 256), (256, 4)]
            and all(l.bias is not None and l.weight.dtype == query.dtype and l.weight.stride(1) == 1 for l in layers))


def decoder_head(query: Tensor, norm, class_head, bbox_layers, reference_points: Tensor, two_sources: bool,
                 eps: float = 1e-3):
    """A decoder layer's output head in one launch (include/salience_hip.h, ``sdetr_decoder_head_bf16``;
    models/bricks/salience_transformer.py:655-668): ``(logits [.., num_classes], boxes [1 | 2, .., 4] fp32)`` -- boxes[0]
    refined from the normed queries (the layer's output), boxes[1] from the raw queries (the next reference points)."""
    layers = list(bbox_layers)
    if not decoder_head_applies(query, norm, class_head, layers):
        raise RuntimeError("decoder_head: 16-bit HIP queries, LayerNorm(256), a Linear class head and a 256-256-256-4 bbox "
                           "chain expected; no CPU fallback")
    q = query if query.is_contiguous() else query.contiguous()
    rows = q.numel() // 256
    ref = reference_points.detach().float().contiguous()
    if ref.numel() != rows * 4:
        raise RuntimeError("decoder_head: reference_points must hold one (cx, cy, w, h) box per query row")
    _hip.require_device("decoder_head", reference_points=ref)
    g, b = _norm_f32(norm)
    pc, bc = _packed_linear_bf16(class_head.weight, class_head.bias)
    ops = [_packed_linear_bf16(l.weight, l.bias) for l in layers]
    lead = tuple(query.shape[:-1])
    ncls = class_head.out_features
    logits = torch.empty(lead + (ncls,), dtype=query.dtype, device=query.device)
    boxes = torch.empty(((2 if two_sources else 1),) + lead + (4,), dtype=torch.float32, device=query.device)
    _hip.launch("sdetr_decoder_head_bf16", query.dtype, query.device, q.data_ptr(), rows, g.data_ptr(), b.data_ptr(),
                float(norm.eps), pc.data_ptr(), bc.data_ptr(), ncls, ops[0][0].data_ptr(), ops[0][1].data_ptr(),
                ops[1][0].data_ptr(), ops[1][1].data_ptr(), ops[2][0].data_ptr(), ops[2][1].data_ptr(), ref.data_ptr(),
                float(eps), 1 if two_sources else 0, logits.data_ptr(), ncls, boxes.data_ptr(), what="decoder_head")
    return logits, boxes


def mlp_rows_applies(x: Tensor, layers) -> bool:
    """``mlp_rows`` takes this Linear + ReLU chain on these rows: 16-bit HIP rows, two layers 256|512 -> 256 -> 256 or
    three layers 256 -> 256 -> 256 -> n <= 32, parameters in the rows' type."""
    layers = list(layers)
    if not (x.is_cuda and _hip.is_act16(x.dtype) and len(layers) in (2, 3) and not torch.is_grad_enabled()):
        return False
    dims = [(l.in_features, l.out_features) for l in layers]
    if x.shape[-1] != dims[0][0] or dims[0][1] != 256 or dims[1] != (256, 256):
        return False
    if len(layers) == 2 and dims[0][0] not in (256, 512):
        return False
    if len(layers) == 3 and (dims[0][0] != 256 or dims[2][0] != 256 or not 1 <= dims[2][1] <= 32):
        return False
    return all(l.bias is not None and l.weight.dtype == x.dtype and l.weight.stride(1) == 1 and l.weight.is_cuda for l in layers)


def _packed_linear_512(weight: Tensor, bias: Tensor):
    """(two packed 256-column blocks back to back, fp32 bias) of a ``[256, 512]`` Linear for ``mlp_rows``; cached on the
    weight tensor like ``_packed_linear_bf16``."""
    def build():
        lib = _hip.lib(weight.dtype)
        w = weight.detach()
        half = lib.sdetr_linear_packed_bytes(256)
        with torch.no_grad(), torch.cuda.device(w.device):
            packed = torch.empty(2 * half, dtype=torch.uint8, device=w.device)
            for i in range(2):
                _hip.launch("sdetr_linear_pack_bf16", lib, w.device, w.data_ptr() + i * 256 * w.element_size(),
                            w.stride(0), 256, 256, packed.data_ptr() + i * half, what="linear_pack")
            return packed, bias.detach().float().contiguous()
    return derived(weight, "token_linear_512", (weight, bias), build)


def mlp_rows(x: Tensor, layers, x_second: Optional[Tensor] = None) -> Tensor:
    """``layers[-1](relu(... relu(layers[0](rows))))`` in one launch (include/salience_hip.h, ``sdetr_mlp_rows_bf16``;
    models/bricks/basic.py:6-26).  With ``x_second`` (same shape as ``x``) the rows are ``stack((x, x_second))`` and the
    result has that leading dimension of 2 -- without the stacked copy."""
    layers = list(layers)
    if not mlp_rows_applies(x, layers):
        raise RuntimeError("mlp_rows: 16-bit HIP rows and a 256|512 -> 256 -> 256 (-> n <= 32) Linear chain expected; "
                           "no CPU fallback")
    K = x.shape[-1]
    xa = x if x.is_contiguous() else x.contiguous()
    rows_a = xa.numel() // K
    rows, xb = rows_a, None
    if x_second is not None:
        if x_second.shape != x.shape or x_second.dtype != x.dtype or x_second.device != x.device:
            raise RuntimeError("mlp_rows: x_second must match x")
        xb = x_second if x_second.is_contiguous() else x_second.contiguous()
        rows = 2 * rows_a
    n_out = layers[-1].out_features
    lead = tuple(x.shape[:-1])
    out = torch.empty(((2,) + lead if xb is not None else lead) + (n_out,), dtype=x.dtype, device=x.device)
    ops = [(_packed_linear_512 if l.in_features == 512 else _packed_linear_bf16)(l.weight, l.bias) for l in layers]
    p3, b3 = ops[2] if len(layers) == 3 else (None, None)
    _hip.launch("sdetr_mlp_rows_bf16", x.dtype, x.device, xa.data_ptr(), _hip.ptr(xb), rows_a, rows, K,
                ops[0][0].data_ptr(), ops[0][1].data_ptr(), ops[1][0].data_ptr(), ops[1][1].data_ptr(), _hip.ptr(p3),
                _hip.ptr(b3), n_out, out.data_ptr(), n_out, what="mlp_rows")
    return out


def box_refine(delta: Tensor, reference_points: Tensor, eps: float = 1e-3) -> Tensor:
    """``sigmoid(delta + inverse_sigmoid(reference_points))`` (salience_transformer.py:659-660, 666-668) in one launch:
    ``delta`` ``[..., 4]`` (fp32 | bf16) whose leading dims are ``reference_points``' ``[B,Nq]`` or ``[G,B,Nq]``
    (G deltas refining the same boxes) -> fp32 of ``delta``'s shape."""
    _hip.require_device("box_refine", delta=delta, reference_points=reference_points)
    ref = reference_points.detach().float().contiguous()
    n = ref.numel() // 4
    if delta.shape[-1] != 4 or ref.shape[-1] != 4 or n == 0 or delta.numel() % (4 * n) != 0 \
            or delta.dtype not in (torch.float32,) + _hip.ACT16:
        raise RuntimeError("box_refine: delta [(G,)B,Nq,4] fp32 | bf16 against boxes [B,Nq,4] expected")
    d = delta.detach().contiguous()
    out = torch.empty(d.shape, dtype=torch.float32, device=d.device)
    _hip.launch("sdetr_box_refine", d.dtype, d.device, d.data_ptr(), _hip.dtype_code(d.dtype), 4, ref.data_ptr(), n,
                d.numel() // (4 * n), float(eps), out.data_ptr())
    return out


class LazyForegroundScore:
    """``foreground_score = masked_fill(flatten(salience maps), mask, min)`` (salience_transformer.py:164-168) NOT yet
    materialised: the flattened scores, the padding mask and the per-level minima.  The sorted-order encoder loop only
    reads the score of the rows it gathers, so ``encoder_prepare_sorted`` applies the fill to those rows on the fly (one
    launch less in the hot path); ``materialize()`` gives the ``[B,S]`` tensor of the reference (``masked_fill_min``)."""

    def __init__(self, score_flat: Tensor, mask: Tensor, level_min: Tensor):
        self.score_flat, self.mask, self.level_min = score_flat, mask, level_min
        self.dtype, self.shape, self.device = score_flat.dtype, score_flat.shape, score_flat.device
        self._full = None

    def is_contiguous(self) -> bool:
        return True

    def materialize(self) -> Tensor:
        if self._full is None:
            self._full = masked_fill_min(self.score_flat, self.mask, self.level_min)
        return self._full


# The encoder's entry gather also computes the first layer's class score (csrc/plumbing.hip, encoder_prepare_cls_kernel);
# False = the class head as a launch of its own (the form up to round 6, for A/B runs).
PREPARE_WITH_CLASS_SCORE = True


def _class_head_fragments(class_head):
    """``(packed fragments, fp32 bias padded to 96 with -inf)`` of a ``[<= 96, 256]`` 16-bit class head for the kernels that
    compute ``max_c(class_head(q))`` from an LDS tile (csrc/class_head_core.h); cached on the weight object."""
    w, b = class_head.weight, class_head.bias

    def build():
        lib = _hip.lib(w.dtype)
        with torch.no_grad(), torch.cuda.device(w.device):
            packed = torch.empty(lib.sdetr_class_head_packed_bytes(), dtype=torch.uint8, device=w.device)
            wc = w.detach().contiguous()
            _hip.launch("sdetr_class_head_pack_bf16", lib, w.device, wc.data_ptr(), wc.shape[0], 256, packed.data_ptr(),
                        what="class_head_pack")
            cb = torch.full((96,), float("-inf"), dtype=torch.float32, device=w.device)
            cb[:wc.shape[0]] = b.detach().float()
        return packed, cb
    return derived(w, "class_head_fragments", (w, b), build)


def prepare_class_score_applies(tokens: Tensor, score, class_head) -> bool:
    return (PREPARE_WITH_CLASS_SCORE and class_head is not None and score is not None and _hip.is_act16(tokens.dtype)
            and tokens.shape[-1] == 256 and class_head.weight.dtype == tokens.dtype and class_head.weight.dim() == 2
            and class_head.weight.shape[1] == 256 and class_head.weight.shape[0] <= 96 and class_head.bias is not None)


def encoder_prepare_sorted(tokens: Tensor, pos: Tensor, score, sorted_index: Tensor, valid_ratios: Tensor,
                           spatial_shapes: Tensor, level_start_index: Tensor, class_head=None):
    """Entry of the sorted-order encoder loop in one launch: ``(tokens[b, idx], pos[b, idx], score[b, idx],
    reference points of idx)`` for ``idx = sorted_index`` ``[B,n]`` -- the two row gathers of
    salience_transformer.py:454-461, the score gather and ``get_reference_points`` (:418-432) restricted to them.
    ``score``: fp32 ``[B,S]``, ``None``, or a ``LazyForegroundScore`` (the masked fill then happens in the gather).
    ``class_head`` (with ``prepare_class_score_applies``): a fifth result, the first layer's selection score
    ``class_head(rows).max(-1)[0] * score rows`` (salience_transformer.py:462, 366) out of the same launch."""
    with_cls = class_head is not None
    if with_cls and not prepare_class_score_applies(tokens, score, class_head):
        raise RuntimeError("encoder_prepare_sorted: the class score needs 16-bit [B,S,256] tokens, a score and a [<= 96, 256] head")
    score_mask = score_mins = None
    if isinstance(score, LazyForegroundScore):
        score_mask = score.mask.view(torch.uint8) if score.mask.dtype == torch.bool else score.mask
        score_mins = score.level_min
        score = score.score_flat
        if not (score_mask.is_contiguous() and tuple(score_mask.shape) == tuple(score.shape) and score_mins.dtype == torch.float32):
            raise RuntimeError("encoder_prepare_sorted: a lazy foreground score needs a contiguous [B,S] mask and fp32 minima")
    _hip.require_device("encoder_prepare_sorted", tokens=tokens, pos=pos, score=score, valid_ratios=valid_ratios,
                        score_mask=score_mask, score_mins=score_mins)
    if not sorted_index.is_cuda:
        raise RuntimeError("encoder_prepare_sorted: sorted_index must be a HIP (cuda) tensor; no CPU fallback")
    B, S, C = tokens.shape
    row_bytes = C * tokens.element_size()
    if (pos.shape != tokens.shape or pos.dtype != tokens.dtype or not tokens.is_contiguous() or not pos.is_contiguous()
            or sorted_index.dtype != torch.int64 or sorted_index.dim() != 2 or sorted_index.stride(1) != 1
            or row_bytes % 16 or 256 % (row_bytes // 16)):
        raise RuntimeError("encoder_prepare_sorted: contiguous [B,S,C] tokens / pos of one dtype and an int64 [B,n] index expected")
    n = sorted_index.shape[1]
    L = valid_ratios.shape[1]
    vr = valid_ratios.float().contiguous()
    q = torch.empty((B, n, C), dtype=tokens.dtype, device=tokens.device)
    ps = torch.empty_like(q)
    fg = None
    if score is not None:
        if score.dtype != torch.float32 or tuple(score.shape) != (B, S) or not score.is_contiguous():
            raise RuntimeError("encoder_prepare_sorted: fp32 contiguous [B,S] score expected")
        fg = torch.empty((B, n), dtype=torch.float32, device=tokens.device)
    ref = torch.empty((B, n, L, 2), dtype=torch.float32, device=tokens.device)
    args = (tokens.data_ptr(), pos.data_ptr(), row_bytes, _hip.ptr(score), sorted_index.data_ptr(),
            sorted_index.stride(0) if B > 1 else n, B, S, n, vr.data_ptr(), spatial_shapes.data_ptr(),
            level_start_index.data_ptr(), L, q.data_ptr(), ps.data_ptr(), _hip.ptr(fg), ref.data_ptr(),
            _hip.ptr(score_mask), _hip.ptr(score_mins), 0 if score_mins is None else score_mins.numel())
    if with_cls:
        packed, cb = _class_head_fragments(class_head)
        cls = torch.empty((B, n), dtype=torch.float32, device=tokens.device)
        _hip.launch("sdetr_encoder_prepare_sorted_scored", tokens.dtype, tokens.device, *args, packed.data_ptr(),
                    cb.data_ptr(), cls.data_ptr(), what="encoder_prepare_sorted")
        return q, ps, fg, ref, cls
    _hip.launch("sdetr_encoder_prepare_sorted", None, tokens.device, *args)
    return q, ps, fg, ref


def token_linear_ln(x: Tensor, linear, norm, residual: Tensor, scatter_index: Optional[Tensor] = None,
                    scatter_into: Optional[Tensor] = None) -> Tensor:
    """``norm(residual + linear(x))`` for a 256 -> 256 bf16 Linear in one launch (include/salience_hip.h (8));
    ``residual`` [B,n,256] may be a row range of a longer buffer.  With ``scatter_index`` [B,n] / ``scatter_into``
    [B,m,256] the rows are written to ``scatter_into[b, scatter_index[b,i]]`` (in place) instead."""
    if not token_linear_applies(x, linear.weight) or linear.out_features != 256 or x.dim() != 3:
        raise RuntimeError("token_linear_ln: bf16 [B,n,256] HIP tokens and a 256 -> 256 Linear expected")
    if not x.is_contiguous():
        x = x.contiguous()
    B, n, _ = x.shape
    if residual.dtype != x.dtype or tuple(residual.shape) != (B, n, 256):
        raise RuntimeError("token_linear_ln: residual must match x")
    packed, b = _packed_linear_bf16(linear.weight, linear.bias)
    g, be = _norm_f32(norm)
    out_rows = 0
    if scatter_index is not None:
        _hip.require_device("token_linear_ln", scatter_index=scatter_index, scatter_into=scatter_into)
        if (scatter_index.dtype != torch.int64 or tuple(scatter_index.shape) != (B, n) or scatter_into.dim() != 3
                or scatter_into.shape[0] != B or scatter_into.shape[2] != 256 or scatter_into.dtype != x.dtype):
            raise RuntimeError("token_linear_ln: scatter_index [B,n] int64 and scatter_into [B,m,256] of x's dtype expected")
        out, out_rows = scatter_into, scatter_into.shape[1]
    else:
        out = torch.empty((B, n, 256), dtype=x.dtype, device=x.device)
    _hip.launch("sdetr_token_linear_ln_bf16", x.dtype, x.device, x.data_ptr(), residual.data_ptr(),
                _batch_stride(residual, "token_linear_ln"), n, B * n, 256, packed.data_ptr(), b.data_ptr(),
                g.data_ptr(), be.data_ptr(), float(norm.eps), out.data_ptr(), _hip.ptr(scatter_index), out_rows,
                what="token_linear_ln")
    return out


def merge_sorted_desc(score: Tensor, payload: Tensor, segment_start, want_scores: bool = False):
    """Stable descending sort of ``score`` [B,n] = concatenation of descending-sorted segments starting at the
    columns ``segment_start`` (python ints, first 0), as a merge (include/salience_hip.h (4)).  Returns
    ``(sorted scores | None, payload in sorted order)``."""
    import ctypes
    _hip.require_device("merge_sorted_desc", score=score, payload=payload)
    if score.dtype != torch.float32 or payload.dtype != torch.int64 or payload.shape != score.shape or score.dim() != 2:
        raise RuntimeError("merge_sorted_desc: fp32 [B,n] scores and an int64 payload of the same shape expected")
    B, n = score.shape
    seg = (ctypes.c_int * len(segment_start))(*[int(v) for v in segment_start])
    out_index = torch.empty_like(payload)
    out_score = torch.empty_like(score) if want_scores else None
    _hip.launch("sdetr_merge_sorted_desc", None, score.device, score.data_ptr(), payload.data_ptr(), seg,
                len(segment_start), B, n, out_index.data_ptr(), _hip.ptr(out_score))
    return out_score, out_index


# ----------------------------------------------------------------------------------------------- row N3: the neck
def _token_map(what: str, name: str, t: Tensor, pixels: int, channels: int) -> int:
    """Checks a token-major feature map ``[B, pixels, >= channels]`` (a channel slice of a wider buffer is fine) and
    returns its row stride in elements."""
    if not t.is_cuda:
        raise RuntimeError(f"{what}: {name} must be a HIP (cuda) tensor; the neck has no CPU fallback")
    if t.dim() != 3 or t.shape[1] != pixels or t.shape[2] < channels or t.dtype not in (torch.float32,) + _hip.ACT16:
        raise RuntimeError(f"{what}: {name} must be [B, {pixels}, >= {channels}] fp32 | bf16 | fp16, got {tuple(t.shape)} {t.dtype}")
    ld = t.stride(1) if pixels > 1 else max(t.shape[2], t.stride(1))
    if t.stride(2) != 1 or (t.shape[0] > 1 and t.stride(0) != pixels * ld) or ld % 4 or t.data_ptr() % (4 * t.element_size()):
        raise RuntimeError(f"{what}: {name} rows must be dense in the channel dim, 4-element aligned, images back to back")
    return ld


def neck_pack_conv3x3(weight: Tensor, act: torch.dtype = torch.bfloat16) -> Optional[Tensor]:
    """16-bit MFMA operand fragments (in the activation type ``act``) of a ``[G, 3, 3, Ci, Co]`` fp32 kernel
    (``sdetr_neck_pack_conv3x3_bf16``), or None when the matrix-core kernel does not take the shape (it needs
    Ci % 16 == 0 and Co % 64 == 0)."""
    _hip.require_device("neck_pack_conv3x3", weight=weight)
    if weight.dim() != 5 or weight.shape[1:3] != (3, 3) or weight.dtype != torch.float32:
        raise RuntimeError("neck_pack_conv3x3: weight must be fp32 [groups, 3, 3, in_per_group, out_per_group]")
    G, _, _, ci, co = weight.shape
    lib = _hip.lib(act)
    nbytes = lib.sdetr_neck_conv3x3_packed_bytes(G, ci, co)
    if nbytes == 0:
        return None
    packed = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
    _hip.launch("sdetr_neck_pack_conv3x3_bf16", lib, weight.device, weight.data_ptr(), G, ci, co, packed.data_ptr(),
                what="neck_pack_conv3x3")
    return packed


def neck_conv3x3(x: Tensor, height: int, width: int, weight: Tensor, bias: Optional[Tensor], stride: int = 1,
                 activation: bool = False, packed: Optional[Tensor] = None) -> Tensor:
    """3x3 convolution (padding 1) + bias (+ SiLU) on a token-major map (include/salience_hip.h (13)): ``x``
    ``[B, height * width, >= G * Ci]``, ``weight`` fp32 ``[G, 3, 3, Ci, Co]`` (BatchNorm already folded in), ``bias``
    fp32 ``[G * Co]`` -> ``[B, Ho * Wo, G * Co]`` in ``x``'s dtype.  With ``packed`` (``neck_pack_conv3x3(weight)``)
    and a bf16 map the matrix-core kernel runs instead of the fp32 one."""
    _hip.require_device("neck_conv3x3", weight=weight, bias=bias)
    if weight.dim() != 5 or weight.shape[1:3] != (3, 3) or weight.dtype != torch.float32:
        raise RuntimeError("neck_conv3x3: weight must be fp32 [groups, 3, 3, in_per_group, out_per_group]")
    G, _, _, ci, co = weight.shape
    B = x.shape[0]
    ld = _token_map("neck_conv3x3", "x", x, height * width, G * ci)
    if bias is not None and (bias.dtype != torch.float32 or bias.numel() != G * co):
        raise RuntimeError("neck_conv3x3: bias must be fp32 [groups * out_per_group]")
    ho, wo = (height - 1) // stride + 1, (width - 1) // stride + 1
    out = torch.empty((B, ho * wo, G * co), dtype=x.dtype, device=x.device)
    if packed is not None and _hip.is_act16(x.dtype) and ld % 8 == 0 and x.data_ptr() % 16 == 0:
        _hip.require_device("neck_conv3x3", packed=packed)
        _hip.launch("sdetr_neck_conv3x3_mfma_bf16", x.dtype, x.device, x.data_ptr(), B, height, width, ld,
                    packed.data_ptr(), _hip.ptr(bias), G, ci, co, int(stride), int(bool(activation)), out.data_ptr(),
                    what="neck_conv3x3_mfma")
        return out
    _hip.launch("sdetr_neck_conv3x3", x.dtype, x.device, x.data_ptr(), _hip.dtype_code(x.dtype), B, height, width, ld,
                weight.data_ptr(), _hip.ptr(bias), G, ci, co, int(stride), int(bool(activation)), out.data_ptr())
    return out


def neck_combine(a: Tensor, height: int, width: int, up: Optional[Tensor] = None, up_hw=None,
                 bias: Optional[Tensor] = None, activation: bool = True) -> Tensor:
    """``act(a + nearest_upsample(up) + bias)`` on token-major maps: ``a`` ``[B, height * width, C]``, ``up``
    ``[B, up_hw[0] * up_hw[1], C]`` read at the source pixel of ``F.interpolate(mode="nearest")``."""
    B, _, C = a.shape
    lda = _token_map("neck_combine", "a", a, height * width, C)
    ldu, uh, uw = 0, 0, 0
    if up is not None:
        uh, uw = int(up_hw[0]), int(up_hw[1])
        if up.dtype != a.dtype or up.shape[0] != B or up.shape[2] != C:
            raise RuntimeError("neck_combine: `up` must have a's dtype, batch and channels")
        ldu = _token_map("neck_combine", "up", up, uh * uw, C)
    if bias is not None:
        _hip.require_device("neck_combine", bias=bias)
        if bias.dtype != torch.float32 or bias.numel() != C:
            raise RuntimeError("neck_combine: bias must be fp32 [C]")
    out = torch.empty((B, height * width, C), dtype=a.dtype, device=a.device)
    _hip.launch("sdetr_neck_combine", a.dtype, a.device, a.data_ptr(), lda, _hip.ptr(up), ldu, uh, uw, _hip.ptr(bias),
                _hip.dtype_code(a.dtype), B, height, width, C, int(bool(activation)), out.data_ptr(), C)
    return out


def neck_gate_shortcut(y: Tensor, mask_weight: Tensor, squeeze_weight: Tensor, excite_weight: Tensor, shortcut: Tensor,
                       shortcut2: Optional[Tensor] = None) -> Tensor:
    """``SqueezeAndExcitation(y) + shortcut (+ shortcut2)`` (models/bricks/basic.py:43-54, models/necks/repnet.py:63-64)
    on token-major maps: ``y`` contiguous ``[B, N, C]``; ``mask_weight`` fp32 ``[C]``, ``squeeze_weight`` ``[R, C]``,
    ``excite_weight`` ``[C, R]``; the shortcuts may be channel slices of wider buffers."""
    _hip.require_device("neck_gate_shortcut", y=y, mask_weight=mask_weight, squeeze_weight=squeeze_weight,
                        excite_weight=excite_weight)
    B, N, C = y.shape
    R = squeeze_weight.shape[0]
    if (mask_weight.numel() != C or tuple(squeeze_weight.shape) != (R, C) or tuple(excite_weight.shape) != (C, R)
            or any(w.dtype != torch.float32 for w in (mask_weight, squeeze_weight, excite_weight))):
        raise RuntimeError("neck_gate_shortcut: fp32 weights [C], [R, C], [C, R] expected")
    _token_map("neck_gate_shortcut", "y", y, N, C)
    ld1 = _token_map("neck_gate_shortcut", "shortcut", shortcut, N, C)
    ld2 = _token_map("neck_gate_shortcut", "shortcut2", shortcut2, N, C) if shortcut2 is not None else 0
    if shortcut.dtype != y.dtype or (shortcut2 is not None and shortcut2.dtype != y.dtype):
        raise RuntimeError("neck_gate_shortcut: the shortcuts must have y's dtype")
    lib = _hip.lib(y.dtype)
    ws_bytes = lib.sdetr_neck_gate_workspace_bytes(B, N, C)
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=y.device)
    gate = torch.empty((B, C), dtype=torch.float32, device=y.device)
    out = torch.empty_like(y)
    _hip.launch("sdetr_neck_gate_shortcut", lib, y.device, y.data_ptr(), _hip.dtype_code(y.dtype), B, N, C,
                mask_weight.data_ptr(), squeeze_weight.data_ptr(), excite_weight.data_ptr(), R, shortcut.data_ptr(),
                ld1, _hip.ptr(shortcut2), ld2, ws.data_ptr(), ws_bytes, gate.data_ptr(), out.data_ptr())
    return out


def topk_self_attention_applies(query: Tensor, pos: Tensor, mha, norm, num_selected: int) -> bool:
    """The two-launch top-k self-attention (csrc/topk_attention.hip) covers the released configuration: bf16,
    embed_dim 256, 8 heads, no dropout, batch-first parameters in bf16."""
    return (query.is_cuda and _hip.is_act16(query.dtype) and pos.dtype == query.dtype and query.dim() == 3
            and query.shape[-1] == 256 and mha.embed_dim == 256 and mha.num_heads == 8 and mha.in_proj_weight is not None
            and mha.in_proj_weight.dtype == query.dtype and mha.in_proj_bias is not None
            and mha.out_proj.bias is not None and norm.weight.dtype == query.dtype and norm.bias is not None
            and 0 < num_selected <= 384 and query.stride(2) == 1 and query.stride(1) == 256
            and pos.stride(2) == 1 and pos.stride(1) == 256)


# The layer's top-k selection and the in-projection of the selected rows in one launch (csrc/topk.hip,
# topk_hsort_inproj_kernel); False = selection launch + in-projection launch (the form up to round 6, for A/B runs).
SELECT_WITH_INPROJECTION = True


class SelectedInProjection:
    """``topk_select_inproj``'s result: ``selected`` int64 [B,k] and the in-projection of those rows (``workspace`` /
    ``hint`` as ``topk_self_attention_`` hands them to the attention launch)."""

    def __init__(self, selected, workspace, hint):
        self.selected, self.workspace, self.hint = selected, workspace, hint


def topk_select_inproj_applies(score: Tensor, k: int, query: Tensor, pos: Tensor, mha, norm) -> bool:
    """Shapes ``sdetr_topk_select_inproj_bf16`` covers: a contiguous fp32 [B,n] score row per image for the one-workgroup
    histogram sort (1024 <= n <= 17 408, 5 k <= 2 n) or its sliced form (longer rows: one launch more), 289 <= k <= 320
    (the attention launch that follows), the layer's queries contiguous."""
    if not SELECT_WITH_INPROJECTION or score.dim() != 2 or score.dtype != torch.float32 or not score.is_contiguous():
        return False
    B, n = score.shape
    if not (B > 0 and 289 <= k <= 320 and query.is_contiguous() and tuple(query.shape[:2]) == (B, n) and pos.shape[1] >= n
            and topk_self_attention_applies(query, pos, mha, norm, k)):
        return False
    if 1024 <= n <= 17408:
        return 5 * k <= 2 * n
    # longer rows: the sliced form (one launch more), where the library covers the shape
    return n > 17408 and _hip.lib(query.dtype).sdetr_topk_select_candidate_bytes(B, n, k) > 0


def topk_select_inproj(score: Tensor, k: int, query: Tensor, pos: Tensor, mha, orders_job=None) -> SelectedInProjection:
    """``torch.topk(score, k, dim=1)[1]`` (ties: lower position first; salience_transformer.py:366) and the in-projection
    of the rows it selects -- the first launch of ``topk_self_attention_`` -- in ONE launch; pass the result as
    ``topk_self_attention_(..., inprojection=result)``.  ``orders_job``: the pending ``RowOrdersJob`` rides along."""
    _hip.require_device("topk_select_inproj", score=score, query=query, pos=pos)
    B, n = score.shape
    lib = _hip.lib(query.dtype)
    dev = query.device
    sel = torch.empty((B, k), dtype=torch.int64, device=dev)
    ws = torch.empty(lib.sdetr_topk_attention_workspace_bytes(B, k), dtype=torch.uint8, device=dev)
    hint = torch.empty((B, n), dtype=torch.int32, device=dev)   # (uninitialised on purpose, see topk_self_attention_)
    job = orders_job if orders_job is not None and not orders_job.done and orders_job.device == dev else None
    cand_bytes = lib.sdetr_topk_select_candidate_bytes(B, n, k)      # (rows beyond one workgroup's sort: their slices' top-k)
    cand = torch.empty(cand_bytes, dtype=torch.uint8, device=dev) if cand_bytes else None
    _hip.launch("sdetr_topk_select_inproj_bf16", lib, dev, score.data_ptr(), B, n, k, sel.data_ptr(), query.data_ptr(),
                query.stride(0) if B > 1 else n * 256, pos.data_ptr(), pos.stride(0) if B > 1 else pos.shape[1] * 256,
                mha.in_proj_weight.data_ptr(), mha.in_proj_bias.data_ptr(), ws.data_ptr(), ws.numel(), hint.data_ptr(),
                hint.stride(0), None if job is None else ctypes.byref(job.struct), _hip.ptr(cand), cand_bytes,
                what="topk_select_inproj")
    if job is not None:
        job.done = True
    return SelectedInProjection(sel, ws, hint)


def topk_self_attention_(query: Tensor, pos: Tensor, selected: Tensor, mha, norm, projection=None,
                         inprojection: Optional[SelectedInProjection] = None):
    """In place on ``query`` [B,rows,256] bf16: rows ``selected[b]`` become
    ``norm(x + mha(q = k = x + pos, v = x))`` (salience_transformer.py:366-379); ``pos`` [B,>=rows,256] holds the position
    rows in the same row order (may be a row prefix of a longer buffer).  Two launches, no library GEMM.

    ``projection = (weight [384,256] bf16 head-major rows, bias)``: the deformable attention's offset | weight
    projection of the UPDATED queries (``token_linear(query, weight, bias, x_add=pos, group_features=48)``) rides in the
    attention's launch (``sdetr_topk_attention_with_projection_bf16``) and is returned as ``[B,8,rows,48]``; ``None`` is
    returned in its place when that launch does not cover the shape (the caller projects afterwards).
    ``inprojection``: ``topk_select_inproj``'s result for this ``selected`` (the carried form only): its launch has done
    the in-projection."""
    _hip.require_device("topk_self_attention_", selected=selected)
    B, rows, _ = query.shape
    N = selected.shape[1]
    if not topk_self_attention_applies(query, pos, mha, norm, N) or selected.dtype != torch.int64 or selected.shape[0] != B:
        raise RuntimeError("topk_self_attention_: bf16 [B,rows,256] HIP tensors, 8 heads, int64 [B,N] selection expected; "
                           "no CPU fallback")
    lib = _hip.lib(query.dtype)
    if inprojection is not None and inprojection.selected is not selected:
        raise RuntimeError("topk_self_attention_: the in-projection belongs to another selection")
    ws = (inprojection.workspace if inprojection is not None
          else torch.empty(lib.sdetr_topk_attention_workspace_bytes(B, N), dtype=torch.uint8, device=query.device))
    qbs = query.stride(0) if B > 1 else rows * 256
    pbs = pos.stride(0) if B > 1 else pos.shape[1] * 256
    carried = (projection is not None and 289 <= N <= 320 and query.is_contiguous()
               and token_linear_applies(query, projection[0]) and tuple(projection[0].shape) == (384, 256)
               and projection[0].is_contiguous())
    if carried:
        w, b = projection
        packed, b_pad = _packed_linear_bf16(w, b)
        slab = torch.empty((B, 8, rows, 48), dtype=query.dtype, device=query.device)
        # marks of the selected rows for the projection part of the launch: UNINITIALISED on purpose -- a mark m
        # counts only if selected[b][m - 1] is the row it sits on, which no garbage value can fake, and the
        # in-projection writes the true marks before anything reads them
        hint = inprojection.hint if inprojection is not None else torch.empty((B, rows), dtype=torch.int32, device=query.device)
        _hip.launch("sdetr_topk_attention_with_projection_bf16", lib, query.device, query.data_ptr(), qbs,
                    pos.data_ptr(), pbs, selected.data_ptr(), B, rows, N, mha.in_proj_weight.data_ptr(),
                    mha.in_proj_bias.data_ptr(), mha.out_proj.weight.data_ptr(), mha.out_proj.bias.data_ptr(),
                    norm.weight.data_ptr(), norm.bias.data_ptr(), float(norm.eps), ws.data_ptr(), ws.numel(),
                    w.data_ptr(), packed.data_ptr(), b_pad.data_ptr(), slab.data_ptr(), hint.data_ptr(),
                    hint.stride(0),
                    _fragment_order(mha.out_proj.weight, 32).data_ptr() if mha.out_proj.weight.is_contiguous() else None,
                    _fragment_order(w, 48).data_ptr(), 1 if inprojection is not None else 0,
                    what="topk_self_attention_")
        return slab
    if inprojection is not None:
        raise RuntimeError("topk_self_attention_: an in-projection from the selection's launch needs the carried form")
    _hip.launch("sdetr_topk_attention_bf16", lib, query.device, query.data_ptr(), qbs, pos.data_ptr(), pbs,
                selected.data_ptr(), B, rows, N, mha.in_proj_weight.data_ptr(), mha.in_proj_bias.data_ptr(),
                mha.out_proj.weight.data_ptr(), mha.out_proj.bias.data_ptr(), norm.weight.data_ptr(),
                norm.bias.data_ptr(), float(norm.eps), 256, 8, ws.data_ptr(), ws.numel(), what="topk_self_attention_")
    return None if projection is not None else query
