"""Detection post-processing (reference models/bricks/post_process.py:PostProcess) as one HIP launch.

``SalienceDETR.forward`` in eval mode ends in ``PostProcess(select_box_nums_for_evaluation=300)`` on the last decoder
layer's ``pred_logits`` / ``pred_boxes`` (models/detectors/salience_detr.py:241-243).  The reference needs torchvision for
the box conversion and the NMS; this module does not.  ``sdetr_detection_postprocess`` (csrc/post_process.hip) selects the
top K of every image's ``Nq * C`` entries by logit (ties to the lower flat index), computes the scores, labels and pixel
boxes, applies the optional confidence / NMS filters and compacts the kept entries, all in one launch per batch.

``detections_padded`` returns fixed-shape device tensors without a host sync (graph capture, ``GraphLanes`` serving);
``PostProcess`` returns the reference's list of per-image dicts.  No CPU fallback.
"""
from typing import Dict, List, Tuple

import numpy as np
import torch
from torch import nn

from . import _hip

MAX_K = 1024


def _round_down_f32(x: float) -> float:
    """Largest float32 <= x: for a float32 value v, ``v > x`` (the double compare torchvision's NMS makes between its
    fp32 IoU and the Python threshold) equals ``v > _round_down_f32(x)``.  Round-to-nearest would differ where float32(x)
    rounds up, e.g. 0.6: an IoU of exactly float32(0.6) (= 3/5 in fp32) is > 0.6 in double and suppresses."""
    f = float(np.float32(x))
    if f > x:
        f = float(np.nextafter(np.float32(f), np.float32(-np.inf)))
    return f


def detections_padded(pred_logits: torch.Tensor, pred_boxes: torch.Tensor, target_sizes: torch.Tensor, k: int,
                      confidence_score: float = -1, nms_iou_threshold: float = -1
                      ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(scores [B, k] in the logits' dtype, labels int64 [B, k], boxes fp32 [B, k, 4] in pixels (x1, y1, x2, y2),
    count int32 [B]).  Entries [0, count) of an image are the kept detections in rank order; the rest are padding
    (score 0, label -1, box 0).  No host sync: can be captured in a graph.

    pred_logits [B, Nq, C] fp32 / bf16 / fp16 (rows contiguous; the batch stride may be larger, as the query slice
    ``dn_post_process`` leaves); pred_boxes fp32 [B, Nq, 4] (cx, cy, w, h) normalised; target_sizes [B, 2] (h, w),
    int64 or fp32.  Filters as in the reference: ``confidence_score > 0`` keeps ``score > confidence_score`` compared in
    the score's dtype; ``nms_iou_threshold > 0`` runs greedy class-agnostic NMS over all k selected boxes (an entry
    must pass both; NMS without a confidence filter is NMS alone, where the reference fails)."""
    what = "detections_padded"
    for name, t in (("pred_logits", pred_logits), ("pred_boxes", pred_boxes), ("target_sizes", target_sizes)):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{what}: {name} must be a tensor")
    if pred_boxes.dtype != torch.float32:
        raise RuntimeError(f"{what}: pred_boxes must be float32 (got {pred_boxes.dtype}); box_refine / decoder_head "
                           "produce fp32 boxes")
    for name, t in (("pred_logits", pred_logits), ("pred_boxes", pred_boxes), ("target_sizes", target_sizes)):
        if not t.is_cuda:
            raise RuntimeError(f"{what}: {name} must be a HIP (cuda) tensor; there is no CPU fallback")
    if pred_logits.dim() != 3:
        raise RuntimeError(f"{what}: pred_logits must be [B, Nq, C], got {tuple(pred_logits.shape)}")
    B, Nq, C = pred_logits.shape
    if pred_logits.dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise RuntimeError(f"{what}: pred_logits dtype {pred_logits.dtype} (float32 / bfloat16 / float16)")
    if tuple(pred_boxes.shape) != (B, Nq, 4):
        raise RuntimeError(f"{what}: pred_boxes must be [B, Nq, 4] = {(B, Nq, 4)}, got {tuple(pred_boxes.shape)}")
    if tuple(target_sizes.shape) != (B, 2):
        raise RuntimeError(f"{what}: target_sizes must be [B, 2] (h, w), got {tuple(target_sizes.shape)}")
    if target_sizes.dtype not in (torch.int64, torch.float32):
        raise RuntimeError(f"{what}: target_sizes dtype {target_sizes.dtype} (int64 / float32)")
    if B == 0:
        raise RuntimeError(f"{what}: empty batch")
    # rows contiguous, images any stride apart (a [:, pad:, :] query slice is fine)
    if pred_logits.stride(2) != 1 or pred_logits.stride(1) != C:
        pred_logits = pred_logits.contiguous()
    logits_stride = pred_logits.stride(0) if B > 1 else Nq * C
    if pred_boxes.stride(2) != 1 or pred_boxes.stride(1) != 4:
        pred_boxes = pred_boxes.contiguous()
    boxes_stride = pred_boxes.stride(0) if B > 1 else Nq * 4
    target_sizes = target_sizes.contiguous()
    dev = pred_logits.device
    scores = torch.empty((B, k), dtype=pred_logits.dtype, device=dev)
    labels = torch.empty((B, k), dtype=torch.int64, device=dev)
    boxes = torch.empty((B, k, 4), dtype=torch.float32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    # thresholds: the score's compare happens in its dtype (torch rounds the Python float to it: no double rounding
    # through fp32); torchvision compares the fp32 IoU with the double threshold
    thr = float(torch.tensor(confidence_score, dtype=torch.float64).to(pred_logits.dtype).float()) \
        if confidence_score > 0 else -1.0
    # (a threshold below FLT_MIN = 1.2e-38 is raised to FLT_MIN: the kernel reads a threshold <= 0 as "no NMS", and the
    # equivalence above then fails only for IoUs in (threshold, FLT_MIN], denormal quotients no box pair produces)
    iou = _round_down_f32(float(nms_iou_threshold)) if nms_iou_threshold > 0 else -1.0
    if nms_iou_threshold > 0 and iou < float(np.finfo(np.float32).tiny):
        iou = float(np.finfo(np.float32).tiny)
    L = _hip.lib(pred_logits.dtype)
    _hip.launch("sdetr_detection_postprocess", L, dev, pred_logits.data_ptr(), _hip.dtype_code(pred_logits.dtype),
                logits_stride, pred_boxes.data_ptr(), boxes_stride, target_sizes.data_ptr(),
                _hip.I64 if target_sizes.dtype == torch.int64 else _hip.F32, B, Nq, C, int(k), thr, iou,
                scores.data_ptr(), labels.data_ptr(), boxes.data_ptr(), count.data_ptr())
    return scores, labels, boxes, count


class PostProcess(nn.Module):
    """Drop-in for the reference's ``models.bricks.post_process.PostProcess`` (same constructor, same ``forward``,
    same output), one HIP launch per batch.  Ranking is by logit with ties to the lower flat index -- one of the orders
    ``torch.topk(prob)`` may return, and a deterministic one."""

    def __init__(self, select_box_nums_for_evaluation=100, nms_iou_threshold=-1, confidence_score=-1):
        super().__init__()
        self.select_box_nums_for_evaluation = select_box_nums_for_evaluation
        self.nms_iou_threshold = nms_iou_threshold
        self.confidence_score = confidence_score

    @torch.no_grad()
    def forward(self, outputs: Dict[str, torch.Tensor], target_sizes: torch.Tensor) -> List[Dict[str, torch.Tensor]]:
        out_logits, out_bbox = outputs["pred_logits"], outputs["pred_boxes"]
        assert len(out_logits) == len(target_sizes)
        assert target_sizes.shape[1] == 2
        scores, labels, boxes, count = detections_padded(out_logits, out_bbox, target_sizes,
                                                         self.select_box_nums_for_evaluation, self.confidence_score,
                                                         self.nms_iou_threshold)
        if self.confidence_score > 0 or self.nms_iou_threshold > 0:
            counts = count.cpu().tolist()          # the one device-to-host copy
            return [{"scores": scores[i, :c], "labels": labels[i, :c], "boxes": boxes[i, :c]}
                    for i, c in enumerate(counts)]
        return [{"scores": s, "labels": l, "boxes": b} for s, l, b in zip(scores, labels, boxes)]
