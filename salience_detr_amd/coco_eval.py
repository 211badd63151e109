"""COCO box evaluation (reference util/engine.py:evaluate_acc -> util/coco_eval.py:CocoEvaluator -> pycocotools COCOeval,
``iouType="bbox"``, default parameters) without pycocotools.

``CocoBoxEvaluator.update`` takes what ``detections_padded`` / ``PostProcess`` return and the targets of the batch and
runs ``sdetr_coco_eval_update`` (csrc/coco_eval.hip): one launch per batch does the per-category ranking, the cap at
100, the float64 IoUs and the greedy matching at 10 thresholds x 4 area ranges, and leaves fixed-size records on the
device -- no host sync, no copy of the detections to the host.  ``accumulate`` sorts the records (two stable
``torch.sort``) and runs ``sdetr_coco_eval_accumulate``: one workgroup per (category, area range, maxDet) fills
pycocotools' ``precision`` / ``recall`` / ``scores`` arrays.  ``summarize`` gives the 12 stats.

Records are rows of int64 words (include/salience_hip.h):
    detection   image id | category index + rank << 32 | score (bits of a double) | matched bits | ignored bits
    ground truth, per (image, category)   image id | category index | non-ignored ground truths in the 4 area ranges |
                ground truths (crowds included)
bit ``area * 10 + threshold``.  Scores are compared as float32 (what the detector produces; a float64 score is rounded
to float32 first).  An empty intersection is IoU 0, also between two empty boxes.

CPU tensors take a plain-torch composite of the same semantics (``_composite_update`` / ``_composite_accumulate``).
"""
from typing import Dict, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _hip

T, R, A, M = 10, 101, 4, 3
IOU_THRESHOLDS = np.linspace(0.5, 0.95, T)
RECALL_THRESHOLDS = np.linspace(0.0, 1.0, R)
MAX_DETS = (1, 10, 100)
AREA_LO = (0.0, 0.0, 1024.0, 9216.0)
AREA_HI = (1e10, 1024.0, 9216.0, 1e10)
AREA_NAMES = ("all", "small", "medium", "large")
DET_WORDS, GT_WORDS = 5, 7
GT_CAPACITY = 128             # ground truths per (image, category) in the HIP form (SDETR_COCO_GT_CAP)
MAX_CATEGORIES = 2048         # SDETR_COCO_MAX_CATEGORIES
MAX_PER_IMAGE = 1024          # detections / ground truths per image (SDETR_COCO_MAX_DET_PER_IMAGE, .._GT_PER_IMAGE)
METRIC_NAMES = ("mAP", "AP@50", "AP@75", "AP-s", "AP-m", "AP-l", "AR_1", "AR_10", "AR_100", "AR-s", "AR-m", "AR-l")

Detections = Union[Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor], Sequence[Dict[str, torch.Tensor]]]


def _categories_of(labels: torch.Tensor, lut: torch.Tensor) -> torch.Tensor:
    labels = labels.long()
    ok = (labels >= 0) & (labels < lut.numel())
    return torch.where(ok, lut[labels.clamp(0, lut.numel() - 1)].long(), torch.full_like(labels, -1))


def pad_detections(detections: Sequence[Dict[str, torch.Tensor]]):
    """``PostProcess``'s list of dicts -> the 4-tuple of ``detections_padded`` (scores float32)."""
    lens = [int(d["scores"].shape[0]) for d in detections]
    B, k = len(detections), max(lens + [1])
    dev = detections[0]["scores"].device
    scores = torch.zeros((B, k), dtype=torch.float32, device=dev)
    labels = torch.full((B, k), -1, dtype=torch.int64, device=dev)
    boxes = torch.zeros((B, k, 4), dtype=torch.float32, device=dev)
    for i, d in enumerate(detections):
        scores[i, :lens[i]] = d["scores"].float()
        labels[i, :lens[i]] = d["labels"].long()
        boxes[i, :lens[i]] = d["boxes"].float()
    return scores, labels, boxes, torch.tensor(lens, dtype=torch.int32).to(dev)


def pad_targets(targets: Sequence[Dict], device) -> Tuple[torch.Tensor, ...]:
    """(boxes fp32 [B, G, 4], labels int64 [B, G], area f64 [B, G], iscrowd uint8 [B, G], count int32 [B], image id
    int64 [B]) on ``device``, built where the targets live and moved once.  Raises above the HIP form's capacity."""
    B = len(targets)
    lens = [int(t["boxes"].shape[0]) for t in targets]
    G = max(lens + [1])
    src = targets[0]["boxes"].device
    boxes = torch.zeros((B, G, 4), dtype=torch.float32, device=src)
    labels = torch.full((B, G), -1, dtype=torch.int64, device=src)
    area = torch.zeros((B, G), dtype=torch.float64, device=src)
    crowd = torch.zeros((B, G), dtype=torch.uint8, device=src)
    for i, t in enumerate(targets):
        n = lens[i]
        if n == 0:
            continue
        bx = t["boxes"].float().reshape(n, 4)
        boxes[i, :n] = bx
        labels[i, :n] = t["labels"].long()
        if t.get("area") is not None:
            area[i, :n] = t["area"].double()
        else:
            bd = bx.double()
            area[i, :n] = (bd[:, 2] - bd[:, 0]) * (bd[:, 3] - bd[:, 1])
        if t.get("iscrowd") is not None:
            crowd[i, :n] = t["iscrowd"].to(torch.uint8)
        if n > GT_CAPACITY and int(torch.unique(t["labels"], return_counts=True)[1].max()) > GT_CAPACITY:
            raise RuntimeError(f"CocoBoxEvaluator: image {int(t['image_id'])} has more than {GT_CAPACITY} ground truths "
                               "of one category (the capacity of the HIP form)")
    ids = torch.tensor([int(t["image_id"]) for t in targets], dtype=torch.int64)
    count = torch.tensor(lens, dtype=torch.int32)
    return tuple(x.to(device) for x in (boxes, labels, area, crowd, count, ids))


def hip_update(scores, labels, boxes, count, gt_boxes, gt_labels, gt_area, gt_crowd, gt_count, image_ids, lut,
               num_categories: int, iou_thresholds, out=None):
    """One ``sdetr_coco_eval_update`` launch; returns (detection records int64 [B * k, 5], ground-truth records int64
    [B * G, 7], totals int32 [2]), every element written.  ``out``: three such tensors to write into."""
    B, k = scores.shape
    G = gt_labels.shape[1]
    dev = scores.device
    tensors = dict(scores=scores, labels=labels, boxes=boxes, count=count, gt_boxes=gt_boxes, gt_labels=gt_labels,
                   gt_area=gt_area, gt_crowd=gt_crowd, gt_count=gt_count, image_ids=image_ids, category_lut=lut,
                   iou_thresholds=iou_thresholds)
    _hip.require_device("coco_eval_update", **tensors)
    want = dict(scores=torch.float32, labels=torch.int64, boxes=torch.float32, count=torch.int32, gt_boxes=torch.float32,
                gt_labels=torch.int64, gt_area=torch.float64, gt_crowd=torch.uint8, gt_count=torch.int32,
                image_ids=torch.int64, category_lut=torch.int32, iou_thresholds=torch.float64)
    for name, t in tensors.items():
        if t.dtype != want[name]:
            raise RuntimeError(f"coco_eval_update: {name} must be {want[name]}, got {t.dtype}")
    if tuple(labels.shape) != (B, k) or tuple(boxes.shape) != (B, k, 4) or tuple(count.shape) != (B,):
        raise RuntimeError("coco_eval_update: detections must be scores [B, k], labels [B, k], boxes [B, k, 4], count [B]")
    if (tuple(gt_boxes.shape) != (B, G, 4) or tuple(gt_area.shape) != (B, G) or tuple(gt_crowd.shape) != (B, G)
            or tuple(gt_count.shape) != (B,) or tuple(image_ids.shape) != (B,) or iou_thresholds.numel() != T):
        raise RuntimeError("coco_eval_update: targets must be padded to [B, G] with one count and one image id per image")
    if out is None:
        out = (torch.empty((B * k, DET_WORDS), dtype=torch.int64, device=dev),
               torch.empty((B * G, GT_WORDS), dtype=torch.int64, device=dev),
               torch.empty((2,), dtype=torch.int32, device=dev))
    det, gt, totals = out
    _hip.launch("sdetr_coco_eval_update", None, dev, scores.data_ptr(), labels.data_ptr(), boxes.data_ptr(),
                count.data_ptr(), B, k, gt_boxes.data_ptr(), gt_labels.data_ptr(), gt_area.data_ptr(), gt_crowd.data_ptr(),
                gt_count.data_ptr(), image_ids.data_ptr(), G, lut.data_ptr(), lut.numel(), int(num_categories),
                iou_thresholds.data_ptr(), det.data_ptr(), gt.data_ptr(), totals.data_ptr())
    return det, gt, totals


def _composite_update(scores, labels, boxes, count, gt_boxes, gt_labels, gt_area, gt_crowd, gt_count, image_ids, lut,
                      num_categories, iou_thresholds):
    """The update in plain torch: the 40 (area range, threshold) walks of an (image, category) advance together as
    [4, 10] tensors.  Returns exactly the real rows (detection records, ground-truth records)."""
    dev = scores.device
    lo = torch.tensor(AREA_LO, dtype=torch.float64, device=dev)[:, None]
    hi = torch.tensor(AREA_HI, dtype=torch.float64, device=dev)[:, None]
    best0 = torch.minimum(iou_thresholds.double(), torch.tensor(1 - 1e-10, dtype=torch.float64, device=dev))
    weight = (torch.ones((), dtype=torch.int64, device=dev) << torch.arange(A * T, device=dev)).view(A, T)
    lanes = torch.arange(A, device=dev)
    det_rows, gt_rows = [], []
    for b in range(scores.shape[0]):
        n, g = int(count[b]), int(gt_count[b])
        image = image_ids[b].long()
        cat = _categories_of(labels[b, :n], lut)
        keep = cat >= 0
        cat, sc, bx = cat[keep], scores[b, :n][keep].float(), boxes[b, :n][keep].double()
        order = torch.sort(sc, descending=True, stable=True).indices
        order = order[torch.sort(cat[order], stable=True).indices]
        cat, sc, bx = cat[order], sc[order], bx[order]
        rank = torch.arange(cat.numel(), device=dev) - torch.searchsorted(cat, cat)
        keep = rank < MAX_DETS[-1]
        cat, sc, bx, rank = cat[keep], sc[keep], bx[keep], rank[keep]
        gcat = _categories_of(gt_labels[b, :g], lut)
        gkeep = gcat >= 0
        gcat, gbx = gcat[gkeep], gt_boxes[b, :g][gkeep].double()
        gar, gcr = gt_area[b, :g][gkeep].double(), gt_crowd[b, :g][gkeep].bool()
        darea = (bx[:, 2] - bx[:, 0]) * (bx[:, 3] - bx[:, 1])
        for c in torch.unique(torch.cat([cat, gcat])).tolist():
            di, gi = (cat == c).nonzero()[:, 0], (gcat == c).nonzero()[:, 0]
            D, G = di.numel(), gi.numel()
            d_box, g_box, crowd = bx[di], gbx[gi], gcr[gi]
            ignore = crowd[None] | (gar[gi][None] < lo) | (gar[gi][None] > hi)                       # [4, G]
            if G:
                gt_rows.append(torch.cat([image.view(1), torch.tensor([c], device=dev), (~ignore).sum(1),
                                          torch.tensor([G], device=dev)]))
            if not D:
                continue
            iw = torch.minimum(d_box[:, None, 2], g_box[None, :, 2]) - torch.maximum(d_box[:, None, 0], g_box[None, :, 0])
            ih = torch.minimum(d_box[:, None, 3], g_box[None, :, 3]) - torch.maximum(d_box[:, None, 1], g_box[None, :, 1])
            inter = iw * ih
            g_area = (g_box[:, 2] - g_box[:, 0]) * (g_box[:, 3] - g_box[:, 1])
            union = torch.where(crowd[None], darea[di][:, None].expand(D, G), darea[di][:, None] + g_area[None] - inter)
            hit = (iw > 0) & (ih > 0)
            iou = torch.where(hit, inter / torch.where(hit, union, torch.ones_like(union)), torch.zeros_like(inter))
            perm = torch.sort(ignore.to(torch.int8), dim=1, stable=True).indices                      # [4, G]
            outside = (darea[di][None] < lo) | (darea[di][None] > hi)                                 # [4, D]
            taken = torch.zeros((A, T, G), dtype=torch.bool, device=dev)
            matched_bits = torch.zeros(D, dtype=torch.int64, device=dev)
            ignored_bits = torch.zeros(D, dtype=torch.int64, device=dev)
            for d in range(D):
                best = best0[None].expand(A, T).clone()
                m = torch.full((A, T), -1, dtype=torch.int64, device=dev)
                m_ign = torch.zeros((A, T), dtype=torch.bool, device=dev)
                stopped = torch.zeros((A, T), dtype=torch.bool, device=dev)
                for i in range(G):
                    gidx = perm[:, i]                                                                 # [4]
                    g_ign = ignore[lanes, gidx][:, None]
                    skip = taken[lanes, :, gidx] & ~crowd[gidx][:, None]
                    stopped = stopped | ((m >= 0) & ~m_ign & g_ign & ~skip)
                    value = iou[d, gidx][:, None]
                    take = ~skip & ~stopped & ~(value < best)
                    best = torch.where(take, value, best)
                    m = torch.where(take, gidx[:, None], m)
                    m_ign = torch.where(take, g_ign, m_ign)
                matched = m >= 0
                if G:
                    taken |= torch.zeros_like(taken).scatter_(2, m.clamp(min=0)[..., None], matched[..., None])
                ignored = torch.where(matched, m_ign, outside[:, d][:, None].expand(A, T))
                matched_bits[d] = (matched.long() * weight).sum()
                ignored_bits[d] = (ignored.long() * weight).sum()
            det_rows.append(torch.stack([image.expand(D), cat[di] | (rank[di] << 32), sc[di].double().view(torch.int64),
                                         matched_bits, ignored_bits], 1))
    det = torch.cat(det_rows) if det_rows else torch.zeros((0, DET_WORDS), dtype=torch.int64, device=dev)
    gt = torch.stack(gt_rows) if gt_rows else torch.zeros((0, GT_WORDS), dtype=torch.int64, device=dev)
    return det, gt


def sort_records(det: torch.Tensor) -> torch.Tensor:
    """The accumulate order: category, then descending score, ties by ascending image id, then rank.  Two stable sorts:
    by image id, then by one int64 key (category << 32 | order-reversing map of the float32 score)."""
    det = det[torch.sort(det[:, 0], stable=True).indices]
    score = det[:, 2].contiguous().view(torch.float64).float() + 0.0
    bits = score.view(torch.int32).long() & 0xFFFFFFFF
    ascending = torch.where(bits >= 0x80000000, bits ^ 0xFFFFFFFF, bits | 0x80000000)
    key = ((det[:, 1] & 0xFFFFFFFF) << 32) | (0xFFFFFFFF - ascending)
    return det[torch.sort(key, stable=True).indices].contiguous()


def hip_accumulate(det, category_first, npig, num_categories: int, recall_thresholds):
    """One ``sdetr_coco_eval_accumulate`` launch over sorted records; (precision, recall, scores) float64 on the device."""
    _hip.require_device("coco_eval_accumulate", records=det, category_first=category_first, npig=npig,
                        recall_thresholds=recall_thresholds)
    if det.dtype != torch.int64 or det.dim() != 2 or det.shape[1] != DET_WORDS:
        raise RuntimeError(f"coco_eval_accumulate: records must be int64 [N, {DET_WORDS}]")
    K, dev = int(num_categories), det.device
    if category_first.dtype != torch.int64 or category_first.numel() != K + 1 or npig.dtype != torch.int64 \
            or tuple(npig.shape) != (K, A) or recall_thresholds.dtype != torch.float64 or recall_thresholds.numel() != R:
        raise RuntimeError("coco_eval_accumulate: category_first int64 [K + 1], npig int64 [K, 4], recall thresholds f64 [101]")
    precision = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
    recall = torch.empty((T, K, A, M), dtype=torch.float64, device=dev)
    scores = torch.empty((T, R, K, A, M), dtype=torch.float64, device=dev)
    _hip.launch("sdetr_coco_eval_accumulate", None, dev, det.data_ptr(), det.shape[0], category_first.data_ptr(),
                npig.data_ptr(), K, recall_thresholds.data_ptr(), precision.data_ptr(), recall.data_ptr(), scores.data_ptr())
    return precision, recall, scores


def _composite_accumulate(det, category_first, npig, num_categories, recall_thresholds):
    dev, K = det.device, int(num_categories)
    precision = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64, device=dev)
    recall = torch.full((T, K, A, M), -1.0, dtype=torch.float64, device=dev)
    scores = torch.full((T, R, K, A, M), -1.0, dtype=torch.float64, device=dev)
    first = category_first.tolist()
    shifts = torch.arange(T, device=dev)[:, None]
    eps = float(np.spacing(1))
    for k in range(K):
        seg = det[first[k]:first[k + 1]]
        rank, sc = seg[:, 1] >> 32, seg[:, 2].contiguous().view(torch.float64)
        for a in range(A):
            n_gt = int(npig[k, a])
            if n_gt == 0:
                continue
            matched = ((seg[:, 3][None] >> (a * T + shifts)) & 1).bool()
            ignored = ((seg[:, 4][None] >> (a * T + shifts)) & 1).bool()
            for m, max_det in enumerate(MAX_DETS):
                sel = rank < max_det
                n = int(sel.sum())
                precision[:, :, k, a, m] = 0.0
                scores[:, :, k, a, m] = 0.0
                recall[:, k, a, m] = 0.0
                if n == 0:
                    continue
                tp = (matched & ~ignored)[:, sel].double().cumsum(1)
                fp = (~matched & ~ignored)[:, sel].double().cumsum(1)
                rc = tp / n_gt
                pr = tp / (fp + tp + eps)
                recall[:, k, a, m] = rc[:, -1]
                envelope = torch.cummax(pr.flip(1), 1).values.flip(1)
                idx = torch.searchsorted(rc.contiguous(), recall_thresholds[None].expand(T, R).contiguous(), right=False)
                inside = idx < n
                idx = idx.clamp(max=n - 1)
                precision[:, :, k, a, m] = torch.where(inside, envelope.gather(1, idx), torch.zeros_like(idx, dtype=torch.float64))
                scores[:, :, k, a, m] = torch.where(inside, sc[sel][idx], torch.zeros_like(idx, dtype=torch.float64))
    return precision, recall, scores


def summarize_stats(precision: torch.Tensor, recall: torch.Tensor) -> torch.Tensor:
    """pycocotools' 12 stats from its ``precision`` [T, R, K, A, M] and ``recall`` [T, K, A, M]."""
    def mean(s):
        s = s[s > -1]
        return s.mean() if s.numel() else torch.tensor(-1.0, dtype=torch.float64, device=precision.device)
    ap = lambda a, m, t=slice(None): mean(precision[t, :, :, a, m])
    ar = lambda a, m: mean(recall[:, :, a, m])
    return torch.stack([ap(0, 2), ap(0, 2, slice(0, 1)), ap(0, 2, slice(5, 6)), ap(1, 2), ap(2, 2), ap(3, 2),
                        ar(0, 0), ar(0, 1), ar(0, 2), ar(1, 2), ar(2, 2), ar(3, 2)]).double()


def summary_lines(stats) -> List[str]:
    rows = [(1, None, 0, 100), (1, 0.5, 0, 100), (1, 0.75, 0, 100), (1, None, 1, 100), (1, None, 2, 100), (1, None, 3, 100),
            (0, None, 0, 1), (0, None, 0, 10), (0, None, 0, 100), (0, None, 1, 100), (0, None, 2, 100), (0, None, 3, 100)]
    out = []
    for value, (is_ap, iou, a, max_det) in zip(stats.tolist(), rows):
        iou_str = "{:0.2f}:{:0.2f}".format(IOU_THRESHOLDS[0], IOU_THRESHOLDS[-1]) if iou is None else "{:0.2f}".format(iou)
        out.append(" {:<18} {} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(
            "Average Precision" if is_ap else "Average Recall", "(AP)" if is_ap else "(AR)", iou_str, AREA_NAMES[a], max_det,
            value))
    return out


class CocoBoxEvaluator:
    """``CocoEvaluator(coco, ["bbox"])`` of the reference, fed with tensors.  ``category_ids``: the dataset's category
    ids (``K`` = sorted unique); detections with another label are dropped.  ``device``: where the records live
    (default: the device of the first batch's detections); HIP kernels on a HIP device, the torch composite on the CPU."""

    def __init__(self, category_ids: Iterable[int], device=None):
        self.category_ids = sorted({int(c) for c in category_ids})
        K = len(self.category_ids)
        if K == 0 or K > MAX_CATEGORIES or self.category_ids[0] < 0:
            raise ValueError(f"CocoBoxEvaluator: 1 .. {MAX_CATEGORIES} non-negative category ids, got {K}")
        self.device = torch.device(device) if device is not None else None
        lut = torch.full((self.category_ids[-1] + 1,), -1, dtype=torch.int32)
        lut[torch.tensor(self.category_ids)] = torch.arange(K, dtype=torch.int32)
        self._lut_host, self._const = lut, None
        self._batches: List[Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]] = []
        self._seen = set()
        self.eval: Optional[Dict[str, object]] = None
        self.stats: Optional[torch.Tensor] = None
        self._det = self._gt = None

    def _constants(self):
        if self._const is None:
            self._const = (self._lut_host.to(self.device), torch.from_numpy(IOU_THRESHOLDS).to(self.device),
                           torch.from_numpy(RECALL_THRESHOLDS).to(self.device))
        return self._const

    def update(self, detections: Detections, targets: Sequence[Dict]) -> None:
        if not (isinstance(detections, tuple) and len(detections) == 4 and isinstance(detections[0], torch.Tensor)):
            detections = pad_detections(list(detections))
        scores, labels, boxes, count = detections
        if len(targets) != scores.shape[0]:
            raise RuntimeError(f"CocoBoxEvaluator.update: {scores.shape[0]} images of detections, {len(targets)} targets")
        ids = [int(t["image_id"]) for t in targets]
        if len(set(ids)) != len(ids) or self._seen & set(ids):
            raise RuntimeError(f"CocoBoxEvaluator.update: image id seen twice: {sorted(set(i for i in ids if ids.count(i) > 1) | (self._seen & set(ids)))}")
        if scores.shape[1] > MAX_PER_IMAGE or max(int(t["boxes"].shape[0]) for t in targets) > MAX_PER_IMAGE:
            raise RuntimeError(f"CocoBoxEvaluator.update: at most {MAX_PER_IMAGE} detections and ground truths per image")
        if self.device is None:
            self.device = scores.device
        lut, thr, _ = self._constants()
        dev = self.device
        args = (scores.to(dev).float().contiguous(), labels.to(dev).long().contiguous(), boxes.to(dev).float().contiguous(),
                count.to(dev).to(torch.int32).contiguous()) + pad_targets(targets, dev)
        if dev.type == "cuda":
            self._batches.append(hip_update(*args, lut, len(self.category_ids), thr))
        else:
            self._batches.append(_composite_update(*args, lut, len(self.category_ids), thr) + (None,))
        self._seen.update(ids)
        self.eval = None

    def _records(self):
        """(detection records, ground-truth records): the real rows of every batch so far."""
        dev = self.device or torch.device("cpu")
        if not self._batches:
            return (torch.zeros((0, DET_WORDS), dtype=torch.int64, device=dev),
                    torch.zeros((0, GT_WORDS), dtype=torch.int64, device=dev))
        padded = [t for _, _, t in self._batches if t is not None]
        totals = iter(torch.stack(padded).cpu().tolist() if padded else ())
        dets, gts = [], []
        for det, gt, t in self._batches:
            if t is not None:
                nd, ng = next(totals)
                det, gt = det[:nd], gt[:ng]
            dets.append(det)
            gts.append(gt)
        det, gt = torch.cat(dets), torch.cat(gts)
        self._batches = [(det, gt, None)]
        return det, gt

    def synchronize_between_processes(self) -> None:
        """All-gather the records (and the image ids seen) when ``torch.distributed`` is initialised; otherwise nothing."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return
        det, gt = self._records()
        seen = torch.tensor(sorted(self._seen), dtype=torch.int64, device=det.device).view(-1, 1)
        via = torch.device("cpu") if dist.get_backend() == "gloo" else det.device
        world = dist.get_world_size()

        def gather(rows):
            rows = rows.to(via)
            sizes = [torch.zeros(1, dtype=torch.int64, device=via) for _ in range(world)]
            dist.all_gather(sizes, torch.tensor([rows.shape[0]], dtype=torch.int64, device=via))
            sizes = [int(s) for s in sizes]
            mine = torch.zeros((max(sizes + [1]), rows.shape[1]), dtype=torch.int64, device=via)
            mine[:rows.shape[0]] = rows
            parts = [torch.zeros_like(mine) for _ in range(world)]
            dist.all_gather(parts, mine)
            return torch.cat([p[:n] for p, n in zip(parts, sizes)]).to(det.device)
        det, gt, seen = gather(det), gather(gt), gather(seen)[:, 0].tolist()
        if len(set(seen)) != len(seen):
            raise RuntimeError("CocoBoxEvaluator.synchronize_between_processes: an image id was evaluated on two ranks")
        self._seen = set(seen)
        self._batches = [(det, gt, None)]
        self.eval = None

    def accumulate(self) -> Dict[str, object]:
        det, gt = self._records()
        K, dev = len(self.category_ids), det.device
        if bool((gt[:, 2] < 0).any()):
            raise RuntimeError(f"CocoBoxEvaluator: more than {GT_CAPACITY} ground truths of one category in an image "
                               "(the capacity of the HIP form)")
        det = sort_records(det)
        category_first = torch.searchsorted((det[:, 1] & 0xFFFFFFFF).contiguous(), torch.arange(K + 1, device=dev))
        npig = torch.zeros((K, A), dtype=torch.int64, device=dev).index_add_(0, gt[:, 1], gt[:, 2:2 + A])
        recall_thresholds = (self._constants()[2] if self.device is not None else torch.from_numpy(RECALL_THRESHOLDS)).to(dev)
        run = hip_accumulate if dev.type == "cuda" else _composite_accumulate
        precision, recall, scores = run(det, category_first, npig, K, recall_thresholds)
        self._det, self._gt = det, gt
        self.eval = {"precision": precision.cpu(), "recall": recall.cpu(), "scores": scores.cpu(),
                     "counts": [T, R, K, A, M]}
        return self.eval

    def summarize(self, verbose: bool = True) -> torch.Tensor:
        if self.eval is None:
            self.accumulate()
        self.stats = summarize_stats(self.eval["precision"], self.eval["recall"])
        if verbose:
            print("\n".join(summary_lines(self.stats)))
        return self.stats

    def per_category_table(self, category_names: Optional[Sequence[str]] = None) -> List[List[object]]:
        """The rows of the reference's per-class table (engine.py:147-169): header, one row per category (class, images
        with a ground truth of it, ground truths, detections, recall at IoU 0.5, AP50; area all, 100 detections) and the
        mean line.  ``dets`` counts the detections that enter the evaluation: at most 100 per image and category."""
        if self.eval is None:
            self.accumulate()
        K = len(self.category_ids)
        names = list(category_names) if category_names is not None else [str(c) for c in self.category_ids]
        images = torch.bincount(self._gt[:, 1], minlength=K).tolist()
        gts = torch.zeros(K, dtype=torch.int64, device=self._gt.device).index_add_(0, self._gt[:, 1], self._gt[:, 6]).tolist()
        dets = torch.bincount(self._det[:, 1] & 0xFFFFFFFF, minlength=K).tolist()
        precision, recall = self.eval["precision"], self.eval["recall"]
        table = [["class", "imgs", "gts", "dets", "recall", "ap"]]
        for k in range(K):
            table.append([names[k], images[k], gts[k], dets[k], f"{recall[0, k, 0, 2].item():.3f}",
                          f"{precision[0, :, k, 0, 2].mean().item():.3f}"])
        cat_recall, cat_ap = recall[0, :, 0, 2], precision[0, :, :, 0, 2]
        valid_recall, valid_ap = cat_recall[cat_recall >= 0], cat_ap[cat_ap >= 0]
        table.append(["mean results", "", "", "", f"{float(valid_recall.sum()) / max(valid_recall.numel(), 1):.3f}",
                      f"{float(valid_ap.sum()) / max(valid_ap.numel(), 1):.3f}"])
        return table


@torch.no_grad()
def evaluate(model, batches: Iterable, category_ids: Iterable[int], verbose: bool = True):
    """The loop of the reference's ``evaluate_acc``: ``model.eval()``, one ``update`` per ``(images, targets)`` batch of
    ``batches`` with what ``model(images)`` returns, then ``synchronize_between_processes``, ``accumulate`` and
    ``summarize``.  Returns ``(evaluator, {metric name: value})`` with the reference's metric names."""
    model.eval()
    evaluator = CocoBoxEvaluator(category_ids)
    for images, targets in batches:
        evaluator.update(model(images), targets)
    evaluator.synchronize_between_processes()
    evaluator.accumulate()
    stats = evaluator.summarize(verbose=verbose)
    return evaluator, dict(zip(METRIC_NAMES, stats.tolist()))
