"""Generate tests/golden/set_criterion_cases.npz from the IMPORTED reference HybridSetCriterion / HungarianMatcher.

Run in the authoring container only (needs the upstream reference checkout and scipy, see _ref_import.py):

    python tests/golden/make_set_criterion_golden.py

The fixture holds real outputs of ``models/bricks/set_criterion.py:HybridSetCriterion`` with
``models/matcher/hungarian_matcher.py:HungarianMatcher(cost_class=2, cost_bbox=5, cost_giou=2)`` on CPU (scipy's
``linear_sum_assignment``) and of ``DNDETRDetector.compute_dn_loss`` (models/detectors/base_detector.py:188-245).
torchvision is absent, so its three box functions are served by restatements set on the stub module below, after
``install()``: ``_box_cxcywh_to_xyxy`` (by _ref_import.py), ``box_iou`` and ``generalized_box_iou`` (torchvision's
formulas: clamp(min=0) on the intersection and on the enclosing box).  Everything else is the reference's own code.

Inputs are redrawn until scipy's assignment of every problem is unchanged under 1e-5 relative noise on the cost in three
draws, so that the optimum is unique with margin and index equality is a fair bar.  Logits are drawn as fp16-representable
fp32 values (stored as fp16, exact) to halve the file; the bf16 case stores bf16 bits and the reference runs on the same
values upcast to fp32.  Case ``full`` (Nq = 900, 7 outputs) is too large to store: its inputs are regenerated in the test
from the stored seed with torch's CPU generator (``draw_full``, mirrored in the test) and checked against stored digests.

Cases (C = 91, alpha = 0.25, gamma = 2; upstream gradient of each loss key a stored random weight):
  main     B = 2, Nq = 300, outputs main + 2 aux + enc, T = (5, 37): indices, losses, d/dboxes of every output,
           d/dlogits of the main output in full and of the others as row / column sums
  empty    B = 2, Nq = 50, main + enc, T = (0, 7)
  binary   B = 2, Nq = 50, main + enc, T = (4, 9), two_stage_binary_cls=True
  dn       B = 2, 5 groups, max_gt = 6, T = (6, 3), Nq = 30, main + 2 aux: compute_dn_loss's indices and losses
  full     B = 2, Nq = 900, 6 + 1 outputs, T = (20, 100): indices, losses, gradient digests (sums)
  bf16     B = 2, Nq = 150, main + enc, T = (6, 21), bf16 logits: indices, losses, d/dboxes, d/dlogits sums
The file stays under 1 MiB.
"""
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
warnings.filterwarnings("ignore")

import _ref_import  # noqa: E402

_ref_import.install()


def _box_area(b):
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def _box_inter_union(boxes1, boxes2):
    area1, area2 = _box_area(boxes1), _box_area(boxes2)
    lt = torch.max(boxes1[:, None, :2], boxes2[:, :2])
    rb = torch.min(boxes1[:, None, 2:], boxes2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter, area1[:, None] + area2 - inter


def box_iou(boxes1, boxes2):
    inter, union = _box_inter_union(boxes1, boxes2)
    return inter / union


def generalized_box_iou(boxes1, boxes2):
    inter, union = _box_inter_union(boxes1, boxes2)
    iou = inter / union
    lti = torch.min(boxes1[:, None, :2], boxes2[:, :2])
    rbi = torch.max(boxes1[:, None, 2:], boxes2[:, 2:])
    whi = (rbi - lti).clamp(min=0)
    areai = whi[:, :, 0] * whi[:, :, 1]
    return iou - (areai - union) / areai


_ops_boxes = sys.modules["torchvision.ops.boxes"]
_ops_boxes.box_iou = box_iou
_ops_boxes.generalized_box_iou = generalized_box_iou

from scipy.optimize import linear_sum_assignment  # noqa: E402

from models.bricks.set_criterion import HybridSetCriterion  # noqa: E402
from models.matcher.hungarian_matcher import HungarianMatcher  # noqa: E402



def _stub_detector_imports():
    """base_detector.py imports the reference's image transforms (pycocotools, torchvision) and util.misc for its
    pre-processing; compute_dn_loss uses none of them.  Import-only stand-ins, like _ref_import.py's."""
    import enum

    class InterpolationMode(enum.Enum):
        BILINEAR = "bilinear"

    tr = _ref_import._stub("transforms")
    tr.functional = _ref_import._stub("transforms.functional", InterpolationMode=InterpolationMode)
    tr.v2 = _ref_import._stub("transforms.v2")
    import util  # noqa: F401  (the real package; only util.misc is replaced)
    _ref_import._stub("util.misc", decode_labels=None, encode_labels=None, image_list_from_tensors=None)


_stub_detector_imports()
from models.detectors.base_detector import DNDETRDetector  # noqa: E402

compute_dn_loss = DNDETRDetector.compute_dn_loss

C = 91
KEYS = ("loss_class", "loss_bbox", "loss_giou")


def draw_full(seed, B=2, Nq=900, n_out=7, counts=(20, 100)):
    """The ``full`` case's inputs from torch's CPU generator (mirrored in tests/test_set_criterion_gpu.py)."""
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(n_out, B, Nq, C, generator=g) * 1.5 - 3.0).half().float()
    cxcy = torch.rand(n_out, B, Nq, 2, generator=g) * 0.8 + 0.1
    wh = torch.rand(n_out, B, Nq, 2, generator=g) * 0.3 + 0.02
    boxes = torch.cat([cxcy, wh], -1)
    targets = []
    for n in counts:
        tc = torch.rand(n, 2, generator=g) * 0.8 + 0.1
        tw = torch.rand(n, 2, generator=g) * 0.3 + 0.02
        targets.append({"boxes": torch.cat([tc, tw], -1), "labels": torch.randint(0, C, (n,), generator=g)})
    return logits, boxes, targets


def draw(g, n_out, B, Nq, counts, dtype=torch.float32):
    logits = (torch.randn(n_out, B, Nq, C, generator=g) * 1.5 - 3.0)
    logits = logits.half().float() if dtype == torch.float32 else logits.to(dtype).float()
    cxcy = torch.rand(n_out, B, Nq, 2, generator=g) * 0.8 + 0.1
    wh = torch.rand(n_out, B, Nq, 2, generator=g) * 0.3 + 0.02
    boxes = torch.cat([cxcy, wh], -1)
    targets = []
    for n in counts:
        tc = torch.rand(n, 2, generator=g) * 0.8 + 0.1
        tw = torch.rand(n, 2, generator=g) * 0.3 + 0.02
        targets.append({"boxes": torch.cat([tc, tw], -1), "labels": torch.randint(0, C, (n,), generator=g)})
    return logits, boxes, targets


def stable(matcher, logits, boxes, targets, binary_last, g):
    """scipy's assignment of every problem is unchanged under 1e-5 relative noise (three draws)."""
    for o in range(logits.shape[0]):
        for b, t in enumerate(targets):
            if len(t["labels"]) == 0:
                continue
            labels = torch.zeros_like(t["labels"]) if (binary_last and o == logits.shape[0] - 1) else t["labels"]
            c = matcher.calculate_cost(boxes[o, b], logits[o, b], t["boxes"], labels).double().numpy()
            base = linear_sum_assignment(c)
            for _ in range(3):
                noise = torch.randn(c.shape, generator=g, dtype=torch.float64).numpy()
                alt = linear_sum_assignment(c * (1 + 1e-5 * noise))
                if not (np.array_equal(alt[0], base[0]) and np.array_equal(alt[1], base[1])):
                    return False
    return True


def outputs_of(logits, boxes, enc=True):
    n = logits.shape[0]
    dec = n - 1 if enc else n
    out = {"pred_logits": logits[0], "pred_boxes": boxes[0],
           "aux_outputs": [{"pred_logits": logits[i], "pred_boxes": boxes[i]} for i in range(1, dec)]}
    if enc:
        out["enc_outputs"] = {"pred_logits": logits[n - 1], "pred_boxes": boxes[n - 1]}
    return out


def suffixes(n, enc=True):
    dec = n - 1 if enc else n
    return [""] + [f"_{i}" for i in range(dec - 1)] + (["_enc"] if enc else [])


def run_case(data, tag, g, counts, B, Nq, n_out, binary=False, dtype=torch.float32, full_grads=True, seed=None):
    matcher = HungarianMatcher(cost_class=2, cost_bbox=5, cost_giou=2)
    crit = HybridSetCriterion(C, matcher, {}, alpha=0.25, gamma=2.0, two_stage_binary_cls=binary)
    while True:
        if seed is not None:
            logits, boxes, targets = draw_full(seed)
        else:
            logits, boxes, targets = draw(g, n_out, B, Nq, counts, dtype)
        if stable(matcher, logits, boxes, targets, binary, g):
            break
        if seed is not None:
            seed += 1
    lg = logits.clone().requires_grad_(True)
    bx = boxes.clone().requires_grad_(True)
    losses = crit(outputs_of(lg, bx), targets)
    sfx = suffixes(n_out)
    weights = torch.rand(n_out, 3, generator=g) * 1.5 + 0.5
    total = sum(weights[i, k] * losses[KEYS[k] + s] for i, s in enumerate(sfx) for k in range(3))
    total.backward()
    data[f"{tag}_losses"] = np.array([[losses[k + s].item() for k in KEYS] for s in sfx], dtype=np.float64)
    data[f"{tag}_weights"] = weights.numpy()
    data[f"{tag}_counts"] = np.array(counts, dtype=np.int64)
    data[f"{tag}_shape"] = np.array([n_out, B, Nq, C, int(binary)], dtype=np.int64)
    # indices of every output (the reference's matcher on each output's own logits / boxes)
    idx = np.full((n_out, B, Nq), -1, dtype=np.int32)
    for o in range(n_out):
        for b, t in enumerate(targets):
            labels = torch.zeros_like(t["labels"]) if (binary and o == n_out - 1) else t["labels"]
            src, tgt = matcher(boxes[o, b], logits[o, b], t["boxes"], labels)
            idx[o, b, src.numpy()] = tgt.numpy()
    data[f"{tag}_match"] = idx
    if seed is None:
        if dtype == torch.bfloat16:
            data[f"{tag}_logits_bf16"] = logits.bfloat16().view(torch.int16).numpy()
        else:
            data[f"{tag}_logits_f16"] = logits.half().numpy()
        data[f"{tag}_boxes"] = boxes.numpy()
        data[f"{tag}_tboxes"] = torch.cat([t["boxes"] for t in targets]).numpy().reshape(-1, 4)
        data[f"{tag}_tlabels"] = torch.cat([t["labels"] for t in targets]).numpy().astype(np.int32)
    else:
        data[f"{tag}_seed"] = np.array([seed], dtype=np.int64)
        data[f"{tag}_input_digest"] = np.array([logits.double().sum().item(), boxes.double().sum().item(),
                                                sum(t["boxes"].double().sum().item() for t in targets)])
    gl, gb = lg.grad.numpy(), bx.grad.numpy()
    data[f"{tag}_grad_boxes"] = gb
    if full_grads:
        data[f"{tag}_grad_logits"] = gl
    else:
        data[f"{tag}_grad_logits0"] = gl[0]
    data[f"{tag}_grad_logits_rowsum"] = gl.astype(np.float64).sum(-1)
    data[f"{tag}_grad_logits_colsum"] = gl.astype(np.float64).sum(-2)
    return lg, bx, targets


def dn_case(data, g):
    groups, max_gt, counts, Nq, n_out = 5, 6, (6, 3), 30, 3
    logits, boxes, targets = draw(g, n_out, 2, Nq, counts)
    matcher = HungarianMatcher(cost_class=2, cost_bbox=5, cost_giou=2)
    crit = HybridSetCriterion(C, matcher, {}, alpha=0.25, gamma=2.0)
    lg = logits.clone().requires_grad_(True)
    bx = boxes.clone().requires_grad_(True)
    dn_out = {"pred_logits": lg[0], "pred_boxes": bx[0],
              "aux_outputs": [{"pred_logits": lg[i], "pred_boxes": bx[i]} for i in range(1, n_out)]}
    captured = []

    class _Crit:
        def calculate_loss(self, outputs, targets, num_boxes, indices=None, **kw):
            captured.append([(s.numpy().copy(), t.numpy().copy()) for s, t in indices])
            return crit.calculate_loss(outputs, targets, num_boxes, indices=indices)

    fake = types.SimpleNamespace(device=torch.device("cpu"), criterion=_Crit())
    losses = compute_dn_loss(fake, {"denoising_output": dn_out, "denoising_groups": groups,
                                    "max_gt_num_per_image": max_gt}, targets)
    sfx = ["_dn"] + [f"_dn_{i}" for i in range(n_out - 1)]
    weights = torch.rand(n_out, 3, generator=g) * 1.5 + 0.5
    total = sum(weights[i, k] * losses[KEYS[k] + s] for i, s in enumerate(sfx) for k in range(3))
    total.backward()
    idx = np.full((2, Nq), -1, dtype=np.int32)
    for b, (s, t) in enumerate(captured[0]):
        idx[b, s] = t
    data["dn_match"] = idx
    data["dn_src"] = np.concatenate([s for s, _ in captured[0]]).astype(np.int64)
    data["dn_tgt"] = np.concatenate([t for _, t in captured[0]]).astype(np.int64)
    data["dn_params"] = np.array([groups, max_gt, Nq, n_out], dtype=np.int64)
    data["dn_counts"] = np.array(counts, dtype=np.int64)
    data["dn_losses"] = np.array([[losses[k + s].item() for k in KEYS] for s in sfx], dtype=np.float64)
    data["dn_weights"] = weights.numpy()
    data["dn_logits_f16"] = logits.half().numpy()
    data["dn_boxes"] = boxes.numpy()
    data["dn_tboxes"] = torch.cat([t["boxes"] for t in targets]).numpy()
    data["dn_tlabels"] = torch.cat([t["labels"] for t in targets]).numpy().astype(np.int32)
    data["dn_grad_logits"] = lg.grad.numpy()
    data["dn_grad_boxes"] = bx.grad.numpy()


def main():
    g = torch.Generator().manual_seed(20261017)
    data = {}
    run_case(data, "main", g, (5, 37), 2, 300, 4, full_grads=False)
    run_case(data, "empty", g, (0, 7), 2, 50, 2)
    run_case(data, "binary", g, (4, 9), 2, 50, 2, binary=True)
    dn_case(data, g)
    run_case(data, "full", g, (20, 100), 2, 900, 7, full_grads=False, seed=900)
    data["full_grad_boxes_sum"] = data.pop("full_grad_boxes").astype(np.float64).sum(2)
    del data["full_grad_logits0"]   # digests only at full size
    run_case(data, "bf16", g, (6, 21), 2, 150, 2, dtype=torch.bfloat16, full_grads=False)
    del data["bf16_grad_logits0"]
    out = os.path.join(HERE, "set_criterion_cases.npz")
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
