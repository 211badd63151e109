"""Generate tests/golden/postprocess_cases.npz from the IMPORTED reference PostProcess.

Run in the authoring container only (needs the upstream reference checkout, see _ref_import.py):

    python tests/golden/make_postprocess_golden.py

The fixture holds real outputs of ``models/bricks/post_process.py:PostProcess`` on CPU.  torchvision is absent, so
two of its functions are served by restatements: ``_box_cxcywh_to_xyxy`` by _ref_import.py (a three-line conversion),
and ``torchvision.ops.boxes.nms`` -- set below, after ``install()`` -- by the oracle's greedy NMS
(oracle/salience_ref.py:nms_greedy).  Everything else (sigmoid, topk, div / mod, gather, scaling, the filter masks) is
the reference's own code.

Cases (B = 2, Nq = 900, C = 91, target sizes int64, one input set shared by the fp32 cases):
  f32_k100, f32_k300        (k, nms, conf) = (100, -1, -1), (300, -1, -1)
  f32_k300_conf             (300, -1, 0.3)
  f32_k300_nms_conf         (300, 0.5, 0.3)
  bf16_k300                 bf16 logits, (300, -1, -1)
The fp32 logits are redrawn until no two of the top 301 probabilities of an image tie, so the reference's order is the
unique one and the fp32 parity can be exact.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
warnings.filterwarnings("ignore")

import _ref_import  # noqa: E402

_ref_import.install()

from oracle import salience_ref as R  # noqa: E402

sys.modules["torchvision.ops.boxes"].nms = lambda boxes, scores, iou_threshold: R.nms_greedy(boxes, scores, iou_threshold)

from models.bricks.post_process import PostProcess  # noqa: E402

B, NQ, C = 2, 900, 91
CASES = [("f32_k100", 100, -1, -1), ("f32_k300", 300, -1, -1), ("f32_k300_conf", 300, -1, 0.3),
         ("f32_k300_nms_conf", 300, 0.5, 0.3)]


def draw_boxes(g):
    """Queries clustered around 40 objects per image (DETR-like duplicates), so that NMS has work to do."""
    base_c = torch.rand(B, 40, 2, generator=g) * 0.8 + 0.1
    base_wh = torch.rand(B, 40, 2, generator=g) * 0.3 + 0.03
    pick = torch.randint(0, 40, (B, NQ), generator=g)
    c = torch.gather(base_c, 1, pick[..., None].expand(-1, -1, 2)) + torch.randn(B, NQ, 2, generator=g) * 0.01
    wh = torch.gather(base_wh, 1, pick[..., None].expand(-1, -1, 2)) * (1 + torch.randn(B, NQ, 2, generator=g) * 0.05)
    return torch.cat([c, wh.abs()], -1).float().contiguous()


def draw_logits(g):
    while True:
        logits = (torch.randn(B, NQ, C, generator=g) * 1.2 - 4.5).float()
        top = torch.topk(logits.sigmoid().view(B, -1), 301, dim=1)[0]
        if bool((top[:, 1:] != top[:, :-1]).all()):
            return logits


def main():
    g = torch.Generator().manual_seed(20261016)
    logits = draw_logits(g)
    boxes = draw_boxes(g)
    sizes = torch.tensor([[800, 1066], [640, 1333]], dtype=torch.int64)
    data = {"logits_f32": logits.numpy(), "boxes": boxes.numpy(), "target_sizes": sizes.numpy()}
    for tag, k, nms, conf in CASES:
        res = PostProcess(k, nms, conf)({"pred_logits": logits, "pred_boxes": boxes}, sizes)
        for i, r in enumerate(res):
            data[f"{tag}_scores{i}"] = r["scores"].numpy()
            data[f"{tag}_labels{i}"] = r["labels"].numpy()
            data[f"{tag}_boxes{i}"] = r["boxes"].numpy()
        data[f"{tag}_params"] = np.array([k, nms, conf], dtype=np.float64)
    lb = (torch.randn(B, NQ, C, generator=g) * 1.2 - 4.5).bfloat16()
    data["logits_bf16_bits"] = lb.view(torch.int16).numpy()
    res = PostProcess(300)({"pred_logits": lb, "pred_boxes": boxes}, sizes)
    for i, r in enumerate(res):
        data[f"bf16_k300_scores{i}"] = r["scores"].float().numpy()
        data[f"bf16_k300_labels{i}"] = r["labels"].numpy()
        data[f"bf16_k300_boxes{i}"] = r["boxes"].numpy()
    out = os.path.join(HERE, "postprocess_cases.npz")
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes;", {t: len(data[f"{t}_scores0"]) for t, *_ in CASES})


if __name__ == "__main__":
    main()
