"""Generate tests/golden/denoising_cases.npz from the IMPORTED reference ``GenerateCDNQueries``.

Run in the authoring container only (needs the upstream reference checkout, see _ref_import.py):

    python tests/golden/make_denoising_golden.py

The fixture holds real outputs of ``models/bricks/denoising.py:GenerateCDNQueries.forward`` on CPU together with the
values ``torch.rand_like`` / ``torch.randint_like`` returned inside the call (recorded by wrapping the two functions for
the duration of the call), so that the product kernel can be driven with the same noise
(``salience_detr_amd.denoising.pack_noise``).  torchvision is absent, so its two box conversions are served by
restatements on the stub module (``_box_cxcywh_to_xyxy`` by _ref_import.py, ``_box_xyxy_to_cxcywh`` below: torchvision's
``((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1)``); ``util.misc`` is the reference's own module, imported with a
stand-in for ``accelerate`` where that package is missing.  Everything else is the reference's own code.

Per case: inputs (counts, target boxes / labels, ``label_encoder.weight``, the constructor arguments), the recorded draws,
and the outputs: box queries, the attention mask (bit-packed), groups, ``2 * max_gt`` and the label queries -- in full
where E = 32, and for every case as ``noised_labels`` ``[B, n_dn]`` (-1 = a zero padding row), the class whose embedding
row each label query equals bit for bit (checked here before it is stored).  A case is redrawn while a flip uniform lies
within 1e-6 of the threshold.  The file stays under 1 MiB.
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


def _box_xyxy_to_cxcywh(boxes):
    x1, y1, x2, y2 = boxes.unbind(-1)
    return torch.stack(((x1 + x2) / 2, (y1 + y2) / 2, x2 - x1, y2 - y1), dim=-1)


sys.modules["torchvision.ops.boxes"]._box_xyxy_to_cxcywh = _box_xyxy_to_cxcywh


def _stub_misc_imports():
    """util/misc.py imports accelerate at module level; inverse_sigmoid (the one function the generator calls) does not
    use it.  An import-only stand-in, like _ref_import.py's, where the package is missing."""
    try:
        import accelerate  # noqa: F401
        import accelerate.logging  # noqa: F401
    except Exception:
        acc = _ref_import._stub("accelerate")
        acc.logging = _ref_import._stub("accelerate.logging", get_logger=lambda *a, **k: None)


_stub_misc_imports()
from models.bricks.denoising import GenerateCDNQueries  # noqa: E402

# tag, counts, C, E, num_queries, denoising_nums, label_noise_prob, box_noise_scale, box style
CASES = [
    ("main", (3, 5), 91, 256, 900, 100, 0.5, 1.0, "inside"),
    ("empty_image", (0, 7), 91, 32, 20, 100, 0.5, 1.0, "inside"),
    ("single", (1,), 91, 32, 20, 100, 0.5, 1.0, "inside"),
    ("empty_batch", (0, 0), 91, 32, 20, 100, 0.5, 1.0, "inside"),
    ("floor", (100, 37), 91, 32, 20, 100, 0.5, 1.0, "inside"),
    ("over", (130, 2), 91, 32, 20, 100, 0.5, 1.0, "inside"),
    ("clamp", (9, 14), 20, 32, 20, 100, 0.5, 1.0, "border"),
    ("no_label_noise", (4, 6), 91, 32, 20, 100, 0.0, 1.0, "inside"),
    ("no_box_noise", (4, 6), 91, 32, 20, 100, 0.5, 0.0, "inside"),
    ("scaled", (6, 2, 11), 7, 32, 50, 40, 0.8, 0.4, "inside"),
]


def draw_targets(g, counts, C, style):
    labels, boxes = [], []
    for n in counts:
        if style == "border":       # boxes that reach over the image border: the clamp at 0 and 1 acts, widths collapse
            cxcy = torch.rand(n, 2, generator=g)
            wh = torch.rand(n, 2, generator=g) * 0.7 + 0.2
        else:
            cxcy = torch.rand(n, 2, generator=g) * 0.6 + 0.2
            wh = torch.rand(n, 2, generator=g) * 0.3 + 0.02
        boxes.append(torch.cat([cxcy, wh], -1))
        labels.append(torch.randint(0, C, (n,), generator=g))
    return labels, boxes


class Recorder:
    """Wraps torch.rand_like / torch.randint_like: draws from a seeded CPU generator and keeps what was returned."""

    def __init__(self, g):
        self.g, self.draws = g, []

    def __enter__(self):
        self._rand_like, self._randint_like = torch.rand_like, torch.randint_like

        def rand_like(x, **kw):
            out = torch.rand(x.shape, generator=self.g, dtype=kw.get("dtype", x.dtype))
            self.draws.append(("rand", out.clone()))
            return out

        def randint_like(x, low=0, high=None, **kw):
            if high is None:
                low, high = 0, low
            out = torch.randint(low, high, x.shape, generator=self.g).to(kw.get("dtype", x.dtype))
            self.draws.append(("randint", out.clone()))
            return out

        torch.rand_like, torch.randint_like = rand_like, randint_like
        return self

    def __exit__(self, *exc):
        torch.rand_like, torch.randint_like = self._rand_like, self._randint_like


def run_case(data, g, tag, counts, C, E, Nq, nums, p_label, s_box, style):
    gen = GenerateCDNQueries(num_queries=Nq, num_classes=C, label_embed_dim=E, denoising_nums=nums,
                             label_noise_prob=p_label, box_noise_scale=s_box)
    weight = torch.randn(C, E, generator=g)
    with torch.no_grad():
        gen.label_encoder.weight.copy_(weight)
    while True:
        labels, boxes = draw_targets(g, counts, C, style)
        with Recorder(g) as rec, torch.no_grad():
            lq, bq, mask, groups, twice_max_gt = gen([l.clone() for l in labels], [b.clone() for b in boxes])
        draws = list(rec.draws)
        flip = new_label = sign = magnitude = None
        if p_label > 0:
            (_, flip), (_, new_label) = draws[0], draws[1]
            draws = draws[2:]
        if s_box > 0:
            (_, sign), (_, magnitude) = draws[0], draws[1]
            draws = draws[2:]
        assert not draws
        if flip is None or flip.numel() == 0 or ((flip - p_label * 0.5).abs() > 1e-6).all():
            break
    B, n_dn = len(counts), lq.shape[1]
    max_gt = max(counts)
    assert twice_max_gt == 2 * max_gt and n_dn == 2 * groups * max_gt
    # the class whose embedding row each label query is, bit for bit (-1: a zero padding row)
    noised = np.full((B, n_dn), -1, dtype=np.int32)
    for b, n in enumerate(counts):
        for r in range(2 * groups):
            for t in range(n):
                s = r * max_gt + t
                hit = (weight == lq[b, s]).all(-1).nonzero().flatten()
                assert hit.numel() == 1, (tag, b, s)
                noised[b, s] = int(hit[0])
    restored = torch.zeros_like(lq)
    for b in range(B):
        for s in range(n_dn):
            if noised[b, s] >= 0:
                restored[b, s] = weight[noised[b, s]]
    assert torch.equal(restored, lq)
    if style == "border":
        sig = bq.sigmoid()
        valid = torch.from_numpy(noised >= 0)
        assert (bq[valid][:, 2:] <= -6.9).sum() >= 2, "no collapsed width in the clamp case"
        assert (sig[valid][:, 2:] > 0.9).sum() >= 2
    data[f"{tag}_counts"] = np.array(counts, dtype=np.int64)
    data[f"{tag}_params"] = np.array([C, E, Nq, nums, groups, twice_max_gt], dtype=np.int64)
    data[f"{tag}_noise_params"] = np.array([p_label, s_box], dtype=np.float64)
    data[f"{tag}_weight"] = weight.numpy()
    data[f"{tag}_tboxes"] = torch.cat(boxes).numpy().reshape(-1, 4)
    data[f"{tag}_tlabels"] = torch.cat(labels).numpy().astype(np.int32)
    if flip is not None:
        data[f"{tag}_draw_flip"] = flip.numpy()
        data[f"{tag}_draw_label"] = new_label.numpy().astype(np.int32)
    if sign is not None:
        data[f"{tag}_draw_sign"] = sign.numpy().astype(np.uint8)
        data[f"{tag}_draw_magnitude"] = magnitude.numpy()
    data[f"{tag}_noised_labels"] = noised
    data[f"{tag}_box_queries"] = bq.numpy()
    if E <= 32:
        data[f"{tag}_label_queries"] = lq.numpy()
    data[f"{tag}_mask_bits"] = np.packbits(mask.numpy().reshape(-1))
    data[f"{tag}_mask_side"] = np.array([mask.shape[0]], dtype=np.int64)
    print(tag, "groups", groups, "n_dn", n_dn, "mask", tuple(mask.shape))


def main():
    g = torch.Generator().manual_seed(20261016)
    data = {"tags": np.array([c[0] for c in CASES])}
    for case in CASES:
        run_case(data, g, *case)
    out = os.path.join(HERE, "denoising_cases.npz")
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
