"""GPU: the detector's training forward (``SalienceDETR.forward(images, targets)`` in ``train()`` mode,
salience_detr_amd/detector.py) at reduced dimensions (256 channels, 2 + 2 layers, 10 proposals, a three-convolution stub
backbone): composition against the same parts called by hand, gradients, the eval path of the same object, errors.

``test_training_forward_matches_the_reference_detector`` holds the weighted loss dict to what the imported reference
``SalienceDETR`` computed in ``train()`` mode on the same stored backbone maps, targets, weights and recorded noise
(tests/golden/detector_train_small.npz, tests/golden/make_detector_train_golden.py).
The generator and both criteria are each pinned to the reference on their own (tests/test_denoising_gpu.py,
tests/test_set_criterion_gpu.py, tests/test_criterion_gpu.py) and the transformer's training step to the reference's
gradients (tests/test_transformer_gpu.py); this file pins how the detector wires them together.
"""
import os
import zlib

import numpy as np
import pytest
import torch
from torch import nn

from salience_detr_amd import denoising as D
from salience_detr_amd.backbone import batch_images
from salience_detr_amd.channel_mapper import ChannelMapper
from salience_detr_amd.detector import SalienceDETR, detector_state_dict, prepare_targets
from salience_detr_amd.position_encoding import PositionEmbeddingSine
from salience_detr_amd.post_process import PostProcess
from salience_detr_amd.salience_criterion import SalienceCriterion
from salience_detr_amd.salience_transformer import build_salience_transformer
from salience_detr_amd.set_criterion import HungarianMatcher, HybridSetCriterion, stage_targets
from salience_detr_amd import synthetic as syn

pytestmark = pytest.mark.gpu
C, PROPOSALS, DEC_LAYERS = 7, 10, 2
SIZES = [(64, 96), (48, 80)]


class StubBackbone(nn.Module):
    """Three strided convolutions: feature maps at strides 8 / 16 / 32 under the ResNet's output names."""

    def __init__(self):
        super().__init__()
        self.c2 = nn.Conv2d(3, 32, 8, 8)
        self.c3 = nn.Conv2d(32, 64, 2, 2)
        self.c4 = nn.Conv2d(64, 64, 2, 2)

    def forward(self, x):
        a = self.c2(x)
        b = self.c3(a.relu())
        return {"layer2": a, "layer3": b, "layer4": self.c4(b.relu())}


def weight_dict():
    base = {"loss_class": 1.0, "loss_bbox": 5.0, "loss_giou": 2.0}
    w = dict(base)
    w.update({k + "_dn": v for k, v in base.items()})
    w.update({k + "_enc": v for k, v in base.items()})
    for i in range(DEC_LAYERS - 1):
        w.update({f"{k}_{i}": v for k, v in base.items()})
        w.update({f"{k}_dn_{i}": v for k, v in base.items()})
    w["loss_salience"] = 2.0
    return w


def build(training=True):
    tr = build_salience_transformer(embed_dim=256, num_heads=8, d_ffn=64, num_encoder_layers=2,
                                    num_decoder_layers=DEC_LAYERS, num_classes=C, topk_sa=6, max_num_embedding=20,
                                    two_stage_num_proposals=PROPOSALS)
    tr.static_proposals = True      # the tiny pyramid may keep fewer than 10 tokens after NMS
    kw = {}
    if training:
        crit = HybridSetCriterion(C, HungarianMatcher(cost_class=2, cost_bbox=5, cost_giou=2), weight_dict())
        kw = dict(criterion=crit, focus_criterion=SalienceCriterion(noise_scale=0.0), num_classes=C,
                  num_queries=PROPOSALS, denoising_nums=12)
    det = SalienceDETR(StubBackbone(), ChannelMapper([32, 64, 64], 256, 4),
                       PositionEmbeddingSine(128, 10000, True, offset=-0.5), tr, PostProcess(5), **kw)
    det.load_state_dict(syn.det_state_dict(det.state_dict(), salt=9))
    return det.cuda()


def batch(counts=(3, 2)):
    g = torch.Generator().manual_seed(11)
    images = [torch.randn(3, h, w, generator=g).cuda() for h, w in SIZES]
    targets = []
    for n, (h, w) in zip(counts, SIZES):
        x0 = torch.rand(n, generator=g) * 0.5 * w
        y0 = torch.rand(n, generator=g) * 0.5 * h
        bw = torch.rand(n, generator=g) * 0.4 * w + 4
        bh = torch.rand(n, generator=g) * 0.4 * h + 4
        targets.append({"boxes": torch.stack((x0, y0, x0 + bw, y0 + bh), -1), "labels": torch.randint(0, C, (n,), generator=g)})
    return images, targets


def noise_for(det, counts):
    max_gt = max(counts)
    groups = D.denoising_groups(det.denoising_generator.denoising_nums, max_gt)
    shape = det.denoising_generator.noise_shape(len(counts), max(max_gt, 1), groups)
    return torch.rand(shape, generator=torch.Generator().manual_seed(21)).cuda()


def by_hand(det, images, targets, noise):
    """The reference's training forward (salience_detr.py:163-240) written out with the public parts."""
    with torch.no_grad():
        canvas, mask = batch_images(images, normalize=False)
    prepared = prepare_targets(targets, SIZES)
    feats = det.neck(det.backbone(canvas))
    from salience_detr_amd.position_encoding import level_masks_and_positions
    masks, pos = level_masks_and_positions(mask, [tuple(f.shape[-2:]) for f in feats], det.position_embedding)
    staged = stage_targets(prepared, device="cuda")
    gen = det.denoising_generator
    label_q, box_q, attn_mask, groups, twice = gen([t["labels"] for t in prepared], [t["boxes"] for t in prepared],
                                                   staged=staged, noise=noise)
    out_cls, out_box, enc_cls, enc_box, salience = det.transformer(
        feats, masks, pos, label_q, box_q, attn_mask=attn_mask, image_sizes=[list(s) for s in SIZES],
        canvas=tuple(canvas.shape[-2:]))
    out_cls[0] += gen.label_encoder.weight[0, 0] * 0.0
    n_dn = groups * twice
    dn = {"pred_logits": out_cls[-1, :, :n_dn], "pred_boxes": out_box[-1, :, :n_dn],
          "aux_outputs": [{"pred_logits": out_cls[i, :, :n_dn], "pred_boxes": out_box[i, :, :n_dn]}
                          for i in range(DEC_LAYERS - 1)]}
    output = {"pred_logits": out_cls[-1, :, n_dn:], "pred_boxes": out_box[-1, :, n_dn:],
              "aux_outputs": [{"pred_logits": out_cls[i, :, n_dn:], "pred_boxes": out_box[i, :, n_dn:]}
                              for i in range(DEC_LAYERS - 1)],
              "enc_outputs": {"pred_logits": enc_cls, "pred_boxes": enc_box}}
    losses = det.criterion(output, prepared, staged=staged)
    losses.update(det.criterion.dn_losses(dn, prepared, groups, twice, staged=staged))
    strides = [(canvas.shape[-2] / f.shape[-2], canvas.shape[-1] / f.shape[-1]) for f in feats]
    losses.update(det.focus_criterion(salience, prepared, strides, [list(s) for s in SIZES]))
    w = det.criterion.weight_dict
    return {k: v * w[k] for k, v in losses.items() if k in w}


def test_training_forward_equals_its_parts_called_by_hand():
    det = build().train()
    images, targets = batch()
    noise = noise_for(det, (3, 2))
    got = det(images, targets, noise=noise)
    want = by_hand(det, images, targets, noise)
    assert set(got) == set(want) == set(weight_dict())
    for k in sorted(got):
        assert torch.equal(got[k], want[k]), (k, got[k].item(), want[k].item())
        assert torch.isfinite(got[k]), k
    assert any(got[k] != 0 for k in ("loss_class_dn", "loss_bbox_dn_0", "loss_giou_enc", "loss_salience"))


def test_backward_reaches_every_part():
    det = build().train()
    images, targets = batch()
    losses = det(images, targets, noise=noise_for(det, (3, 2)))
    sum(losses.values()).backward()
    params = dict(det.named_parameters())
    wanted = ["denoising_generator.label_encoder.weight", "transformer.tgt_embed.weight"]
    for part in ("transformer.decoder.layers.0.", "transformer.encoder.layers.0.", "neck.convs.0.", "transformer.enc_mask_predictor."):
        wanted.append(next(n for n, p in params.items() if n.startswith(part) and p.dim() >= 2))
    for n in wanted:
        g = params[n].grad
        assert g is not None, n
        assert torch.isfinite(g).all() and g.abs().max() > 0, n


def test_batch_without_targets_still_gives_the_embedding_a_gradient():
    det = build().train()
    images, _ = batch()
    empty = [{"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.long)} for _ in SIZES]
    losses = det(images, empty)
    assert set(losses) == set(weight_dict())
    assert all(torch.isfinite(v) for v in losses.values())
    assert all(losses[k] == 0 for k in losses if "_dn" in k or "bbox" in k or "giou" in k)
    sum(losses.values()).backward()
    g = det.denoising_generator.label_encoder.weight.grad
    assert g is not None and (g == 0).all()
    assert det.transformer.tgt_embed.weight.grad.abs().max() > 0       # the classification loss of the empty batch


def test_eval_mode_of_the_training_detector_is_the_eval_detector():
    det = build().eval()
    plain = build(training=False).eval()
    plain.load_state_dict(detector_state_dict(det.state_dict()))
    g = torch.Generator().manual_seed(5)
    images = [torch.rand(3, h, w, generator=g).cuda() for h, w in SIZES]
    got, want = det(images), plain(images)
    assert len(got) == len(want) == 2
    for a, b in zip(got, want):
        assert set(a) == set(b)
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert not any(t.requires_grad for d in got for t in d.values())
    # targets do not switch an eval-mode detector to the training branch
    _, targets = batch()
    again = det(images, targets)
    assert isinstance(again, list) and torch.equal(again[0]["scores"], got[0]["scores"])


def test_training_mode_without_targets_raises():
    det = build().train()
    images, _ = batch()
    with pytest.raises(RuntimeError, match="needs targets"):
        det(images)
    bad = [{"boxes": torch.tensor([[5.0, 5.0, 5.0, 9.0]]), "labels": torch.tensor([1])},
           {"boxes": torch.zeros(0, 4), "labels": torch.zeros(0, dtype=torch.long)}]
    with pytest.raises(RuntimeError, match="positive height and width"):
        det(images, bad)


class StoredBackbone(nn.Module):
    """Returns stored maps (the fixture's C3..C5), as the golden generator's stub backbone does."""

    def __init__(self, maps):
        super().__init__()
        self.maps = maps

    def forward(self, x):
        return {f"layer{i + 2}": m for i, m in enumerate(self.maps)}


def test_training_forward_matches_the_reference_detector():
    """The reference's own ``SalienceDETR.forward(images, targets)`` in ``train()`` mode (CPU, reduced dimensions, stub
    backbone with stored maps, inputs redrawn until every Hungarian assignment is unique with margin) against this
    detector on the same maps, targets, name-seeded weights and recorded noise.  Bar per weighted loss: the one
    tests/test_transformer_gpu.py applies to the loss of the ``transformer_train_small`` fixture,
    ``|got - want| < 2e-3 * max(1, |want|)``.  Measured on MI355X: worst key ``loss_class_dn`` at
    2.4e-7 of ``max(1, |want|)`` (8.071884 against 8.071886); five keys agree to the printed digits."""
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "detector_train_small.npz"))
    sizes = [tuple(int(v) for v in s) for s in d["image_sizes"]]
    counts = [int(c) for c in d["counts"]]
    assert sizes == SIZES
    tr = build_salience_transformer(embed_dim=256, num_heads=8, d_ffn=64, num_encoder_layers=2,
                                    num_decoder_layers=DEC_LAYERS, num_classes=C, topk_sa=6, max_num_embedding=20,
                                    two_stage_num_proposals=PROPOSALS, layer_filter_ratio=(1.0, 0.6))
    crit = HybridSetCriterion(C, HungarianMatcher(cost_class=2, cost_bbox=5, cost_giou=2), weight_dict())
    maps = [torch.from_numpy(d[f"map{i}"]).cuda() for i in range(3)]
    det = SalienceDETR(StoredBackbone(maps), ChannelMapper([m.shape[1] for m in maps], 256, 4),
                       PositionEmbeddingSine(128, 10000, True, offset=-0.5), tr, PostProcess(5), criterion=crit,
                       focus_criterion=SalienceCriterion(noise_scale=0.0), num_classes=C, num_queries=PROPOSALS,
                       denoising_nums=int(d["denoising_nums"]))
    from salience_detr_amd.detector import train_state_dict
    # the reference detector's keys (its stub backbone and criteria hold none), name-seeded values with the same salt
    reference_keys = d["sd_keys"].tolist()
    own = det.state_dict()
    sd = syn.det_state_dict({k: own[k] for k in reference_keys}, salt=int(d["salt"]))
    crc = [zlib.crc32(sd[k].contiguous().numpy().tobytes()) for k in sorted(sd)]
    assert sorted(sd) == reference_keys and crc == d["sd_crc"].tolist()
    det.load_state_dict(train_state_dict(sd))
    det = det.cuda().train()
    targets, o = [], 0
    for n in counts:
        targets.append({"boxes": torch.from_numpy(d["tboxes"][o:o + n]), "labels": torch.from_numpy(d["tlabels"][o:o + n]).long()})
        o += n
    groups = D.denoising_groups(int(d["denoising_nums"]), max(counts))
    noise = D.pack_noise(counts, groups, C, max(counts), torch.from_numpy(d["draw_flip"]), torch.from_numpy(d["draw_label"]),
                         torch.from_numpy(d["draw_sign"]), torch.from_numpy(d["draw_magnitude"])).cuda()
    images = [torch.zeros(3, h, w).cuda() for h, w in sizes]
    got = det(images, targets, noise=noise)
    want = dict(zip(d["loss_keys"].tolist(), d["loss_values"].tolist()))
    assert set(got) == set(want)
    rel = {k: abs(got[k].item() - want[k]) / max(1.0, abs(want[k])) for k in want}
    worst = max(rel, key=rel.get)
    for k in sorted(want):
        print(f"{k:20s} got {got[k].item():.6f} want {want[k]:.6f} rel {rel[k]:.2e}")
    print("worst key", worst, rel[worst])
    bad = {k: (got[k].item(), want[k]) for k in want if not abs(got[k].item() - want[k]) < 2e-3 * max(1.0, abs(want[k]))}
    assert not bad, bad
