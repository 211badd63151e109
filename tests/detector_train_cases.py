"""Shared by tests/test_detector_train_cpu.py and tests/test_detector_train_gpu.py: the fixtures the imported reference
``SalienceDETR`` left of one training step each (tests/golden/detector_train_<tag>.npz, made by
tests/golden/make_detector_train_golden.py) and this project's detector built on a fixture's stored maps and name-seeded
weights.  Nothing here needs a GPU; the GPU tests move the detector over themselves."""
import os
import zlib

import numpy as np
import torch
from torch import nn

from salience_detr_amd import denoising as D
from salience_detr_amd import synthetic as syn
from salience_detr_amd.channel_mapper import ChannelMapper
from salience_detr_amd.detector import SalienceDETR, train_state_dict
from salience_detr_amd.position_encoding import PositionEmbeddingSine
from salience_detr_amd.post_process import PostProcess
from salience_detr_amd.salience_criterion import SalienceCriterion
from salience_detr_amd.salience_transformer import build_salience_transformer
from salience_detr_amd.set_criterion import HungarianMatcher, HybridSetCriterion

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# counts (3, 2); (0, 4): an image without targets next to one with four; (5, 1) at denoising_nums = 3: one denoising group
TAGS = ["small", "empty_first", "groups_one"]
C, PROPOSALS, DEC_LAYERS, ENC_LAYERS = 7, 10, 2, 2
SIZES = [(64, 96), (48, 80)]


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


class StoredBackbone(nn.Module):
    """Returns stored maps (the fixture's C3..C5), as the golden generator's stub backbone does."""

    def __init__(self, maps):
        super().__init__()
        self.maps = maps

    def forward(self, x):
        return {f"layer{i + 2}": m for i, m in enumerate(self.maps)}


class Case:
    def __init__(self, tag):
        self.tag = tag
        self.d = d = np.load(os.path.join(GOLDEN, f"detector_train_{tag}.npz"))
        self.sizes = [tuple(int(v) for v in s) for s in d["image_sizes"]]
        self.counts = [int(c) for c in d["counts"]]
        self.denoising_nums = int(d["denoising_nums"])
        self.max_gt = max(self.counts)
        self.groups = D.denoising_groups(self.denoising_nums, self.max_gt)
        self.losses = dict(zip(d["loss_keys"].tolist(), d["loss_values"].tolist()))

    def targets(self):
        """xyxy pixels, as the detector's ``forward(images, targets)`` takes them."""
        out, o = [], 0
        for n in self.counts:
            out.append({"boxes": torch.from_numpy(self.d["tboxes"][o:o + n]).reshape(-1, 4),
                        "labels": torch.from_numpy(self.d["tlabels"][o:o + n]).long()})
            o += n
        return out

    def noise(self):
        """The reference's recorded draws as the generator's noise tensor (host)."""
        d = self.d
        return D.pack_noise(self.counts, self.groups, C, self.max_gt, torch.from_numpy(d["draw_flip"]),
                            torch.from_numpy(d["draw_label"]), torch.from_numpy(d["draw_sign"]),
                            torch.from_numpy(d["draw_magnitude"]))

    def detector(self, maps):
        """This project's training detector (host) on ``maps`` as its backbone's output, holding the reference
        detector's weights: its keys (the reference's stub backbone and criteria hold none), name-seeded values with the
        fixture's salt, checked against the fixture's checksums."""
        d = self.d
        tr = build_salience_transformer(embed_dim=256, num_heads=8, d_ffn=64, num_encoder_layers=ENC_LAYERS,
                                        num_decoder_layers=DEC_LAYERS, num_classes=C, topk_sa=6, max_num_embedding=20,
                                        two_stage_num_proposals=PROPOSALS, layer_filter_ratio=(1.0, 0.6))
        crit = HybridSetCriterion(C, HungarianMatcher(cost_class=2, cost_bbox=5, cost_giou=2), weight_dict())
        det = SalienceDETR(StoredBackbone(maps), ChannelMapper([m.shape[1] for m in maps], 256, 4),
                           PositionEmbeddingSine(128, 10000, True, offset=-0.5), tr, PostProcess(5), criterion=crit,
                           focus_criterion=SalienceCriterion(noise_scale=0.0), num_classes=C, num_queries=PROPOSALS,
                           denoising_nums=self.denoising_nums)
        reference_keys = d["sd_keys"].tolist()
        own = det.state_dict()
        sd = syn.det_state_dict({k: own[k] for k in reference_keys}, salt=int(d["salt"]))
        crc = [zlib.crc32(sd[k].contiguous().numpy().tobytes()) for k in sorted(sd)]
        assert sorted(sd) == reference_keys and crc == d["sd_crc"].tolist()
        det.load_state_dict(train_state_dict(sd))
        return det

    def stored_maps(self):
        return [torch.from_numpy(self.d[f"map{i}"]) for i in range(3)]

    def stored(self, g):
        """A gradient as the fixture stores it: whole when small, every ``sub_step``-th row / column of big matrices."""
        step = int(self.d["sub_step"])
        return g[::step, ::step] if g.numel() > int(self.d["sub_above"]) and g.dim() >= 2 else g
