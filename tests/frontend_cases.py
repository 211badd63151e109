"""Inputs of the input-stage cases (row N7): shared by tests/golden/make_frontend_golden.py (which runs the imported
reference on them) and the tests.  Everything comes from ``synthetic.det_randn`` / ``det_state_dict``, bit-identical on
every machine."""
import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from salience_detr_amd import synthetic as syn  # noqa: E402

# name -> (in_channels, out_channels, num_outs, backbone strides, image sizes (h, w))
MAPPER_CASES = {
    "reduced": ((64, 128, 256), 64, 4, (8, 16, 32), [(90, 130), (70, 100)]),
    "r50": ((512, 1024, 2048), 256, 4, (8, 16, 32), [(160, 224), (150, 200)]),
    "five": ((256, 512, 1024, 2048), 256, 4, (4, 8, 16, 32), [(64, 96), (50, 90)]),
    "swin": ((384, 768, 1536), 256, 5, (8, 16, 32), [(96, 128), (80, 120)]),
    "full": ((512, 1024, 2048), 256, 4, (8, 16, 32), [(800, 1333), (800, 1066)]),
}
FULL_SIZE = ("full",)
SUB = 4096   # strided sub-sample length of a digested output


def canvas_mask(image_sizes):
    h_pad, w_pad = syn.pad_to_32(max(s[0] for s in image_sizes), max(s[1] for s in image_sizes))
    mask = torch.ones(len(image_sizes), h_pad, w_pad, dtype=torch.bool)
    for i, (h, w) in enumerate(image_sizes):
        mask[i, :h, :w] = False
    return mask


def backbone_shapes(h_pad, w_pad, strides):
    return [(math.ceil(h_pad / s), math.ceil(w_pad / s)) for s in strides]


def mapper_inputs(name):
    """(state-dict rule, backbone feature list, padded image mask) of a mapper case."""
    cin, _, _, strides, sizes = MAPPER_CASES[name]
    mask = canvas_mask(sizes)
    shapes = backbone_shapes(mask.shape[1], mask.shape[2], strides)
    feats = [syn.det_randn(f"frontend.{name}.c{l}", (len(sizes), c, h, w)) for l, (c, (h, w)) in enumerate(zip(cin, shapes))]
    return feats, mask


def mapper_state(module_state, name):
    return syn.det_state_dict(module_state, salt=len(name))


def extra_shapes(shapes, num_outs):
    out = list(shapes)
    while len(out) < num_outs:
        h, w = out[-1]
        out.append(((h - 1) // 2 + 1, (w - 1) // 2 + 1))
    return out


def blob_mask():
    """A non-rectangular padding mask: two images, discs and stripes of padding."""
    B, H, W = 2, 72, 104
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    m0 = ((yy - 20) ** 2 + (xx - 30) ** 2 < 15 ** 2) | (xx > 90)
    m1 = ((yy - 50) ** 2 + (xx - 70) ** 2 < 20 ** 2) | ((yy.long() % 7) == 3) | (yy > 66)
    return torch.stack([m0, m1])


# name -> (PositionEmbeddingSine kwargs, mask source, level shapes)
POSITION_CASES = {
    "config_r50": (dict(num_pos_feats=128, temperature=10000, normalize=True, offset=-0.5), "r50", None),
    "config_full": (dict(num_pos_feats=128, temperature=10000, normalize=True, offset=-0.5), "full", None),
    "unnormalized": (dict(num_pos_feats=64, temperature=10000, normalize=False), "reduced", None),
    "tuple_temperature": (dict(num_pos_feats=32, temperature=(10000, 20), normalize=True, offset=-0.5), "reduced", None),
    "blob": (dict(num_pos_feats=128, temperature=10000, normalize=True, offset=-0.5), "blob",
             [(72, 104), (36, 52), (18, 26), (9, 13), (5, 7), (25, 40)]),
}


def position_inputs(name):
    """(module kwargs, padded mask [B, H, W] bool, level shapes) of a position case."""
    kw, src, shapes = POSITION_CASES[name]
    if src == "blob":
        return kw, blob_mask(), shapes
    cin, _, num_outs, strides, sizes = MAPPER_CASES[src]
    mask = canvas_mask(sizes)
    return kw, mask, extra_shapes(backbone_shapes(mask.shape[1], mask.shape[2], strides), num_outs)


def reference_level_mask(mask, shape):
    return F.interpolate(mask[None].float(), size=tuple(shape)).to(torch.bool)[0]


def sub_sample(t, n=SUB):
    flat = t.reshape(-1)
    idx = torch.linspace(0, flat.numel() - 1, min(n, flat.numel())).round().long()
    return flat[idx]


def channel_sums(t):
    """[B, C] float64 sums over pixels of a [B, C, H, W] map."""
    return t.double().sum((2, 3))
