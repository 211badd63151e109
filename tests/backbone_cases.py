"""Inputs of the backbone cases (row N0): shared by tests/golden/make_backbone_golden.py (which runs the imported
reference ``ResNet`` on them) and the tests.  Everything comes from ``synthetic.det_rand`` / ``det_state_dict``,
bit-identical on every machine."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from salience_detr_amd import synthetic as syn  # noqa: E402

# name -> (arch, return_indices, image sizes (h, w))
CASES = {
    "r50": ("resnet50", (1, 2, 3), [(64, 96), (50, 80)]),
    "r18": ("resnet18", (1, 2, 3), [(64, 96), (50, 80)]),
    "r50_5": ("resnet50", (0, 1, 2, 3), [(64, 96), (50, 80)]),
    "full": ("resnet50", (1, 2, 3), [(800, 1333), (800, 1066)]),
}
FULL_SIZE = ("full",)
SUB = 4096          # strided sub-sample length of a digested output
WHOLE_MAX = 30000   # outputs up to this many elements are stored whole
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def images(name):
    """The case's images: [3, h, w] float in [0, 1]."""
    return [syn.det_rand(f"backbone.{name}.img{i}", (3, h, w)) for i, (h, w) in enumerate(CASES[name][2])]


def canvas_and_mask(imgs):
    """The reference's eval pre-processing on the CPU: Normalize (sub, then div) per image, then pad with 0 to a
    multiple of 32 (``image_list_from_tensors(fill_value=0)``); the mask is True on padding."""
    h_pad, w_pad = syn.pad_to_32(max(i.shape[1] for i in imgs), max(i.shape[2] for i in imgs))
    canvas = torch.zeros(len(imgs), 3, h_pad, w_pad)
    mask = torch.ones(len(imgs), h_pad, w_pad, dtype=torch.bool)
    mean, std = torch.tensor(MEAN).view(3, 1, 1), torch.tensor(STD).view(3, 1, 1)
    for b, im in enumerate(imgs):
        canvas[b, :, :im.shape[1], :im.shape[2]] = (im - mean) / std
        mask[b, :im.shape[1], :im.shape[2]] = False
    return canvas, mask


def state(module_state, name):
    """Weights of a case: ``det_state_dict`` with the arch as salt (so the r50 cases share one weight set)."""
    return syn.det_state_dict(module_state, salt=len(CASES[name][0]))


def sub_index(numel):
    step = max(1, numel // SUB)
    return torch.arange(0, numel, step)[:SUB]


def sub_sample(t):
    return t.reshape(-1)[sub_index(t.numel())]
