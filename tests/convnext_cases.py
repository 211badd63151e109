"""Inputs of the ConvNeXt backbone cases: shared by tests/golden/make_convnext_golden.py (which runs the imported
reference ``ConvNeXt`` on them) and the tests.  Everything comes from ``synthetic.det_rand`` / ``det_state_dict``,
bit-identical on every machine.  The cases are the smallest shapes that reach every code path, not the workload."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from salience_detr_amd import synthetic as syn  # noqa: E402
from backbone_cases import SUB, WHOLE_MAX, canvas_and_mask, sub_index, sub_sample  # noqa: E402,F401

# name -> (widths, depths, return_indices, image sizes (h, w))
CASES = {
    "cnt": ((96, 192, 384, 768), (3, 3, 9, 3), (1, 2, 3), [(64, 96), (50, 80)]),       # the real conv_t setting
    "cnl": ((192, 384, 768, 1536), (1, 1, 2, 1), (1, 2, 3), [(64, 96), (50, 80)]),     # conv_l's widths (C = 1536 tile)
    "cnt4": ((96, 192, 384, 768), (1, 1, 1, 1), (0, 1, 2, 3), [(160, 224), (130, 200)]),  # ragged tiles, four outputs
}


def setting(name):
    """``[(input_channels, out_channels, num_layers), ...]`` of the case."""
    widths, depths = CASES[name][0], CASES[name][1]
    return [(widths[i], widths[i + 1] if i + 1 < len(widths) else None, depths[i]) for i in range(len(widths))]


def images(name):
    """The case's images: [3, h, w] float in [0, 1]."""
    return [syn.det_rand(f"convnext.{name}.img{i}", (3, h, w)) for i, (h, w) in enumerate(CASES[name][3])]


def state(module_state, name, salt=None):
    """Weights of a case: ``det_state_dict`` (salted by the case's name length unless ``salt`` is given), with every
    ``layer_scale`` set to ``0.1 + 0.2 * det_rand`` so that the residual branch matters and the activations do not grow
    through the depth."""
    salt = len(name) if salt is None else salt
    sd = syn.det_state_dict(module_state, salt=salt)
    for k in sd:
        if k.endswith("layer_scale"):
            sd[k] = (0.1 + 0.2 * syn.det_rand(k, tuple(sd[k].shape), salt)).to(sd[k].dtype)
    return sd
