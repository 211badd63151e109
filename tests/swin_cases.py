"""Inputs of the Swin backbone cases: shared by tests/golden/make_swin_golden.py (which runs the imported reference
``SwinTransformer`` on them) and the tests.  Everything comes from ``synthetic.det_rand`` / ``det_state_dict``,
bit-identical on every machine.  The cases are the smallest shapes that reach every code path, not the workload."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from salience_detr_amd import synthetic as syn  # noqa: E402
from backbone_cases import SUB, WHOLE_MAX, sub_index, sub_sample  # noqa: E402,F401

# name -> (SwinTransformer arguments, return_indices, input shape); num_heads = dim / 32 at every stage
CASES = {
    # maps 12 x 30 -> 6 x 15 -> 3 x 8 -> 2 x 4: the floor stem (50 is no multiple of 4), shift on both axes with both
    # paddings (12 x 30 pads to 14 x 35), shift off on one axis only (6 x 15 pads to 7 x 21), off on both (2 x 4 pads to
    # 7 x 7), odd-W and odd-H merging
    "w7": (dict(embed_dim=96, depths=(2, 2, 2, 2), num_heads=(3, 6, 12, 24), window_size=(7, 7)), (0, 1, 2, 3),
           (2, 3, 50, 120)),
    # maps 25 x 37 -> 13 x 19 -> 7 x 10 -> 4 x 5 with 144-token windows
    "w12": (dict(embed_dim=64, depths=(2, 2, 2, 2), num_heads=(2, 4, 8, 16), window_size=(12, 12)), (0, 1, 2, 3),
            (1, 3, 100, 150)),
    # the swin_l widths: maps 16 x 24 -> 8 x 12 -> 4 x 6 -> 2 x 3, 48 heads, the 4 C = 3072 merging LayerNorm
    "l": (dict(embed_dim=192, depths=(2, 2, 2, 2), num_heads=(6, 12, 24, 48), window_size=(7, 7)), (1, 2, 3),
          (1, 3, 64, 96)),
}


def config(name):
    """The ``SwinTransformer`` keyword arguments of the case (``patch_size`` and ``stochastic_depth_prob`` included)."""
    return dict(CASES[name][0], patch_size=(4, 4), stochastic_depth_prob=0.0)


def canvas(name):
    """The case's input ``[B, 3, H, W]``, normalised-image-like values."""
    return 2.0 * syn.det_rand(f"swin.{name}.canvas", CASES[name][2]) - 1.0


def state(module_state, name, salt=None):
    """Weights of a case: ``det_state_dict`` (salted by the case's name length unless ``salt`` is given).  Every
    ``relative_position_index`` stays as constructed (an index, not a weight); every ``relative_position_bias_table`` is
    ``2 * det_rand - 1`` so that the bias matters (the reference's 0.02 initialisation would hide it)."""
    salt = len(name) if salt is None else salt
    sd = syn.det_state_dict(module_state, salt=salt)
    for k in sd:
        if k.endswith("relative_position_index"):
            sd[k] = module_state[k].clone()
        elif k.endswith("relative_position_bias_table"):
            sd[k] = (2.0 * syn.det_rand(k, tuple(sd[k].shape), salt) - 1.0).to(sd[k].dtype)
    return sd
