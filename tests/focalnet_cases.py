"""Inputs of the FocalNet backbone cases: shared by tests/golden/make_focalnet_golden.py (which runs the imported
reference ``FocalNet`` + ``PostProcess`` on them) and the tests.  Everything comes from ``synthetic.det_rand`` /
``det_state_dict``, bit-identical on every machine.  The cases are the smallest shapes that reach every code path, not the
workload."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from salience_detr_amd import synthetic as syn  # noqa: E402
from backbone_cases import SUB, WHOLE_MAX, sub_index, sub_sample  # noqa: E402,F401

BIG = dict(use_conv_embed=True, use_postln=True, use_layerscale=True)
# name -> (FocalNet arguments, return_indices, input shape)
CASES = {
    # the focalnet_large_lrf_fl4 form at its widths 192 .. 1536; 50 x 77 is no multiple of 4: the stage maps are
    # 13 x 20 -> 7 x 10 -> 4 x 5 -> 2 x 3, so the pad-to-patch rule fires at the stem and at every down-sampler
    "fl4": (dict(embed_dim=192, depths=(1, 1, 2, 1), focal_levels=(4, 4, 4, 4), focal_windows=(3, 3, 3, 3),
                 normalize_modulator=True, **BIG), (1, 2, 3), (2, 3, 50, 77)),
    # the focalnet_tiny_srf form: 4 x 4 / 2 x 2 patchify, pre-LN, no layer scale
    "srf": (dict(embed_dim=96, depths=(2, 1, 1, 1), focal_levels=(2, 2, 2, 2), focal_windows=(3, 3, 3, 3)),
            (0, 1, 2, 3), (2, 3, 64, 96)),
    # the focalnet_huge_fl3 form: a LayerNorm inside the modulation, modulator not normalised
    "hg": (dict(embed_dim=64, depths=(1, 1, 1, 1), focal_levels=(3, 3, 3, 3), focal_windows=(3, 3, 3, 3),
                use_postln_in_modulation=True, **BIG), (2, 3), (1, 3, 45, 70)),
}


def config(name):
    """The ``FocalNet`` keyword arguments of the case (``patch_size`` and ``stochastic_depth_prob`` included)."""
    return dict(CASES[name][0], patch_size=(4, 4), stochastic_depth_prob=0.0)


def canvas(name):
    """The case's input ``[B, 3, H, W]``, normalised-image-like values."""
    return 2.0 * syn.det_rand(f"focalnet.{name}.canvas", CASES[name][2]) - 1.0


def state(module_state, name, salt=None):
    """Weights of a case: ``det_state_dict`` (salted by the case's name length unless ``salt`` is given), with every
    ``gamma_1`` / ``gamma_2`` set to ``0.1 + 0.2 * det_rand`` so that the branches matter (the reference's 1e-4
    initialisation would hide them)."""
    salt = len(name) if salt is None else salt
    sd = syn.det_state_dict(module_state, salt=salt)
    for k in sd:
        if k.endswith(("gamma_1", "gamma_2")):
            sd[k] = (0.1 + 0.2 * syn.det_rand(k, tuple(sd[k].shape), salt)).to(sd[k].dtype)
    return sd
