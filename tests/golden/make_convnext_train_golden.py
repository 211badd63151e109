"""tests/golden/convnext_train.npz: the training gradients of the reference ConvNeXt backbone, run on the CPU by the
IMPORTED reference ``ConvNeXt`` (loaded as tests/golden/make_convnext_golden.py loads it) on the cases of
tests/convnext_train_cases.py.  ``stochastic_depth_prob`` is 0, with which ``train()`` and ``eval()`` compute the same
function (the reference has no other mode-dependent layer), so the stub ``StochasticDepth`` of that loader serves.

Stored per case ``<case>.*``: ``names`` (the trainable parameters, ``freeze_indices=(0,)``); per parameter ``g:<name>``
(the float64 gradient, whole up to 1024 elements, else the strided sub-sample ``backbone_cases.sub_index`` cut to 1024),
``norm:<name>`` and ``max:<name>`` (L2 norm and max abs of the whole float64 gradient), ``d32:<name>`` / ``dbf16:<name>``:
the own-scale distance (max|g - ref| on the stored elements / max|ref|) of the reference's fp32 run and of its
``torch.autocast("cpu", bfloat16)`` run from the float64 gradient.

Run from the repository root: ``python tests/golden/make_convnext_train_golden.py`` (needs the reference checkout).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import convnext_train_cases as TC  # noqa: E402
from make_convnext_golden import load_reference_convnext  # noqa: E402


def main():
    mod = load_reference_convnext()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    data = {}
    for case in TC.CASES:
        net = mod.ConvNeXt(block_setting=[mod.CNBlockConfig(*row) for row in TC.setting(case)]).eval()
        keys = [k for k in net.state_dict() if k.startswith("features.")]
        net.load_state_dict(TC.state({k: net.state_dict()[k] for k in keys}, case), strict=False)
        names = TC.trainable_names([n for n, _ in net.named_parameters()])
        canvas = TC.canvas()
        ref = TC.torch_grads(net.double().features, canvas, names, case)
        g32 = TC.torch_grads(net.float().features, canvas, names, case, dtype=torch.float32)
        gbf = TC.torch_grads(net.features, canvas, names, case, dtype=torch.float32, autocast=torch.bfloat16)
        data[f"{case}.names"] = np.array(names)
        for n in names:
            idx = TC.stored_index(ref[n].numel())
            pick = lambda t: t.reshape(-1)[idx]
            scale = ref[n].abs().max().item()
            data[f"{case}.g:{n}"] = pick(ref[n]).numpy()
            data[f"{case}.norm:{n}"] = np.float64(ref[n].norm().item())
            data[f"{case}.max:{n}"] = np.float64(scale)
            data[f"{case}.d32:{n}"] = np.float64(TC.own_scale(pick(g32[n]), pick(ref[n]), scale))
            data[f"{case}.dbf16:{n}"] = np.float64(TC.own_scale(pick(gbf[n]), pick(ref[n]), scale))
        d32 = [data[f"{case}.d32:{n}"] for n in names]
        dbf = [data[f"{case}.dbf16:{n}"] for n in names]
        print(case, len(names), "parameters; d32 %.2e .. %.2e, dbf16 %.2e .. %.2e" % (min(d32), max(d32), min(dbf), max(dbf)),
              flush=True)
    np.savez_compressed(TC.GOLDEN, **data)
    print(TC.GOLDEN, os.path.getsize(TC.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
