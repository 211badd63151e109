"""The ConvNeXt backbone's training cases (``ConvNeXtBackbone.set_train_form("hip")``): shared by
tests/golden/make_convnext_train_golden.py (which runs the imported reference ``ConvNeXt``) and the tests.  Built on
tests/convnext_cases.py and ``synthetic``: bit-identical on every machine.

Both cases take the two images of ``convnext_cases`` "cnt" on one canvas, ``return_indices=(1, 2, 3)``,
``freeze_indices=(0,)`` (the stem, stage 0 and its down-sampler frozen) and the cotangents
``det_rand("convnext_train.<case>.<map>", shape) - 0.5``."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import convnext_cases as CC  # noqa: E402
from salience_detr_amd import synthetic as syn  # noqa: E402

# name -> (widths, depths)
CASES = {
    "ct1": ((96, 192, 384, 768), (1, 2, 2, 1)),
    "ct2": ((192, 384, 768, 1536), (1, 1, 2, 1)),     # conv_l's widths
}
RETURN = (1, 2, 3)
FREEZE = (0,)
IMAGES = "cnt"
STORE = 1024    # gradient elements stored per tensor
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convnext_train.npz")


def setting(case):
    """``[(input_channels, out_channels, num_layers), ...]`` of the case."""
    widths, depths = CASES[case]
    return [(widths[i], widths[i + 1] if i + 1 < len(widths) else None, depths[i]) for i in range(len(widths))]


def canvas():
    return CC.canvas_and_mask(CC.images(IMAGES))[0]


def state(module_state, case):
    return CC.state(module_state, case)


def trainable_names(names):
    """The parameters ``freeze_indices=(0,)`` leaves trainable: everything from ``features.3`` on, in module order."""
    return [n for n in names if n.startswith("features.") and int(n.split(".")[1]) >= 3]


def run_features(features, x, num_stages=4):
    """The returned maps of a module tree's ``features`` (this project's or the reference's)."""
    outs = {}
    for idx in range(2 * num_stages):
        x = features[idx](x)
        if idx % 2 == 1 and idx // 2 in RETURN:
            outs[f"features.{idx}"] = x
    return outs


def cotangents(case, outs):
    return {k: syn.det_rand(f"convnext_train.{case}.{k}", tuple(v.shape)) - 0.5 for k, v in outs.items()}


def torch_grads(features, x, names, case, dtype=torch.float64, autocast=None):
    """``{name: gradient (float64)}`` of sum(out * cotangent) over the returned maps, by torch autograd on the CPU."""
    params = {"features." + n: p for n, p in features.named_parameters()}
    x = x.to(dtype)
    if autocast is not None:
        with torch.autocast("cpu", dtype=autocast):
            outs = run_features(features, x)
    else:
        outs = run_features(features, x)
    cots = cotangents(case, outs)
    loss = sum((outs[k].double() * cots[k].double()).sum() for k in outs)
    grads = torch.autograd.grad(loss, [params[n] for n in names])
    return {n: g.double() for n, g in zip(names, grads)}


def stored_index(numel):
    return torch.arange(numel) if numel <= STORE else CC.sub_index(numel)[:STORE]


def own_scale(got, ref, scale):
    """max|got - ref| on the stored elements over the whole tensor's max|ref|."""
    return (got - ref).abs().max().item() / (scale if scale > 0 else 1.0)
