"""The Swin backbone's training cases (``SwinBackbone.set_train_form("hip")``): shared by
tests/golden/make_swin_train_golden.py (which runs the imported reference ``SwinTransformer``) and the tests.  Built on
tests/swin_cases.py and ``synthetic``: bit-identical on every machine.

Every case has ``return_indices=(1, 2, 3)``, ``freeze_indices=(0,)`` (the stem, stage 0 and its merging frozen),
``stochastic_depth_prob=0`` and the cotangents ``det_rand("swin_train.<case>.<map>", shape) - 0.5``.  The weights are
``swin_cases.state``'s, so the tables are +-1 and the bias matters.  The shapes are the smallest that reach every path:
  w7t   maps 12 x 30 -> 6 x 15 -> 3 x 8 -> 2 x 4: shift on both axes with both paddings, shift off on one axis, a window
        that is mostly padding, odd-H and odd-W merging;
  w12t  144-token windows, maps 25 x 37 -> 13 x 19 -> 7 x 10 -> 4 x 5;
  lt    the swin_l widths: 48 heads and the 4 C = 3072 merging LayerNorm."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import swin_cases as SC  # noqa: E402
from salience_detr_amd import synthetic as syn  # noqa: E402

# name -> (SwinTransformer arguments, input shape); num_heads = dim / 32 at every stage
CASES = {
    "w7t": (dict(embed_dim=96, depths=(1, 2, 2, 2), num_heads=(3, 6, 12, 24), window_size=(7, 7)), (2, 3, 50, 120)),
    "w12t": (dict(embed_dim=64, depths=(1, 2, 2, 2), num_heads=(2, 4, 8, 16), window_size=(12, 12)), (1, 3, 100, 150)),
    "lt": (dict(embed_dim=192, depths=(1, 2, 2, 1), num_heads=(6, 12, 24, 48), window_size=(7, 7)), (1, 3, 64, 96)),
}
RETURN = (1, 2, 3)
FREEZE = (0,)
SAMPLE = 1024   # gradient elements the reference's own distances d32 / dbf16 are measured on, as in convnext_train_cases
STORE = 160     # of which the fixture stores the first this many per tensor (it stays below convnext_train.npz)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swin_train.npz")


def config(case, stochastic_depth_prob=0.0):
    """The ``SwinTransformer`` keyword arguments of the case."""
    return dict(CASES[case][0], patch_size=(4, 4), stochastic_depth_prob=stochastic_depth_prob)


def canvas(case):
    return 2.0 * syn.det_rand(f"swin_train.{case}.canvas", CASES[case][1]) - 1.0


def state(module_state, case, salt=None):
    return SC.state(module_state, case, salt=salt)


def trainable_names(names):
    """The parameters ``freeze_indices=(0,)`` leaves trainable: everything from ``0.features.3`` on, in module order."""
    return [n for n in names if n.startswith("0.features.") and int(n.split(".")[2]) >= 3]


def run_features(features, x, num_stages=4):
    """The returned fp32 NCHW maps of a module tree's ``features`` (this project's or the reference's)."""
    outs = {}
    x = features[0](x)
    for i in range(num_stages):
        x = features[2 * i + 1](x)
        if i in RETURN:
            outs[f"features.{2 * i + 1}"] = x.permute(0, 3, 1, 2)
        if i < num_stages - 1:
            x = features[2 * i + 2](x)
    return outs


def cotangents(case, outs):
    return {k: syn.det_rand(f"swin_train.{case}.{k}", tuple(v.shape)) - 0.5 for k, v in outs.items()}


def torch_grads(features, x, names, case, dtype=torch.float64, autocast=None):
    """``{name: gradient (float64)}`` of sum(out * cotangent) over the returned maps, by torch autograd on the CPU."""
    params = {"0.features." + n: p for n, p in features.named_parameters()}
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


def sample_index(numel):
    """The elements the golden's ``d32`` / ``dbf16`` are measured on: whole up to ``SAMPLE``, else the strided sub-sample."""
    return torch.arange(numel) if numel <= SAMPLE else SC.sub_index(numel)[:SAMPLE]


def stored_index(numel):
    """The elements the golden stores: the first ``STORE`` of ``sample_index``."""
    return sample_index(numel)[:STORE]


def own_scale(got, ref, scale):
    """max|got - ref| on the stored elements over the whole tensor's max|ref|."""
    return (got - ref).abs().max().item() / (scale if scale > 0 else 1.0)
