"""The ChannelMapper's training cases (``ChannelMapper.set_train_form("hip")``): shared by
tests/golden/make_frontend_train_golden.py (which runs the imported reference ``ChannelMapper``) and the tests.  Built on
``synthetic``: bit-identical on every machine.

Every input requires grad, every parameter is trainable, the cotangents are ``det_rand("frontend_train.<case>.out<l>",
shape) - 0.5`` and, after ``det_state_dict``, GroupNorm weights ``ZERO_GAMMA`` of every level are exactly 0.0 (a backward
that recovered the normalised map from the output would divide by them).  The shapes are the smallest that reach every path:
  t4   (64, 128, 256) -> 64, 4 levels, 2 channels per group, maps 11 x 16, 6 x 8, 3 x 4 -> 2 x 2: odd sizes, so the
       stride-2 3x3 meets both edges;
  x2   (64, 96) -> 64, 4 levels, maps 9 x 13, 5 x 7 -> 3 x 4 -> 2 x 2: the second extra level reads the normalised first,
       whose GroupNorm backward takes the ``add`` path;
  g16  (64,) -> 48, 2 levels, 3 channels per group, maps 13 x 20 -> 7 x 10: 260 pixels, more than two 128-pixel tiles with
       a ragged last one;
  r50  (512, 1024, 2048) -> 256, the real widths, maps 8 x 10, 4 x 5, 2 x 3 -> 1 x 2: backward-weight over 9 x 2048."""
import os
import sys
from functools import partial

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from backbone_cases import sub_index  # noqa: E402
from salience_detr_amd import synthetic as syn  # noqa: E402

# name -> (in_channels, out_channels, num_outs, GroupNorm groups, batch, input maps (h, w))
CASES = {
    "t4": ((64, 128, 256), 64, 4, 32, 2, [(11, 16), (6, 8), (3, 4)]),
    "x2": ((64, 96), 64, 4, 32, 1, [(9, 13), (5, 7)]),
    "g16": ((64,), 48, 2, 16, 2, [(13, 20)]),
    "r50": ((512, 1024, 2048), 256, 4, 32, 1, [(8, 10), (4, 5), (2, 3)]),
}
ZERO_GAMMA = (1, 6)   # channels of every level's GroupNorm whose weight is exactly 0.0
SAMPLE = 1024         # gradient elements the reference's own distances d32 / dbf16 are measured on
STORE = 160           # of which the fixture stores the first this many per tensor
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_train.npz")


def build(cls, case):
    """A ``ChannelMapper`` (this project's or the reference's: ``cls``) of the case, with the case's weights."""
    cin, cout, num_outs, groups, _, _ = CASES[case]
    m = cls(list(cin), cout, num_outs, norm_layer=partial(nn.GroupNorm, groups))
    m.load_state_dict(state(m.state_dict(), case))
    return m


def state(module_state, case, salt=None):
    sd = syn.det_state_dict(module_state, salt=len(case) if salt is None else salt)
    for k, v in sd.items():
        if k.endswith(".1.weight"):
            v[list(ZERO_GAMMA)] = 0.0
    return sd


def inputs(case):
    cin, _, _, _, batch, maps = CASES[case]
    return [syn.det_randn(f"frontend_train.{case}.c{l}", (batch, c, h, w)) for l, (c, (h, w)) in enumerate(zip(cin, maps))]


def cotangents(case, outs):
    return [syn.det_rand(f"frontend_train.{case}.out{l}", tuple(o.shape)) - 0.5 for l, o in enumerate(outs)]


def names(module, case):
    """The fixture's names: the trainable parameters in module order, then ``input.<l>``."""
    return [n for n, _ in module.named_parameters()] + [f"input.{l}" for l in range(len(CASES[case][0]))]


def torch_grads(module, case, dtype=torch.float64, autocast=None):
    """``{name: gradient (float64)}`` of sum(out * cotangent) over the levels, by torch autograd on the CPU; ``module``
    takes the maps as a dict, as the reference does."""
    xs = [x.to(dtype).requires_grad_(True) for x in inputs(case)]
    feats = {str(l): x for l, x in enumerate(xs)}
    if autocast is not None:
        with torch.autocast("cpu", dtype=autocast):
            outs = module(feats)
    else:
        outs = module(feats)
    cots = cotangents(case, outs)
    loss = sum((o.double() * c.double()).sum() for o, c in zip(outs, cots))
    params = dict(module.named_parameters())
    grads = torch.autograd.grad(loss, list(params.values()) + xs)
    return {n: g.double() for n, g in zip(names(module, case), grads)}


def sample_index(numel):
    """The elements the golden's ``d32`` / ``dbf16`` are measured on: whole up to ``SAMPLE``, else the strided sub-sample."""
    return torch.arange(numel) if numel <= SAMPLE else sub_index(numel)[:SAMPLE]


def stored_index(numel):
    """The elements the golden stores: the first ``STORE`` of ``sample_index``."""
    return sample_index(numel)[:STORE]


def own_scale(got, ref, scale):
    """max|got - ref| on the given elements over the whole tensor's max|ref|."""
    return (got - ref).abs().max().item() / (scale if scale > 0 else 1.0)
