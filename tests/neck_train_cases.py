"""The RepVGGPluX neck's training cases (``RepVGGPluXNetwork.set_train_form("hip")``): shared by
tests/golden/make_neck_train_golden.py (which runs the imported reference ``RepVGGPluXNetwork`` in ``train()`` mode) and
the tests.  Built on ``synthetic``: bit-identical on every machine.

Every input level requires grad, every parameter is trainable, the cotangents are ``det_rand("neck_train.<case>.out<l>",
shape) - 0.5`` and, after ``det_state_dict``, the BatchNorm weights ``ZERO_GAMMA`` of every norm are exactly 0.0 (a backward
that recovered the normalised map from the output would divide by them).  The shapes are the smallest that reach every path:
  c32   C = 32, groups 4 (8 per group), 3 levels, batch 2, maps 9 x 13 -> 5 x 7 -> 3 x 4: odd sizes, so the stride-2 3x3 and
        its backward meet both edges; the up-sampling ratios are not 2 (5 -> 9, 7 -> 13);
  g1    C = 16, groups 1, 2 levels, batch 1, maps 13 x 20 -> 7 x 10: 260 pixels, more than two pixel tiles with a ragged last
        one; the dense path runs through the grouped kernels;
  w256  C = 256, groups 4 (64 per group), 2 levels, batch 1, maps 6 x 8 -> 3 x 4: the real widths on maps smaller than a tile.
No level has fewer than 12 values per channel: below that the batch variance is ill-conditioned and the reference's own fp32
step becomes the noise."""
import os
import sys
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from backbone_cases import sub_index  # noqa: E402
from salience_detr_amd import synthetic as syn  # noqa: E402

# name -> (channels, groups, batch, maps (h, w) fine to coarse)
CASES = {
    "c32": (32, 4, 2, [(9, 13), (5, 7), (3, 4)]),
    "g1": (16, 1, 1, [(13, 20), (7, 10)]),
    "w256": (256, 4, 1, [(6, 8), (3, 4)]),
}
ZERO_GAMMA = (1, 6)   # channels of every BatchNorm whose weight is exactly 0.0
SAMPLE = 1024         # gradient elements the reference's own distance d32 is measured on
STORE = 160           # of which the fixture stores the first this many per tensor
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "neck_train.npz")


def build(cls, case):
    """A ``RepVGGPluXNetwork`` (this project's or the reference's: ``cls``) of the case, with the case's weights, in
    ``train()`` mode."""
    c, groups, _, maps = CASES[case]
    m = cls([c] * len(maps), [c] * len(maps), groups=groups)
    m.load_state_dict(state(m.state_dict(), case))
    return m.train()


def state(module_state, case):
    sd = syn.det_state_dict(module_state, salt=len(case))
    for k, v in sd.items():
        if k.endswith(".1.weight"):
            v[list(ZERO_GAMMA)] = 0.0
    return sd


def inputs(case):
    """The NCHW levels, fine to coarse."""
    c, _, batch, maps = CASES[case]
    return [syn.det_randn(f"neck_train.{case}.c{l}", (batch, c, h, w)) for l, (h, w) in enumerate(maps)]


def cotangents(case, outs):
    return [syn.det_rand(f"neck_train.{case}.out{l}", tuple(o.shape)) - 0.5 for l, o in enumerate(outs)]


def names(module, case):
    """The fixture's gradient names: the parameters in module order, then ``input.<l>``."""
    return [n for n, _ in module.named_parameters()] + [f"input.{l}" for l in range(len(CASES[case][3]))]


def stat_names(module):
    """The running statistics, in module order."""
    return [n for n, _ in module.named_buffers() if n.endswith(("running_mean", "running_var", "num_batches_tracked"))]


def run(forward, module, case, dtype=torch.float64):
    """One training forward + backward on the CPU: ``forward(list of NCHW maps) -> list of NCHW maps``.  Returns ``(outputs,
    {gradient name: tensor}, {statistic name: tensor})``, everything float64."""
    xs = [x.to(dtype).requires_grad_(True) for x in inputs(case)]
    outs = list(forward(xs))
    cots = cotangents(case, outs)
    loss = sum((o.double() * c.double()).sum() for o, c in zip(outs, cots))
    params = dict(module.named_parameters())
    grads = torch.autograd.grad(loss, list(params.values()) + xs)
    stats = {n: t.detach().double().clone() for n, t in module.named_buffers() if n in set(stat_names(module))}
    return ([o.detach().double() for o in outs], {n: g.double() for n, g in zip(names(module, case), grads)}, stats)


def reference_forward(module):
    """The reference's interface: an ordered dict of NCHW maps in and out."""
    return lambda xs: module(OrderedDict((str(l), x) for l, x in enumerate(xs))).values()


def sample_index(numel):
    """The elements the golden's ``d32`` is measured on: whole up to ``SAMPLE``, else the strided sub-sample."""
    return torch.arange(numel) if numel <= SAMPLE else sub_index(numel)[:SAMPLE]


def stored_index(numel):
    """The elements the golden stores: the first ``STORE`` of ``sample_index``."""
    return sample_index(numel)[:STORE]


def own_scale(got, ref, scale):
    """max|got - ref| on the given elements over the whole tensor's max|ref|."""
    return (got - ref).abs().max().item() / (scale if scale > 0 else 1.0)
