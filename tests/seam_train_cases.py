"""The backbone-to-neck training cases: a backbone and a ``ChannelMapper`` trained together, in every pair of training
forms (``set_train_form`` of either module).  Shared by tests/test_seam_train_cpu.py and tests/test_seam_train_gpu.py.
Everything is built on ``synthetic`` (bit-identical on every machine) and on this project's own torch composites: no
fixture and nothing of the reference project is involved.

Backbones (the small configurations of the detector tests, ``return_indices=(1, 2, 3)``, ``freeze_indices=(0,)``, no
stochastic depth): ``resnet`` (resnet18, widths 128 / 256 / 512), ``convnext`` (``convnext_cases`` "cnt4": 192 / 384 /
768), ``swin`` (embed_dim 32, 7 x 7 windows: 64 / 128 / 256) and ``focalnet`` (``focalnet_cases`` "hg", the smallest: 128 /
256 / 512; it has no HIP backward, so it trains in its torch form only).
Neck: ``ChannelMapper(num_channels, 64, 4, GroupNorm(32))``: two extra levels, so the last backbone map receives the sum
of two backward-data results and the second extra level's GroupNorm backward takes the ``add`` path; its weights are
``frontend_train_cases.state`` (name-seeded, GroupNorm weights ``ZERO_GAMMA`` exactly 0.0).
Input: one ``det_randn`` canvas ``[2, 3, 96, 160]``: maps 12 x 20, 6 x 10, 3 x 5 -> 2 x 3 -> 1 x 2, odd somewhere at every
level, so the stride-2 3x3 meets both edges.  Loss: ``sum_l (out_l * cot_l).sum()`` with ``cot_l = det_rand - 0.5``.

Reference (``reference(name)``, computed once per process): ``copy.deepcopy`` of both modules, ``.double()``, on the CPU,
``neck.forward_torch(backbone.forward_torch(canvas))`` and ``torch.autograd.grad`` for every trainable parameter of both
modules (``backbone.<n>``, ``neck.<n>``) and for the three seam maps (``seam.<l>``: what the neck hands the backbone,
with the graph cut at the seam -- see ``torch_grads``).
Yardsticks, measured on the reference side only: ``d32``, the same composites in fp32, and ``dbf16``, the fp32 copies
under ``torch.autocast("cpu", torch.bfloat16)``, each against float64.  ``distance`` gives both measures of a tensor,
compared whole: max|got - ref| over the whole tensor's max|ref| (``own``) and the relative difference of the L2 norms
(``norm``).  ``d32`` / ``dbf16`` hold the ``own`` measure, the yardstick of the per-module training tests; ``d32_norm`` /
``dbf16_norm`` the other one, for the record.
"""
import copy
import os
import sys
from functools import partial

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import backbone_cases as BC  # noqa: E402
import backbone_train_cases as BT  # noqa: E402
import convnext_cases as CC  # noqa: E402
import focalnet_cases as FC  # noqa: E402
import frontend_train_cases as FT  # noqa: E402
import swin_cases as SC  # noqa: E402
from salience_detr_amd import synthetic as syn  # noqa: E402
from salience_detr_amd.backbone import ResNetBackbone  # noqa: E402
from salience_detr_amd.channel_mapper import ChannelMapper  # noqa: E402
from salience_detr_amd.convnext import CNBlockConfig, ConvNeXtBackbone  # noqa: E402
from salience_detr_amd.focalnet import FocalNetBackbone  # noqa: E402
from salience_detr_amd.swin import SwinBackbone  # noqa: E402

HIP_BACKBONES = ("resnet", "convnext", "swin")     # the backbones with a HIP backward
BACKBONES = HIP_BACKBONES + ("focalnet",)
RETURN, FREEZE = (1, 2, 3), (0,)
CANVAS = (2, 3, 96, 160)
MAPS = [(12, 20), (6, 10), (3, 5)]                 # the three backbone maps; the neck adds 2 x 3 and 1 x 2
OUT_CHANNELS, NUM_OUTS, GROUPS = 64, 4, 32
SWIN = dict(embed_dim=32, depths=(1, 2, 2, 1), num_heads=(1, 2, 4, 8), window_size=(7, 7), stochastic_depth_prob=0.0)
FOCALNET = "hg"


def build_backbone(name):
    """The backbone ``name`` with its family's name-seeded weights: on the CPU, fp32, ``train()`` mode."""
    if name == "resnet":
        m = ResNetBackbone("resnet18", return_indices=RETURN, freeze_indices=FREEZE)
        m.load_state_dict(BC.state(m.state_dict(), "r18"))
    elif name == "convnext":
        m = ConvNeXtBackbone(None, return_indices=RETURN, freeze_indices=FREEZE,
                             block_setting=[CNBlockConfig(*r) for r in CC.setting("cnt4")])
        m.load_state_dict(CC.state(m.state_dict(), "cnt4"))
    elif name == "swin":
        m = SwinBackbone(None, return_indices=RETURN, freeze_indices=FREEZE, **SWIN)
        m.load_state_dict(SC.state(m.state_dict(), "det"))
    elif name == "focalnet":
        m = FocalNetBackbone(None, return_indices=RETURN, freeze_indices=FREEZE, **FC.config(FOCALNET))
        m.load_state_dict(FC.state(m.state_dict(), FOCALNET))
    else:
        raise KeyError(name)
    return m.train()


def build_neck(backbone):
    m = ChannelMapper(list(backbone.num_channels), OUT_CHANNELS, NUM_OUTS, norm_layer=partial(nn.GroupNorm, GROUPS))
    m.load_state_dict(FT.state(m.state_dict(), "seam"))
    return m.train()


def canvas():
    return syn.det_randn("seam_train.canvas", CANVAS)


def level_shapes(batch=CANVAS[0]):
    shapes = list(MAPS)
    for _ in range(NUM_OUTS - len(MAPS)):
        shapes.append(((shapes[-1][0] - 1) // 2 + 1, (shapes[-1][1] - 1) // 2 + 1))
    return [(batch, OUT_CHANNELS, h, w) for h, w in shapes]


def cotangents():
    return [syn.det_rand(f"seam_train.out{l}", shape) - 0.5 for l, shape in enumerate(level_shapes())]


def trainable(backbone, neck):
    """``[(name, parameter)]`` of both modules' trainable parameters: ``backbone.<n>`` in module order, then ``neck.<n>``."""
    return ([("backbone." + n, p) for n, p in backbone.named_parameters() if p.requires_grad]
            + [("neck." + n, p) for n, p in neck.named_parameters() if p.requires_grad])


def seam_names():
    return [f"seam.{l}" for l in range(len(MAPS))]


def masked_resnet_forward(masks):
    """The ResNet composite with every ReLU replaced by ``x * mask`` (``backbone_train_cases.walk``; ``masks`` in forward
    order, stem first), as a ``forward`` of ``torch_grads``: runs in different precisions then differentiate the same
    piecewise-linear function, and a pre-activation within rounding of zero cannot put them on different sides."""
    def forward(backbone, x):
        return BT.walk(backbone, x, backbone.num_stages, backbone.return_indices, masks=masks)
    return forward


def torch_grads(backbone, neck, x, cots, dtype=torch.float64, autocast=None, forward=None):
    """``{name: gradient (float64)}`` of the loss for ``trainable(backbone, neck)`` and the three seam maps, by torch
    autograd over the two torch composites on the CPU; the modules are converted to ``dtype`` in place.  The graph is cut
    at the seam: ``seam.<l>`` is the neck's gradient for its input ``l`` alone -- the cotangent a backbone node receives --
    and not the map's total gradient (in the torch composite a map also feeds the next stage); the backbone's parameters
    get theirs from those three cotangents, which is the chain rule written out.  ``forward(backbone, x)`` replaces
    ``backbone.forward_torch(x)`` where given."""
    backbone.to(dtype), neck.to(dtype)

    def run():
        maps = list((backbone.forward_torch(x.to(dtype)) if forward is None else forward(backbone, x.to(dtype))).values())
        leaves = [m.detach().requires_grad_(True) for m in maps]
        return maps, leaves, neck.forward_torch(leaves)
    if autocast is not None:
        with torch.autocast("cpu", dtype=autocast):
            maps, leaves, outs = run()
    else:
        maps, leaves, outs = run()
    assert [tuple(o.shape) for o in outs] == [tuple(c.shape) for c in cots]
    loss = sum((o.double() * c.double()).sum() for o, c in zip(outs, cots))
    named = trainable(backbone, neck)
    below = [(n, p) for n, p in named if n.startswith("backbone.")]
    above = [(n, p) for n, p in named if n.startswith("neck.")]
    upper = torch.autograd.grad(loss, [p for _, p in above] + leaves)
    seam = list(upper[len(above):])
    lower = torch.autograd.grad(maps, [p for _, p in below], grad_outputs=seam)
    names = [n for n, _ in below] + [n for n, _ in above] + seam_names()
    return {n: g.double() for n, g in zip(names, list(lower) + list(upper))}


def distance(got, ref):
    """``(own, norm)`` of the whole tensor: max|got - ref| / max|ref| and | ||got|| - ||ref|| | / ||ref||."""
    got, ref = got.detach().cpu().double(), ref.double()
    scale, norm = ref.abs().max().item(), ref.norm().item()
    return ((got - ref).abs().max().item() / (scale if scale > 0 else 1.0),
            abs(got.norm().item() - norm) / (norm if norm > 0 else 1.0))


def yardsticks(backbone, neck, x, cots, forward=None):
    """The float64 gradients of a CPU fp32 pair and the reference's own distances from them:
    ``{"g64", "g32", "d32", "d32_norm", "dbf16", "dbf16_norm"}``, each ``{name: ...}``.  The pair is left in fp32."""
    backbone, neck = copy.deepcopy(backbone), copy.deepcopy(neck)
    g64 = torch_grads(backbone, neck, x, cots, torch.float64, forward=forward)
    g32 = torch_grads(backbone, neck, x, cots, torch.float32, forward=forward)
    gbf = torch_grads(backbone, neck, x, cots, torch.float32, autocast=torch.bfloat16, forward=forward)
    out = {"g64": g64, "g32": g32, "d32": {}, "d32_norm": {}, "dbf16": {}, "dbf16_norm": {}}
    for n, ref in g64.items():
        out["d32"][n], out["d32_norm"][n] = distance(g32[n], ref)
        out["dbf16"][n], out["dbf16_norm"][n] = distance(gbf[n], ref)
    return out


_reference = {}


def reference(name):
    """``yardsticks`` of the case's own pair, canvas and cotangents; computed once per process, to be left unchanged."""
    if name not in _reference:
        backbone = build_backbone(name)
        _reference[name] = yardsticks(backbone, build_neck(backbone), canvas(), cotangents())
    return _reference[name]
