"""The backbone's training cases (``set_train_form("hip")``): shared by tests/golden/make_backbone_train_golden.py (which
runs the imported reference ``ResNet``) and the tests.  The cases are ``r18`` and ``r50`` of tests/backbone_cases.py with
``freeze_indices=(0,)``; the cotangents are ``det_rand("backbone_train.<case>.<layer>", shape) - 0.5``.

``walk`` is the masked restatement: the ResNet forward written over a module tree's own convs and norms (this project's
or the reference's: the attribute names are the same) with every ReLU either recorded (``masks=None``: ``relu`` runs and
its sign mask is appended to ``record``) or REPLACED by ``x * mask`` from the list, in forward order (stem first).  With
the masks as an input, two runs in different precisions differentiate the same piecewise-linear function, so their
gradients differ by rounding alone and not by the luck of a ReLU that changes side."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import backbone_cases as BC  # noqa: E402
from salience_detr_amd import synthetic as syn  # noqa: E402

CASES = ("r18", "r50")
FREEZE = (0,)
STORE = 1024    # gradient elements stored per tensor
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "backbone_train.npz")


def walk(net, x, num_stages, return_indices, masks=None, record=None):
    it = iter(masks) if masks is not None else None

    def act(t):
        if it is None:
            t = torch.relu(t)
            if record is not None:
                record.append(t.detach() > 0)
            return t
        return t * next(it).to(t.dtype)

    y = net.maxpool(act(net.bn1(net.conv1(x))))
    outs = {}
    for i in range(num_stages):
        for blk in getattr(net, f"layer{i + 1}"):
            identity = y if blk.downsample is None else blk.downsample(y)
            o = act(blk.bn1(blk.conv1(y)))
            if hasattr(blk, "conv3"):
                o = blk.bn3(blk.conv3(act(blk.bn2(blk.conv2(o)))))
            else:
                o = blk.bn2(blk.conv2(o))
            y = act(o + identity)
        if i in return_indices:
            outs[f"layer{i + 1}"] = y
    return outs


def trainable_names(net, num_stages):
    """Conv weights of layer2 .. (the stem and layer1 are frozen), in module order."""
    return [n for n, _ in net.named_parameters()
            if n.endswith("weight") and any(n.startswith(f"layer{i + 1}.") for i in range(1, num_stages))
            and (".conv" in n or ".downsample.0." in n)]


def cotangents(case, outs):
    return {k: syn.det_rand(f"backbone_train.{case}.{k}", tuple(v.shape)) - 0.5 for k, v in outs.items()}


def masked_grads(net, canvas, num_stages, return_indices, names, case, masks=None, record=None, dtype=torch.float64,
                 autocast=None):
    """``{name: gradient (float64)}`` of sum(out * cotangent) over the returned maps for the conv weights ``names``."""
    params = dict(net.named_parameters())
    for p in params.values():
        p.grad = None
    ws = [params[n] for n in names]
    x = canvas.to(dtype)
    if autocast is not None:
        with torch.autocast("cpu", dtype=autocast):
            outs = walk(net, x, num_stages, return_indices, masks, record)
    else:
        outs = walk(net, x, num_stages, return_indices, masks, record)
    cots = cotangents(case, outs)
    loss = sum((outs[k].double() * cots[k].double()).sum() for k in outs)
    grads = torch.autograd.grad(loss, ws)
    return {n: g.double() for n, g in zip(names, grads)}


def stored_index(numel):
    return torch.arange(numel) if numel <= STORE else BC.sub_index(numel)[:STORE]


def own_scale(got, ref, scale):
    """max|got - ref| on the stored elements over the whole tensor's max|ref|."""
    return (got - ref).abs().max().item() / (scale if scale > 0 else 1.0)


def pack_masks(masks):
    return np.packbits(torch.cat([m.reshape(-1) for m in masks]).numpy())


def unpack_masks(packed, shapes):
    bits = torch.from_numpy(np.unpackbits(packed)).bool()
    out, at = [], 0
    for s in shapes:
        n = int(np.prod(s))
        out.append(bits[at:at + n].reshape(tuple(s)))
        at += n
    return out
