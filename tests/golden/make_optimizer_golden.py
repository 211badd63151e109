"""Generate tests/golden/optimizer_cases.npz: what the reference's optimizer lines do, as data.

Run in the authoring container only (needs the upstream reference checkout, see _ref_import.py):

    python tests/golden/make_optimizer_golden.py

Groups.  The reference's three ``optimizer/param_dict.py`` functions run on a reference-side module tree: the reference
detector as make_detector_train_golden.py builds it, its backbone replaced by a stub that registers convolution, norm and
bias parameters under ResNet key names.  Per policy (``POLICIES``: this project's policy name -> the reference function)
the file keeps the parameter names in model order (``model_names``) and in group order (``groups.<policy>.names``), each name's group index and the group's
effective ``lr`` / ``weight_decay`` under ``AdamW(lr=1e-4, weight_decay=1e-4)``.

Trajectories.  ``STEPS`` steps of the reference's own sequence (util/engine.py:56-61): ``clip_grad_norm_(0.1)``,
``torch.optim.AdamW.step()``, ``LinearLR(start_factor=1/1000)`` stepping per iteration of the first epoch (three
iterations: ``total_iters = 2``), and ``MultiStepLR(milestones=[1], gamma=0.1)`` stepping at the end of each epoch, so the
decay falls inside the run.  It runs on CPU in float64 and again in float32 from the same fp32-drawn parameters and
gradients.  Nothing drawn is stored: parameter i starts as ``det_randn("opt.p.<i>", shape) * 3`` and its gradient at
step k is ``det_randn("opt.g.<k>.<i>", shape) * grad_scale[i] * step_scale[k]``, with the exceptions the file lists
(``none_grad``: (step, tensor) without a gradient; ``zero_grad``: (step, tensor) whose gradient is all zero).
Stored per step and tensor: the float64 parameter and both moments (tensors above ``SAMPLE_ABOVE`` elements as
``flat[::stride]``, ``strides`` in the file), the float64 total norm, and ``d_ref``: max |float32 run - float64 run| over
the stored elements (``d_ref_norm``: relative).  ``lrs[k, group]`` is the learning rate step k ran with.
"""
import os
import sys
import warnings

import numpy as np
import torch
from torch import nn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
warnings.filterwarnings("ignore")

from salience_detr_amd import synthetic as syn  # noqa: E402

POLICIES = {"backbone_and_linear_projection": "finetune_backbone_and_linear_projection",
            "backbone": "finetune_backbone_param",
            "backbone_no_norm_weight_decay": "finetune_backbone_with_no_norm_weight_decay"}
LR, WEIGHT_DECAY, MAX_NORM = 1e-4, 1e-4, 0.1
STEPS = 6
SAMPLE_ABOVE = 1024
# shape, group, gradient scale: 1 element, odd sizes, a 1-D tensor longer than a chunk, 2048 x 256
TENSORS = [((1,), 0, 1.0), ((7,), 5, 10.0), ((333,), 2, 1e-4), ((5000,), 4, 1e-2), ((2048, 256), 0, 1e-3),
           ((91, 256), 3, 1e-1), ((17, 3, 3), 1, 1.0), ((256,), 5, 1e-3), ((3, 5), 2, 1e-2), ((1027,), 1, 1e-4),
           ((4,), 3, 10.0), ((255,), 4, 1e-1)]
# six groups with distinct lr and weight_decay
GROUPS = [(1e-4, 1e-4), (1e-5, 2e-4), (2e-5, 0.0), (3e-5, 5e-5), (4e-5, 1e-3), (2e-4, 1e-2)]
STEP_SCALE = [1.0, 1.0, 1.0, 1e-4, 1.0, 1.0]       # step 3: a total norm below max_norm, the clip is inactive
NONE_GRAD = (2, 6)                                  # (step, tensor): no gradient
ZERO_GRAD = (1, 8)                                  # (step, tensor): an all-zero gradient


class StubBottleneck(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(4, 4, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(4)
        self.conv2 = nn.Conv2d(4, 4, 3, bias=True)
        self.bn2 = nn.GroupNorm(2, 4)
        self.downsample = nn.Sequential(nn.Conv2d(4, 4, 1, bias=False), nn.BatchNorm2d(4))


class StubBackbone(nn.Module):
    """Registers parameters under ResNet key names (conv1, bn1, layer1.0.conv1, layer1.0.downsample.1, ..)."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 4, 7, bias=False)
        self.bn1 = nn.BatchNorm2d(4)
        self.layer1 = nn.Sequential(StubBottleneck())
        self.layer2 = nn.Sequential(StubBottleneck())


def groups_fixture():
    import _ref_import
    _ref_import.install()
    import make_detector_train_golden as DTG
    from optimizer import param_dict
    maps = [torch.zeros(2, ch, 64 // s, 96 // s) for ch, s in zip(DTG.BACKBONE_CHANNELS, (8, 16, 32))]
    det, _ = DTG.build(maps, 12)
    det.backbone = StubBackbone()
    names = {id(p): n for n, p in det.named_parameters()}
    data = {"model_names": np.array([n for n, _ in det.named_parameters()])}
    for policy, fn in POLICIES.items():
        groups = getattr(param_dict, fn)(det, LR)
        ordered, index, lr, wd = [], [], [], []
        for gi, g in enumerate(groups):
            for p in g["params"]:
                ordered.append(names[id(p)])
                index.append(gi)
                lr.append(g.get("lr", LR))
                wd.append(g.get("weight_decay", WEIGHT_DECAY))
        assert len(set(ordered)) == len(ordered) == len(names), (policy, len(ordered), len(names))
        data[f"groups.{policy}.names"] = np.array(ordered)
        data[f"groups.{policy}.index"] = np.array(index, dtype=np.int32)
        data[f"groups.{policy}.lr"] = np.array(lr, dtype=np.float64)
        data[f"groups.{policy}.weight_decay"] = np.array(wd, dtype=np.float64)
        print(policy, "groups", [len(g["params"]) for g in groups])
    return data


def stride_of(numel):
    if numel <= SAMPLE_ABOVE:
        return 1
    s = -(-numel // SAMPLE_ABOVE)
    return s + 1 - s % 2        # odd: walks every column of a power-of-two row length


def gradient(k, i, dtype):
    shape, _, scale = TENSORS[i]
    if (k, i) == NONE_GRAD:
        return None
    if (k, i) == ZERO_GRAD:
        return torch.zeros(shape, dtype=dtype)
    return (syn.det_randn(f"opt.g.{k}.{i}", shape) * (scale * STEP_SCALE[k])).to(dtype)


def run(dtype):
    params = [nn.Parameter((syn.det_randn(f"opt.p.{i}", shape) * 3).to(dtype)) for i, (shape, _, _) in enumerate(TENSORS)]
    groups = [{"params": [p for p, t in zip(params, TENSORS) if t[1] == gi], "lr": lr, "weight_decay": wd}
              for gi, (lr, wd) in enumerate(GROUPS)]
    opt = torch.optim.AdamW(groups, lr=LR, weight_decay=WEIGHT_DECAY)
    warm = torch.optim.lr_scheduler.LinearLR(opt, start_factor=1.0 / 1000, total_iters=2)
    decay = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[1], gamma=0.1)
    out, norms, lrs = [], [], []
    for k in range(STEPS):
        for i, p in enumerate(params):
            p.grad = gradient(k, i, dtype)
        lrs.append([g["lr"] for g in opt.param_groups])
        norm = torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
        opt.step()
        if k < 3:                       # the first epoch's three iterations
            warm.step()
        if k % 3 == 2:                  # end of an epoch
            decay.step()
        norms.append(float(norm.double()))
        step = []
        for p in params:
            s = opt.state.get(p, {})
            m = s.get("exp_avg", torch.zeros_like(p)).detach()
            v = s.get("exp_avg_sq", torch.zeros_like(p)).detach()
            step.append((p.detach().double().clone(), m.double().clone(), v.double().clone()))
        out.append(step)
    return out, np.array(norms), np.array(lrs)


def trajectory_fixture():
    t64, n64, lrs = run(torch.float64)
    t32, n32, lrs32 = run(torch.float32)
    assert np.array_equal(lrs, lrs32)
    assert n64[3] < MAX_NORM and all(n64[k] > MAX_NORM for k in range(STEPS) if k != 3), n64
    assert lrs[0, 0] < lrs[2, 0] and lrs[3, 0] < 0.2 * lrs[2, 0], lrs[:, 0]      # warm-up, then the decay inside the run
    strides = [stride_of(int(np.prod(s))) for s, _, _ in TENSORS]
    data = {"shapes": np.array([";".join(str(v) for v in s) for s, _, _ in TENSORS]),
            "group_of": np.array([g for _, g, _ in TENSORS], dtype=np.int32),
            "grad_scale": np.array([s for _, _, s in TENSORS]), "step_scale": np.array(STEP_SCALE),
            "group_lr": np.array([g[0] for g in GROUPS]), "group_weight_decay": np.array([g[1] for g in GROUPS]),
            "lrs": lrs, "max_norm": np.array(MAX_NORM), "none_grad": np.array(NONE_GRAD), "zero_grad": np.array(ZERO_GRAD),
            "strides": np.array(strides, dtype=np.int32), "norms": n64,
            "d_ref_norm": np.abs(n32 - n64) / n64, "default_lr": np.array(LR), "default_weight_decay": np.array(WEIGHT_DECAY)}
    d_ref = np.zeros((STEPS, len(TENSORS), 3))
    for k in range(STEPS):
        for i, s in enumerate(strides):
            for j, kind in enumerate(("param", "exp_avg", "exp_avg_sq")):
                a, b = t64[k][i][j].reshape(-1)[::s], t32[k][i][j].reshape(-1)[::s]
                data[f"{kind}.{k}.{i}"] = a.numpy()
                d_ref[k, i, j] = (a - b).abs().max().item()
    data["d_ref"] = d_ref
    print("norms", n64, "\nd_ref_norm", data["d_ref_norm"])
    print("d_ref param", d_ref[..., 0].max(0), "\nd_ref exp_avg", d_ref[..., 1].max(0), "\nd_ref exp_avg_sq", d_ref[..., 2].max(0))
    return data


def main():
    data = trajectory_fixture()
    data.update(groups_fixture())
    out = os.path.join(HERE, "optimizer_cases.npz")
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes")
    assert os.path.getsize(out) < 1_000_000


if __name__ == "__main__":
    main()
