"""tests/golden/backbone_train.npz: the training gradients of the reference backbone, run on the CPU by the IMPORTED
reference ``ResNet`` (loaded as tests/golden/make_backbone_golden.py loads it) on the cases of
tests/backbone_train_cases.py (``r18`` / ``r50`` of backbone_cases, ``freeze_indices=(0,)``, cotangents
``det_rand("backbone_train.<case>.<layer>") - 0.5``).

Stored per case ``<case>.*``: ``masks`` (the sign masks of every ReLU output of the float64 run, bit-packed, in forward
order) with their ``mask_shapes``; ``names`` (the trainable conv weights); per weight ``g:<name>`` (the float64 gradient,
whole up to 1024 elements, else the strided sub-sample ``backbone_cases.sub_index`` cut to 1024), ``norm:<name>`` and
``max:<name>`` (L2 norm and max abs of the whole float64 gradient), ``d32:<name>`` / ``dbf16:<name>``: the own-scale
distance (max|g - ref| on the stored elements / max|ref|) of the reference's fp32 run, and of its
``torch.autocast("cpu", bfloat16)`` run, from the float64 gradient with EVERY run under the float64 run's masks (each
ReLU of the reference's module tree replaced by ``x * mask``).

Run from the repository root: ``python tests/golden/make_backbone_train_golden.py`` (needs the reference checkout).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import backbone_cases as BC  # noqa: E402
import backbone_train_cases as TC  # noqa: E402
from make_backbone_golden import load_reference_resnet  # noqa: E402


def main():
    mod, FrozenBatchNorm2d = load_reference_resnet()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    archs = {"resnet50": (mod.Bottleneck, (3, 4, 6, 3)), "resnet18": (mod.BasicBlock, (2, 2, 2, 2))}
    data = {}
    for case in TC.CASES:
        arch, ret, _ = BC.CASES[case]
        block, layers = archs[arch]
        net = mod.ResNet(block=block, layers=layers, norm_layer=FrozenBatchNorm2d).eval()
        stages = max(ret) + 1
        keys = [k for k in net.state_dict() if not k.startswith(("fc.", "avgpool.")) and
                not any(k.startswith(f"layer{i + 1}.") for i in range(stages, 4))]
        net.load_state_dict(BC.state({k: net.state_dict()[k] for k in keys}, case), strict=False)
        names = TC.trainable_names(net, stages)
        canvas, _ = BC.canvas_and_mask(BC.images(case))
        masks = []
        net.double()
        ref = TC.masked_grads(net, canvas, stages, ret, names, case, record=masks)
        again = TC.masked_grads(net, canvas, stages, ret, names, case, masks=masks)
        assert all(torch.equal(ref[n], again[n]) for n in names)   # x * mask is relu under the run's own masks
        net.float()
        flips = []
        g32_free = TC.masked_grads(net, canvas, stages, ret, names, case, record=flips, dtype=torch.float32)
        del g32_free
        print(case, "relu outputs", sum(m.numel() for m in masks), "fp32 sign flips",
              sum(int((a != b).sum()) for a, b in zip(masks, flips)), flush=True)
        g32 = TC.masked_grads(net, canvas, stages, ret, names, case, masks=masks, dtype=torch.float32)
        gbf = TC.masked_grads(net, canvas, stages, ret, names, case, masks=masks, dtype=torch.float32,
                              autocast=torch.bfloat16)
        data[f"{case}.masks"] = TC.pack_masks(masks)
        data[f"{case}.mask_shapes"] = np.array([list(m.shape) for m in masks], dtype=np.int64)
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
        print(case, len(names), "weights; d32 %.2e .. %.2e, dbf16 %.2e .. %.2e" % (min(d32), max(d32), min(dbf), max(dbf)),
              flush=True)
    out = TC.GOLDEN
    np.savez_compressed(out, **data)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
