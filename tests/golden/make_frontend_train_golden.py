"""tests/golden/frontend_train.npz: the training gradients of the reference ``ChannelMapper``
(models/necks/channel_mapper.py), run on the CPU by the IMPORTED reference (loaded as tests/golden/make_frontend_golden.py
loads it) on the cases of tests/frontend_train_cases.py.

Stored per case ``<case>.*``: ``names`` (every parameter, then ``input.<l>``: every input requires grad); per name
``g:<name>`` (the float64 gradient: of the 1024-element sample -- whole up to 1024 elements, else the strided sub-sample
``backbone_cases.sub_index`` cut to 1024 -- the first ``frontend_train_cases.STORE``), ``norm:<name>`` and ``max:<name>``
(L2 norm and max abs of the whole float64 gradient), ``d32:<name>`` / ``dbf16:<name>``: the own-scale distance (max|g - ref|
on the 1024-element sample / max|ref|) of the reference's fp32 run and of its ``torch.autocast("cpu", bfloat16)`` run from
the float64 gradient.

Run from the repository root: ``python tests/golden/make_frontend_train_golden.py`` (needs the reference checkout).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
import frontend_train_cases as TC  # noqa: E402


def main():
    _ref_import.install()
    from models.necks.channel_mapper import ChannelMapper

    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    data = {}
    for case in TC.CASES:
        net = TC.build(ChannelMapper, case)
        names = TC.names(net, case)
        ref = TC.torch_grads(net.double(), case)
        g32 = TC.torch_grads(net.float(), case, dtype=torch.float32)
        gbf = TC.torch_grads(net, case, dtype=torch.float32, autocast=torch.bfloat16)
        data[f"{case}.names"] = np.array(names)
        for n in names:
            idx, wide = TC.stored_index(ref[n].numel()), TC.sample_index(ref[n].numel())
            pick, sample = (lambda t: t.reshape(-1)[idx]), (lambda t: t.reshape(-1)[wide])
            scale = ref[n].abs().max().item()
            data[f"{case}.g:{n}"] = pick(ref[n]).numpy()
            data[f"{case}.norm:{n}"] = np.float64(ref[n].norm().item())
            data[f"{case}.max:{n}"] = np.float64(scale)
            data[f"{case}.d32:{n}"] = np.float64(TC.own_scale(sample(g32[n]), sample(ref[n]), scale))
            data[f"{case}.dbf16:{n}"] = np.float64(TC.own_scale(sample(gbf[n]), sample(ref[n]), scale))
        d32 = [data[f"{case}.d32:{n}"] for n in names]
        dbf = [data[f"{case}.dbf16:{n}"] for n in names]
        print(case, len(names), "tensors; d32 %.2e .. %.2e, dbf16 %.2e .. %.2e" % (min(d32), max(d32), min(dbf), max(dbf)),
              flush=True)
    np.savez_compressed(TC.GOLDEN, **data)
    print(TC.GOLDEN, os.path.getsize(TC.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
