"""tests/golden/neck_train.npz: one training step of the reference ``RepVGGPluXNetwork`` (models/necks/repnet.py) in
``train()`` mode, run in float64 on the CPU by the IMPORTED reference (loaded as the other makers load it) on the cases of
tests/neck_train_cases.py.

Stored per case ``<case>.*``: ``names`` (every parameter, then ``input.<l>``), ``stats`` (the running statistics' names);
per output level ``out:<l>`` / ``outmax:<l>`` / ``outd32:<l>``; per statistic ``s:<name>`` (after one forward) and
``sd32:<name>``; per gradient ``g:<name>`` (float64: of the 1024-element sample -- whole up to 1024 elements, else the
strided sub-sample ``backbone_cases.sub_index`` cut to 1024 -- the first ``neck_train_cases.STORE``), ``norm:<name>`` and
``max:<name>`` (L2 norm and max abs of the whole float64 gradient) and ``d32:<name>``: the own-scale distance (max|g - ref|
on the sample / max|ref|) of the reference's own float32 run from its float64 run.  Outputs and statistics are sub-sampled
and measured the same way.

Run from the repository root: ``python tests/golden/make_neck_train_golden.py`` (needs the reference checkout).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
import neck_train_cases as TC  # noqa: E402


def main():
    _ref_import.install()
    from models.necks.repnet import RepVGGPluXNetwork

    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    data = {}
    for case in TC.CASES:
        net = TC.build(RepVGGPluXNetwork, case).double()
        outs, ref, stats = TC.run(TC.reference_forward(net), net, case)
        net32 = TC.build(RepVGGPluXNetwork, case).float()
        outs32, g32, stats32 = TC.run(TC.reference_forward(net32), net32, case, dtype=torch.float32)
        names = TC.names(net, case)
        data[f"{case}.names"] = np.array(names)
        data[f"{case}.stats"] = np.array(TC.stat_names(net))

        def put(prefix, dkey, key, t, t32, extra=False):
            idx, wide = TC.stored_index(t.numel()), TC.sample_index(t.numel())
            scale = t.abs().max().item()
            data[f"{case}.{prefix}:{key}"] = t.reshape(-1)[idx].numpy()
            data[f"{case}.{prefix}max:{key}" if prefix != "g" else f"{case}.max:{key}"] = np.float64(scale)
            data[f"{case}.{dkey}:{key}"] = np.float64(TC.own_scale(t32.reshape(-1)[wide], t.reshape(-1)[wide], scale))
            if extra:
                data[f"{case}.norm:{key}"] = np.float64(t.norm().item())

        for l, (o, o32) in enumerate(zip(outs, outs32)):
            put("out", "outd32", str(l), o, o32)
        for n in TC.stat_names(net):
            put("s", "sd32", n, stats[n], stats32[n])
        for n in names:
            put("g", "d32", n, ref[n], g32[n], extra=True)
        d32 = [data[f"{case}.d32:{n}"] for n in names]
        print(case, len(names), "gradients; d32 %.2e .. %.2e" % (min(d32), max(d32)), flush=True)
    np.savez_compressed(TC.GOLDEN, **data)
    print(TC.GOLDEN, os.path.getsize(TC.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
