"""tests/golden/frontend_cases.npz: the input stage of the reference detector (row N7), run on the CPU by the
IMPORTED reference ``ChannelMapper`` (models/necks/channel_mapper.py) and ``PositionEmbeddingSine``
(models/bricks/position_encoding.py), on the inputs of tests/frontend_cases.py.

Stored per mapper case ``m.<case>.*``: the reference's state-dict keys and shapes; per level the output's strided
sub-sample (``sub<l>``) and float64 per-(image, channel) sums (``sum<l>``), the whole output for the reduced case
(``out<l>``); for the reduced and ResNet50 cases the reference's own distance under ``torch.autocast("cpu", bfloat16 /
float16)`` from its fp32 run (``ac_bf16<l>`` / ``ac_f16<l>``, max abs).  Per position case ``p.<case>.*``: the level masks
(exact) and the positions (whole, or sub-sample + sums at full size).

Run from the repository root: ``python tests/golden/make_frontend_golden.py`` (needs the reference checkout).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))   # tests/ (frontend_cases)
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
import frontend_cases as FC  # noqa: E402

OUT = os.path.join(HERE, "frontend_cases.npz")
FULL_OUTPUT = ("reduced",)
AUTOCAST = ("reduced", "r50")


def main():
    _ref_import.install()
    from models.necks.channel_mapper import ChannelMapper
    from models.bricks.position_encoding import PositionEmbeddingSine

    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    data = {}
    for name, (cin, cout, num_outs, _, _) in FC.MAPPER_CASES.items():
        ref = ChannelMapper(list(cin), cout, num_outs).eval()
        sd = FC.mapper_state(ref.state_dict(), name)
        ref.load_state_dict(sd)
        feats, _ = FC.mapper_inputs(name)
        keys = list(sd.keys())
        data[f"m.{name}.keys"] = np.array(keys)
        data[f"m.{name}.shapes"] = np.array([",".join(map(str, sd[k].shape)) for k in keys])
        with torch.no_grad():
            outs = ref({str(i): f for i, f in enumerate(feats)})
            for l, o in enumerate(outs):
                data[f"m.{name}.sub{l}"] = FC.sub_sample(o).numpy()
                data[f"m.{name}.sum{l}"] = FC.channel_sums(o).numpy()
                if name in FULL_OUTPUT:
                    data[f"m.{name}.out{l}"] = o.numpy()
            if name in AUTOCAST:
                for tag, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
                    with torch.autocast("cpu", dtype=dt):
                        ac = ref({str(i): f for i, f in enumerate(feats)})
                    for l, (a, o) in enumerate(zip(ac, outs)):
                        data[f"m.{name}.ac_{tag}{l}"] = np.float64((a.float() - o).abs().max().item())
        print(name, [tuple(o.shape) for o in outs], flush=True)

    for name in FC.POSITION_CASES:
        kw, mask, shapes = FC.position_inputs(name)
        pe = PositionEmbeddingSine(**kw)
        for l, s in enumerate(shapes):
            m = FC.reference_level_mask(mask, s)
            pos = pe(m)
            data[f"p.{name}.mask{l}"] = np.packbits(m.numpy().reshape(-1))
            if pos.numel() <= 300_000:
                data[f"p.{name}.pos{l}"] = pos.numpy()
            else:
                data[f"p.{name}.sub{l}"] = FC.sub_sample(pos).numpy()
                data[f"p.{name}.sum{l}"] = FC.channel_sums(pos).numpy()
        print(name, shapes, flush=True)
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
