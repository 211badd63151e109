"""tests/golden/convnext_cases.npz: the reference ConvNeXt backbone run on the CPU by the IMPORTED reference ``ConvNeXt``
(models/backbones/convnext.py) on the inputs of tests/convnext_cases.py.

The reference module imports torchvision's feature extractor and ``StochasticDepth`` at module level; this script
installs stubs for them as make_backbone_golden.py does (``StochasticDepth`` is the identity in eval, which is all this
script runs), points the ``models`` packages at the reference checkout without running ``models/backbones/__init__.py``
and loads ``convnext.py`` alone.  It builds ``ConvNeXt(block_setting=...)`` directly and runs ``features`` stage by stage.

Stored per case ``<case>.*``: the state-dict keys the reference's feature extractor keeps (``keys``: ``features.0`` ..
``features.{2 * max(return_indices) + 1}``); per returned stage ``features.N``: the float64 run stored as fp32
(``ref_features.N``, whole when small, else the strided sub-sample of tests/backbone_cases.sub_index), the max abs
distance of the reference's fp32 run from it (``d32_``) and of its ``torch.autocast("cpu", bfloat16 / float16)`` runs
(``dbf16_`` / ``df16_``), all measured on the stored elements; the RMS of the float64 output (``rms_``).

Run from the repository root: ``python tests/golden/make_convnext_golden.py`` (needs the reference checkout).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))   # tests/ (convnext_cases)
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
import convnext_cases as CC  # noqa: E402
from make_backbone_golden import _stub  # noqa: E402

OUT = os.path.join(HERE, "convnext_cases.npz")


class _EvalStochasticDepth(torch.nn.Module):
    def __init__(self, p, mode):
        super().__init__()
        self.p, self.mode = p, mode

    def forward(self, x):
        assert not self.training
        return x


def load_reference_convnext():
    _ref_import.install()
    root = _ref_import.REFERENCE_ROOT
    if "omegaconf" not in sys.modules:
        try:
            import omegaconf  # noqa: F401
        except ImportError:
            _stub("omegaconf", DictConfig=dict, ListConfig=list, OmegaConf=object)
    try:
        import accelerate  # noqa: F401
        import accelerate.logging  # noqa: F401
    except ImportError:
        _stub("accelerate")
        _stub("accelerate.logging", get_logger=lambda *a, **k: None)
    _stub("torchvision.models.feature_extraction", create_feature_extractor=None)
    _stub("torchvision.ops.stochastic_depth", StochasticDepth=_EvalStochasticDepth)
    sys.modules["torchvision.ops"].DeformConv2d = object
    for pkg, sub in (("models", "models"), ("models.backbones", os.path.join("models", "backbones"))):
        _stub(pkg).__path__ = [os.path.join(root, sub)]
    spec = importlib.util.spec_from_file_location("models.backbones.convnext", os.path.join(root, "models", "backbones",
                                                                                            "convnext.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def run(net, x, num_stages):
    outs = []
    for idx in range(2 * num_stages):
        x = net.features[idx](x)
        if idx % 2 == 1:
            outs.append(x)
    return outs


def main():
    mod = load_reference_convnext()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    data = {}
    for name in sys.argv[1:] or list(CC.CASES):
        ret = CC.CASES[name][2]
        net = mod.ConvNeXt(block_setting=[mod.CNBlockConfig(*row) for row in CC.setting(name)]).eval()
        stages = max(ret) + 1
        keys = [k for k in net.state_dict() if k.startswith("features.") and int(k.split(".")[1]) <= 2 * stages - 1]
        net.load_state_dict(CC.state({k: net.state_dict()[k] for k in keys}, name), strict=False)
        data[f"{name}.keys"] = np.array(keys)
        canvas, _ = CC.canvas_and_mask(CC.images(name))
        with torch.no_grad():
            ref64 = run(net.double(), canvas.double(), stages)
            net.float()
            ref32 = run(net, canvas, stages)
            ac = {}
            for tag, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
                with torch.autocast("cpu", dtype=dt):
                    ac[tag] = run(net, canvas, stages)
        for i in ret:
            key = f"features.{2 * i + 1}"
            r64, r32 = ref64[i], ref32[i].double()
            pick = (lambda t: t.reshape(-1)) if r64.numel() <= CC.WHOLE_MAX else CC.sub_sample
            data[f"{name}.ref_{key}"] = pick(r64).float().numpy()   # (fp32 storage: 1e-7 relative, far below d32)
            data[f"{name}.d32_{key}"] = np.float64((pick(r32) - pick(r64)).abs().max().item())
            for tag in ac:
                data[f"{name}.d{tag}_{key}"] = np.float64((pick(ac[tag][i].double()) - pick(r64)).abs().max().item())
            data[f"{name}.rms_{key}"] = np.float64(r64.pow(2).mean().sqrt().item())
            print(name, key, tuple(r64.shape), "rms %.3g max %.3g d32 %.3g dbf16 %.3g df16 %.3g" % (
                data[f"{name}.rms_{key}"], r64.abs().max().item(), data[f"{name}.d32_{key}"],
                data[f"{name}.dbf16_{key}"], data[f"{name}.df16_{key}"]), flush=True)
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
