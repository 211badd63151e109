"""tests/golden/swin_cases.npz: the reference Swin backbone run on the CPU by the IMPORTED reference ``SwinTransformer``
(models/backbones/swin.py) on the inputs of tests/swin_cases.py.

The reference module imports torchvision's feature extractor, ``MLP``, ``Permute`` and ``StochasticDepth`` at module
level; torchvision is absent, so this script installs stubs as make_focalnet_golden.py does: ``StochasticDepth`` is the
identity in eval (all this script runs), ``Permute`` permutes, ``MLP`` is Linear, GELU, Dropout, Linear, Dropout (so its
keys are ``mlp.0`` / ``mlp.3``, as torchvision's).  It points the ``models`` packages at the reference checkout without
running ``models/backbones/__init__.py``, loads ``swin.py`` alone, builds ``SwinTransformer(...)`` directly (no
checkpoint loading) and walks ``features``: the stem, then per stage its blocks, the NCHW permutation for a returned
stage, and the stage's merging layer.

Stored per case ``<case>.*``: ``keys``, the state-dict keys of the reference's ``nn.Sequential(feature_extractor,
PostProcess)``: the ``SwinTransformer``'s keys restricted to what the extractor keeps for ``return_indices``
(``features`` up to the last returned stage, no ``norm`` / ``head``) prefixed ``0.``; ``PostProcess`` has none.  Per
returned stage ``features.N``: the float64 run stored as fp32 (``ref_``, whole when small, else the strided sub-sample
of tests/backbone_cases.sub_index), the max abs distance of the reference's fp32 run from it (``d32_``) and of its
``torch.autocast("cpu", bfloat16 / float16)`` runs (``dbf16_`` / ``df16_``), all measured on the stored elements; the RMS
of the float64 output (``rms_``).

Run from the repository root: ``python tests/golden/make_swin_golden.py`` (needs the reference checkout).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))   # tests/ (swin_cases)
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
import swin_cases as SC  # noqa: E402
from make_backbone_golden import _stub  # noqa: E402
from make_convnext_golden import _EvalStochasticDepth  # noqa: E402

OUT = os.path.join(HERE, "swin_cases.npz")


class _Permute(torch.nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.dims = list(dims)

    def forward(self, x):
        return x.permute(*self.dims)


class _MLP(torch.nn.Sequential):
    def __init__(self, in_channels, hidden_channels, activation_layer=torch.nn.ReLU, inplace=None, dropout=0.0):
        layers, dim = [], in_channels
        for hidden in hidden_channels[:-1]:
            layers += [torch.nn.Linear(dim, hidden), activation_layer(), torch.nn.Dropout(dropout)]
            dim = hidden
        layers += [torch.nn.Linear(dim, hidden_channels[-1]), torch.nn.Dropout(dropout)]
        super().__init__(*layers)


def load_reference_swin():
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
    ops = sys.modules["torchvision.ops"]
    ops.StochasticDepth, ops.Permute, ops.MLP, ops.DeformConv2d = _EvalStochasticDepth, _Permute, _MLP, object
    for pkg, sub in (("models", "models"), ("models.backbones", os.path.join("models", "backbones"))):
        _stub(pkg).__path__ = [os.path.join(root, sub)]
    spec = importlib.util.spec_from_file_location("models.backbones.swin", os.path.join(root, "models", "backbones", "swin.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def kept(key, last):
    """Does the feature extractor for a last returned stage ``last`` keep this ``SwinTransformer`` key?"""
    parts = key.split(".")
    return parts[0] == "features" and int(parts[1]) <= 2 * last + 1


def run(net, x, ret):
    outs = {}
    x = net.features[0](x)
    for i in range(max(ret) + 1):
        x = net.features[2 * i + 1](x)
        if i in ret:
            outs[i] = x.permute(0, 3, 1, 2).contiguous()
        if i < max(ret):
            x = net.features[2 * i + 2](x)
    return outs


def main():
    mod = load_reference_swin()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    data = {}
    for name in sys.argv[1:] or list(SC.CASES):
        ret = SC.CASES[name][1]
        net = mod.SwinTransformer(**SC.config(name)).eval()
        own = {"0." + k: v for k, v in net.state_dict().items() if kept(k, max(ret))}
        sd = SC.state(own, name)
        net.load_state_dict({k[2:]: v for k, v in sd.items()}, strict=False)
        data[f"{name}.keys"] = np.array(list(own))
        x = SC.canvas(name)
        with torch.no_grad():
            ref64 = run(net.double(), x.double(), ret)
            net.float()
            ref32 = run(net, x, ret)
            ac = {}
            for tag, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
                with torch.autocast("cpu", dtype=dt):
                    ac[tag] = run(net, x, ret)
        for i in ret:
            key = f"features.{2 * i + 1}"
            r64, r32 = ref64[i], ref32[i].double()
            pick = (lambda t: t.reshape(-1)) if r64.numel() <= SC.WHOLE_MAX else SC.sub_sample
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
