"""tests/golden/focalnet_cases.npz: the reference FocalNet backbone run on the CPU by the IMPORTED reference ``FocalNet``
and ``PostProcess`` (models/backbones/focalnet.py) on the inputs of tests/focalnet_cases.py.

The reference module imports torchvision's feature extractor and ``StochasticDepth`` at module level; this script
installs stubs for them as make_convnext_golden.py does (``StochasticDepth`` is the identity in eval, which is all this
script runs), points the ``models`` packages at the reference checkout without running ``models/backbones/__init__.py``
and loads ``focalnet.py`` alone.  It builds ``FocalNet(...)`` directly (no checkpoint loading) and walks its stages: the
blocks of stage i, ``PostProcess.norm{i}`` + the NCHW permutation for a returned stage, then the stage's down-sampler.

Stored per case ``<case>.*``: ``keys``, the state-dict keys of the reference's ``nn.Sequential(feature_extractor,
PostProcess)``.  torchvision is absent, so they cannot come from ``create_feature_extractor``: they are the reference
``FocalNet``'s keys restricted to what the extractor keeps for ``return_indices`` (stages up to the last returned one,
that one without its down-sampler) prefixed ``0.``, plus ``PostProcess``'s prefixed ``1.``.  Per returned stage
``layers.N.blocks``: the float64 run stored as fp32 (``ref_``, whole when small, else the strided sub-sample of
tests/backbone_cases.sub_index), the max abs distance of the reference's fp32 run from it (``d32_``) and of its
``torch.autocast("cpu", bfloat16 / float16)`` runs (``dbf16_`` / ``df16_``), all measured on the stored elements; the RMS
of the float64 output (``rms_``).

Run from the repository root: ``python tests/golden/make_focalnet_golden.py`` (needs the reference checkout).
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))   # tests/ (focalnet_cases)
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
import focalnet_cases as FC  # noqa: E402
from make_backbone_golden import _stub  # noqa: E402
from make_convnext_golden import _EvalStochasticDepth  # noqa: E402

OUT = os.path.join(HERE, "focalnet_cases.npz")


def load_reference_focalnet():
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
    sys.modules["torchvision.ops"].StochasticDepth = _EvalStochasticDepth
    sys.modules["torchvision.ops"].DeformConv2d = object
    for pkg, sub in (("models", "models"), ("models.backbones", os.path.join("models", "backbones"))):
        _stub(pkg).__path__ = [os.path.join(root, sub)]
    spec = importlib.util.spec_from_file_location("models.backbones.focalnet", os.path.join(root, "models", "backbones",
                                                                                            "focalnet.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod


def kept(key, last):
    """Does the feature extractor for a last returned stage ``last`` keep this ``FocalNet`` key?"""
    parts = key.split(".")
    if parts[0] != "layers":
        return True
    i = int(parts[1])
    return i < last or (i == last and parts[2] == "blocks")


def run(net, post, x, ret):
    outs = {}
    x = net.pos_drop(net.patch_embed(x.permute(0, 2, 3, 1)))
    for i in range(max(ret) + 1):
        x = net.layers[i].blocks(x)
        if i in ret:
            outs[i] = getattr(post, f"norm{i}")(x).permute(0, 3, 1, 2).contiguous()
        if i < max(ret):
            x = net.layers[i].downsample(x)
    return outs


def main():
    mod = load_reference_focalnet()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    data = {}
    for name in sys.argv[1:] or list(FC.CASES):
        ret = FC.CASES[name][1]
        cfg = FC.config(name)
        net = mod.FocalNet(**cfg).eval()
        post = mod.PostProcess([cfg["embed_dim"] * 2 ** i for i in ret], ret).eval()
        own = {"0." + k: v for k, v in net.state_dict().items() if kept(k, max(ret))}
        own.update({"1." + k: v for k, v in post.state_dict().items()})
        sd = FC.state(own, name)
        net.load_state_dict({k[2:]: v for k, v in sd.items() if k.startswith("0.")}, strict=False)
        post.load_state_dict({k[2:]: v for k, v in sd.items() if k.startswith("1.")})
        data[f"{name}.keys"] = np.array(list(own))
        x = FC.canvas(name)
        with torch.no_grad():
            ref64 = run(net.double(), post.double(), x.double(), ret)
            net.float(), post.float()
            ref32 = run(net, post, x, ret)
            ac = {}
            for tag, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
                with torch.autocast("cpu", dtype=dt):
                    ac[tag] = run(net, post, x, ret)
        for i in ret:
            key = f"layers.{i}.blocks"
            r64, r32 = ref64[i], ref32[i].double()
            pick = (lambda t: t.reshape(-1)) if r64.numel() <= FC.WHOLE_MAX else FC.sub_sample
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
