"""tests/golden/backbone_cases.npz: the reference backbone (row N0) run on the CPU by the IMPORTED reference ``ResNet``
(models/backbones/resnet.py, ``norm_layer=FrozenBatchNorm2d``) on the inputs of tests/backbone_cases.py.

The reference module imports torchvision's feature extractor and deformable conv at module level; neither is needed
to build and run ``ResNet`` itself, so this script installs stubs for them (and for ``omegaconf`` / ``accelerate`` when
they are missing), points the ``models`` packages at the reference checkout without running
``models/backbones/__init__.py`` and loads ``resnet.py`` alone.

Stored per case ``<case>.*``: the state-dict keys the reference's feature extractor keeps (``keys``: ``conv1``, ``bn1``,
``layer1`` .. ``layer{max(return_indices) + 1}``); per returned stage ``layerN``: the float64 run stored as fp32 (``ref_layerN``,
whole when small, else the strided sub-sample of tests/backbone_cases.sub_index), the max abs distance of the reference's
fp32 run from it (``d32_layerN``) and of its ``torch.autocast("cpu", bfloat16 / float16)`` runs (``dbf16_layerN`` /
``df16_layerN``), all measured on the stored elements; the RMS of the float64 output (``rms_layerN``).

Run from the repository root: ``python tests/golden/make_backbone_golden.py`` (needs the reference checkout).
"""
import importlib.machinery
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))   # tests/ (backbone_cases)
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
import backbone_cases as BC  # noqa: E402

OUT = os.path.join(HERE, "backbone_cases.npz")


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def load_reference_resnet():
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
    sys.modules["torchvision.ops"].DeformConv2d = object
    for pkg, sub in (("models", "models"), ("models.backbones", os.path.join("models", "backbones"))):
        _stub(pkg).__path__ = [os.path.join(root, sub)]
    spec = importlib.util.spec_from_file_location("models.backbones.resnet", os.path.join(root, "models", "backbones",
                                                                                          "resnet.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    from models.bricks.misc import FrozenBatchNorm2d
    return mod, FrozenBatchNorm2d


def run(net, x, num_stages):
    y = net.maxpool(net.relu(net.bn1(net.conv1(x))))
    outs = []
    for i in range(num_stages):
        y = getattr(net, f"layer{i + 1}")(y)
        outs.append(y)
    return outs


def main():
    mod, FrozenBatchNorm2d = load_reference_resnet()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    archs = {"resnet50": (mod.Bottleneck, (3, 4, 6, 3)), "resnet18": (mod.BasicBlock, (2, 2, 2, 2))}
    data = {}
    only = sys.argv[1:] or list(BC.CASES)
    for name in only:
        arch, ret, _ = BC.CASES[name]
        block, layers = archs[arch]
        net = mod.ResNet(block=block, layers=layers, norm_layer=FrozenBatchNorm2d).eval()
        stages = max(ret) + 1
        keys = [k for k in net.state_dict() if not k.startswith(("fc.", "avgpool.")) and
                not any(k.startswith(f"layer{i + 1}.") for i in range(stages, 4))]
        sd = BC.state({k: net.state_dict()[k] for k in keys}, name)
        net.load_state_dict(sd, strict=False)
        data[f"{name}.keys"] = np.array(keys)
        canvas, _ = BC.canvas_and_mask(BC.images(name))
        with torch.no_grad():
            ref64 = run(net.double(), canvas.double(), stages)
            net.float()
            ref32 = run(net, canvas, stages)
            ac = {}
            for tag, dt in (("bf16", torch.bfloat16), ("f16", torch.float16)):
                with torch.autocast("cpu", dtype=dt):
                    ac[tag] = run(net, canvas, stages)
        for i in ret:
            key = f"layer{i + 1}"
            r64, r32 = ref64[i], ref32[i].double()
            whole = r64.numel() <= BC.WHOLE_MAX
            pick = (lambda t: t.reshape(-1)) if whole else BC.sub_sample
            data[f"{name}.ref_{key}"] = pick(r64).float().numpy()   # (fp32 storage: 1e-7 relative, far below d32)
            data[f"{name}.d32_{key}"] = np.float64((pick(r32) - pick(r64)).abs().max().item())
            for tag in ac:
                data[f"{name}.d{tag}_{key}"] = np.float64((pick(ac[tag][i].double()) - pick(r64)).abs().max().item())
            data[f"{name}.rms_{key}"] = np.float64(r64.pow(2).mean().sqrt().item())
            print(name, key, tuple(r64.shape), "rms %.3g d32 %.3g dbf16 %.3g df16 %.3g" % (
                data[f"{name}.rms_{key}"], data[f"{name}.d32_{key}"], data[f"{name}.dbf16_{key}"],
                data[f"{name}.df16_{key}"]), flush=True)
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
