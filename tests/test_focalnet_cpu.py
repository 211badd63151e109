"""CPU: the FocalNet backbone's module surface: state-dict keys and the torch composite against the imported reference
(tests/golden/focalnet_cases.npz, make_focalnet_golden.py), the arch table, checkpoint loading, freezing, stochastic
depth, argument checks of the HIP entries (no launch)."""
import os

import numpy as np
import pytest
import torch

import focalnet_cases as FC
from salience_detr_amd import _hip
from salience_detr_amd.focalnet import ARCHS, FocalNetBackbone

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "focalnet_cases.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(G))


def _model(name, **kw):
    m = FocalNetBackbone(None, return_indices=FC.CASES[name][1], **dict(FC.config(name), **kw))
    m.load_state_dict(FC.state(m.state_dict(), name))
    return m


@pytest.mark.parametrize("name", list(FC.CASES))
def test_state_dict_keys_channels_and_names(gold, name):
    m = _model(name)
    assert list(m.state_dict()) == list(gold[f"{name}.keys"])
    ret = FC.CASES[name][1]
    assert m.num_channels == [FC.CASES[name][0]["embed_dim"] * 2 ** i for i in ret]
    with torch.no_grad():
        out = m.eval().forward_torch(torch.zeros(1, 3, 32, 32))
    assert list(out) == [f"layers.{i}.blocks" for i in ret]
    assert [t.shape[1] for t in out.values()] == m.num_channels
    assert all(t.is_contiguous() and t.dtype == torch.float32 for t in out.values())


# arch -> (embed_dim, depths, focal levels, first kernel, stochastic depth, large form, in-modulation LN, normalised)
TABLE = {
    "focalnet_tiny_srf": (96, (2, 2, 6, 2), 2, 3, 0.2, False, False, False),
    "focalnet_tiny_lrf": (96, (2, 2, 18, 2), 3, 3, 0.2, False, False, False),
    "focalnet_small_srf": (96, (2, 2, 18, 2), 2, 3, 0.3, False, False, False),
    "focalnet_small_lrf": (96, (2, 2, 18, 2), 3, 3, 0.3, False, False, False),
    "focalnet_base_srf": (128, (2, 2, 18, 2), 2, 3, 0.5, False, False, False),
    "focalnet_base_lrf": (128, (2, 2, 18, 2), 3, 3, 0.5, False, False, False),
    "focalnet_large_lrf": (192, (2, 2, 18, 2), 3, 5, 0.5, True, False, False),
    "focalnet_large_lrf_fl4": (192, (2, 2, 18, 2), 4, 3, 0.5, True, False, True),
    "focalnet_xlarge_lrf": (256, (2, 2, 18, 2), 3, 5, 0.5, True, False, False),
    "focalnet_xlarge_lrf_fl4": (256, (2, 2, 18, 2), 4, 3, 0.5, True, False, True),
    "focalnet_huge_fl3": (352, (2, 2, 18, 2), 3, 3, 0.5, True, True, False),
    "focalnet_huge_fl4": (352, (2, 2, 18, 2), 4, 3, 0.5, True, True, False),
}


@pytest.mark.parametrize("arch", list(TABLE))
def test_every_arch_of_the_table(arch):
    dim, depths, levels, first, sd, big, mod_ln, normed = TABLE[arch]
    assert set(TABLE) == set(ARCHS)
    m = FocalNetBackbone(arch, return_indices=(1, 2))
    assert m.num_channels == [2 * dim, 4 * dim]
    layers = m.body.layers
    assert len(layers) == 3 and [len(s.blocks) for s in layers] == list(depths[:3])     # the last stage is not held
    assert hasattr(layers[1], "downsample") and not hasattr(layers[2], "downsample")
    total, seen = sum(depths), 0
    for i, stage in enumerate(layers):
        for blk in stage.blocks:
            mod = blk.modulation
            assert [layer[0].kernel_size[0] for layer in mod.focal_layers] == [first + 2 * l for l in range(levels)]
            assert tuple(mod.f.weight.shape) == (2 * dim * 2 ** i + levels + 1, dim * 2 ** i)
            assert tuple(mod.h.weight.shape) == (dim * 2 ** i, dim * 2 ** i, 1, 1)
            assert blk.drop_path.p == pytest.approx(sd * seen / (total - 1))            # counts the whole depths
            assert blk.use_postln == big and blk.use_layerscale == big and isinstance(blk.gamma_1, torch.nn.Parameter) == big
            assert hasattr(mod, "ln") == mod_ln and mod.normalize_modulator == normed
            seen += 1
    assert m.body.patch_embed.proj.kernel_size == ((7, 7) if big else (4, 4))
    assert layers[0].downsample.proj.kernel_size == ((3, 3) if big else (2, 2))
    assert m.hip_form()


def test_lazy_export_overrides_and_argument_checks():
    import salience_detr_amd
    assert salience_detr_amd.FocalNetBackbone is FocalNetBackbone
    m = FocalNetBackbone("focalnet_tiny_srf", return_indices=(0,), stochastic_depth_prob=0.0, focal_levels=(1, 1, 1, 1))
    assert m.body.layers[0].blocks[1].drop_path.p == 0.0 and len(m.body.layers[0].blocks[0].modulation.focal_layers) == 1
    assert not any("url" in k for k in m.config)
    with pytest.raises(ValueError):
        FocalNetBackbone("focalnet_x")
    with pytest.raises(ValueError):
        FocalNetBackbone(None)
    with pytest.raises(ValueError):
        FocalNetBackbone("focalnet_tiny_srf", return_indices=(4,))
    with pytest.raises(ValueError):
        FocalNetBackbone("focalnet_tiny_srf", return_indices=())
    with pytest.raises(ValueError):
        FocalNetBackbone("focalnet_tiny_srf", return_indices=(0,)).set_dtype(torch.int32)
    # widths that are no multiple of 32, or a focal kernel the level kernel does not have, leave the HIP form
    assert not FocalNetBackbone(None, return_indices=(0,), embed_dim=48, depths=(1,)).hip_form()
    assert not FocalNetBackbone(None, return_indices=(0,), embed_dim=64, depths=(1,), focal_windows=(11,)).hip_form()
    assert not FocalNetBackbone(None, return_indices=(0,), embed_dim=64, depths=(1,), norm_layer=torch.nn.Identity).hip_form()


@pytest.mark.parametrize("name", list(FC.CASES))
def test_composite_is_the_references_network(gold, name):
    m = _model(name).eval()
    with torch.no_grad():
        out = m.forward_torch(FC.canvas(name))
    for key, t in out.items():
        ref = gold[f"{name}.ref_{key}"]
        flat = t.reshape(-1).double()
        flat = flat if ref.size == flat.numel() else flat[FC.sub_index(flat.numel())]
        d = (flat - torch.from_numpy(ref).double()).abs().max().item()
        bound = max(2 * gold[f"{name}.d32_{key}"], 1e-5 * np.abs(ref).max())
        assert d <= bound, (key, d, bound)


def test_nonstrict_loading(tmp_path):
    m = _model("hg")
    sd = FC.state(m.state_dict(), "hg", salt=3)
    full = dict(sd)
    full["0.layers.3.downsample.proj.weight"], full["head.weight"] = torch.zeros(4, 4), torch.zeros(1000, 512)
    wrong = "0.layers.0.blocks.0.modulation.f.weight"
    full[wrong] = torch.zeros(7, 7)
    path = tmp_path / "fn.pth"
    torch.save({"model": full}, path)
    cfg, ret = FC.config("hg"), FC.CASES["hg"][1]
    torch.manual_seed(0)
    loaded = FocalNetBackbone(None, weights=str(path), return_indices=ret, **cfg)
    torch.manual_seed(0)
    fresh = FocalNetBackbone(None, return_indices=ret, **cfg)
    for k, v in loaded.state_dict().items():
        assert torch.equal(v, fresh.state_dict()[k] if k == wrong else sd[k]), k
    by_dict = FocalNetBackbone(None, weights=sd, return_indices=ret, **cfg)
    assert all(torch.equal(v, sd[k]) for k, v in by_dict.state_dict().items())
    with pytest.raises(FileNotFoundError):
        FocalNetBackbone("focalnet_tiny_srf", weights=str(tmp_path / "missing.pth"))


def test_freezing_follows_freeze_indices():
    cfg = FC.config("srf")
    m = FocalNetBackbone(None, freeze_indices=(0, 2), **cfg)
    frozen = {".".join(n.split(".")[1:3]) for n, p in m.named_parameters() if not p.requires_grad}
    assert frozen == {"patch_embed.proj", "patch_embed.norm", "layers.0", "layers.2"}
    free = {".".join(n.split(".")[:3]) for n, p in m.named_parameters() if p.requires_grad}
    assert free == {"0.layers.1", "0.layers.3", "1.norm0.weight", "1.norm0.bias", "1.norm1.weight", "1.norm1.bias",
                    "1.norm2.weight", "1.norm2.bias", "1.norm3.weight", "1.norm3.bias"}
    assert any(n.startswith("0.layers.2.downsample") for n, p in m.named_parameters() if not p.requires_grad)
    assert all(p.requires_grad for p in FocalNetBackbone(None, **cfg).parameters())
    last = FocalNetBackbone(None, freeze_indices=(3,), return_indices=(0, 1), **cfg)   # a stage that is not held
    assert {n.split(".")[1] for n, p in last.named_parameters() if not p.requires_grad} == {"patch_embed"}


def test_stochastic_depth_in_training():
    cfg = dict(embed_dim=32, depths=(2,), focal_levels=(2,), focal_windows=(3,), use_postln=True, use_layerscale=True)
    x = FC.syn.det_randn("focalnet.sd.x", (6, 3, 16, 16))
    m = FocalNetBackbone(None, return_indices=(0,), stochastic_depth_prob=0.0, **cfg)
    a = m.eval()(x)["layers.0.blocks"]
    b = m.train()(x)["layers.0.blocks"]
    assert b.grad_fn is not None and torch.equal(a, b)
    p = 0.5
    m = FocalNetBackbone(None, return_indices=(0,), stochastic_depth_prob=p, **cfg)
    blk = m.body.layers[0].blocks[1].train()
    assert blk.drop_path.p == p and m.body.layers[0].blocks[0].drop_path.p == 0.0
    with torch.no_grad():
        blk.gamma_1.fill_(0.5)
        blk.gamma_2.zero_()                         # the second branch contributes nothing: one Bernoulli draw shows
        inp = m.body.patch_embed(x.permute(0, 2, 3, 1))
        branch = blk.gamma_1 * blk.norm1(blk.modulation(inp))
        torch.manual_seed(1)
        out = blk(inp)
    dropped = kept = 0
    for n in range(x.shape[0]):
        if torch.equal(out[n], inp[n]):
            dropped += 1
        else:
            assert torch.allclose(out[n], inp[n] + branch[n] * (1.0 / (1.0 - p)), rtol=0, atol=1e-6)
            kept += 1
    assert dropped > 0 and kept > 0


def test_hip_form_on_cpu_tensor_raises():
    m = _model("hg").eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP"):
        m(torch.zeros(1, 3, 64, 64))


def _op(**kw):
    base = dict(kind=0, x=16, weight=16, bias=16, gamma=16, beta=16, residual=None, q=16, out=16, out2=16, batch=2,
                in_channels=64, height=8, width=8, out_channels=64, out_height=8, out_width=8, kernel_size=1, stride=1,
                padding=0, x_nchw=0, out_f32=0, x_ld=64, q_ld=64, accumulate=0, last=0, splits=0, eps=1e-5)
    base.update(kw)
    return (_hip.FocalnetOpStruct * 1)(_hip.FocalnetOpStruct(**base))


GOOD = {0: {}, 1: {}, 2: {}, 3: dict(kernel_size=3), 4: {}, 5: dict(out2=None), 6: dict(out2=None), 7: {}}


def test_abi_entries_reject_bad_arguments():
    for lib in (_hip.lib(), _hip.lib(torch.float16)):
        err = lambda: lib.sdetr_last_error().decode()
        ok = lambda arr, precision=1: lib.sdetr_focalnet_workspace_bytes(arr, 1, precision)
        for kind, kw in GOOD.items():
            assert ok(_op(kind=kind, **kw)) >= 0, (kind, err())
            assert ok(_op(kind=kind, **dict(kw, x=None))) == -1 and "null" in err()                # null pointer
            assert kind == 3 or ok(_op(kind=kind, **dict(kw, out=None))) == -1           # (a last level keeps no ctx)
            assert ok(_op(kind=kind, **dict(kw, in_channels=48))) == -1 and "32" in err()          # C % 32
            assert ok(_op(kind=kind, **kw), 2) == -1 and "precision" in err()                      # precision
            assert ok(_op(kind=kind, **dict(kw, x=8))) == -1 and "aligned" in err()                # alignment
        for k in (1, 4, 11):
            assert ok(_op(kind=3, kernel_size=k)) == -1 and "kernel size" in err()                 # unsupported k
        for k in (3, 5, 7, 9):
            assert ok(_op(kind=3, kernel_size=k)) == 0
        assert ok(_op(kind=3, kernel_size=3, last=1)) == 2 * 1 * 64 * 4                            # one 8 x 16 tile
        assert ok(_op(kind=4)) == 2 * 1 * 64 * 4 + 2 * 64 * 4
        assert ok(_op(kind=3, kernel_size=3, q=None)) == -1 and ok(_op(kind=3, kernel_size=3, out2=None)) == -1
        assert ok(_op(kind=3, kernel_size=3, out=None)) == 0                                       # the last level keeps no ctx
        assert ok(_op(kind=3, kernel_size=3, x_ld=32)) == -1                                       # rows shorter than C
        assert ok(_op(kind=3, kernel_size=3, in_channels=3104, x_ld=3104)) == -1                   # past the widest row
        assert ok(_op(kind=2, q=None)) == -1 and ok(_op(kind=2, q_ld=32)) == -1
        assert ok(_op(kind=5, gamma=None, out2=None)) == -1 and ok(_op(kind=6, beta=None, out2=None)) == -1
        assert ok(_op(kind=5), 0) == -1                                                            # 16-bit copy in fp32 mode
        assert ok(_op(kind=6)) == -1 and ok(_op(kind=7), 0) == -1
        assert ok(_op(kind=1, residual=16)) == -1
        assert ok(_op(kind=9)) == -1 and "kind" in err()
        # the patch embeddings: the output size is the op's own, between the floor size and the padded input's
        stem = dict(kind=0, x_nchw=1, in_channels=3, height=50, width=77, kernel_size=7, stride=4, padding=2)
        assert ok(_op(out_height=13, out_width=20, **stem)) >= 0 and ok(_op(out_height=12, out_width=19, **stem)) >= 0
        assert ok(_op(out_height=14, out_width=20, **stem)) == -1 and ok(_op(out_height=11, out_width=20, **stem)) == -1
        assert ok(_op(kind=0, height=13, width=21, kernel_size=3, stride=2, padding=1, out_height=7, out_width=11)) >= 0
        assert ok(_op(kind=0, kernel_size=8, stride=4, padding=0, out_height=1, out_width=1)) == -1
        # run / op_run: a plan is validated before any launch, a workspace that is too small is refused
        assert lib.sdetr_focalnet_run(None, _op(kind=9), 1, 1, None, 0) == -1
        assert lib.sdetr_focalnet_run(None, None, 0, 1, None, 0) == -1
        assert lib.sdetr_focalnet_op_run(None, None, 1, None, 0) == -1
        assert lib.sdetr_focalnet_run(None, _op(kind=4), 1, 1, 16, 512) == -1 and "workspace" in err()
        assert lib.sdetr_focalnet_run(None, _op(kind=3, kernel_size=9, last=1), 1, 1, None, 0) == -1 and "workspace" in err()
        assert lib.sdetr_focalnet_op_run(None, _op(kind=4), 1, None, 0) == -1 and "workspace" in err()
        assert lib.sdetr_focalnet_op_run(None, _op(kind=3, kernel_size=3, last=1), 1, 16, 16) == -1 and "workspace" in err()
        assert lib.sdetr_focalnet_op_run(None, _op(kind=0, in_channels=256, splits=2), 1, None, 0) == -1 and "workspace" in err()
        assert lib.sdetr_focalnet_op_run(None, _op(kind=3, kernel_size=4), 1, None, 0) == -1
