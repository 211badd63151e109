"""CPU: the ConvNeXt backbone's module surface: state-dict keys and the torch composite against the imported reference
(tests/golden/convnext_cases.npz, make_convnext_golden.py), checkpoint loading, freezing, stochastic depth, argument
checks of the HIP entries (no launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import convnext_cases as CC
from salience_detr_amd import _hip
from salience_detr_amd.convnext import CNBlockConfig, ConvNeXtBackbone

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convnext_cases.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(G))


def _model(name, **kw):
    m = ConvNeXtBackbone(None, return_indices=CC.CASES[name][2], block_setting=[CNBlockConfig(*r) for r in CC.setting(name)],
                         **kw)
    m.load_state_dict(CC.state(m.state_dict(), name))
    return m


@pytest.mark.parametrize("name", list(CC.CASES))
def test_state_dict_keys_channels_and_names(gold, name):
    m = _model(name)
    assert list(m.state_dict()) == list(gold[f"{name}.keys"])
    ret = CC.CASES[name][2]
    assert m.num_channels == [CC.CASES[name][0][i] for i in ret]
    with torch.no_grad():
        out = m.forward_torch(torch.zeros(1, 3, 32, 32))
    assert list(out) == [f"features.{2 * i + 1}" for i in ret]
    assert [t.shape[1] for t in out.values()] == m.num_channels


def test_archs_and_lazy_export():
    import salience_detr_amd
    assert salience_detr_amd.ConvNeXtBackbone is ConvNeXtBackbone
    m = ConvNeXtBackbone("conv_t", return_indices=(1, 2))
    assert m.num_channels == [192, 384] and len(m.features) == 6 and len(m.features[5]) == 9
    assert not any(k.startswith(("avgpool", "classifier")) for k in m.state_dict())
    # stochastic depth counts the blocks of the whole setting (18), also when the last stage is dropped
    assert m.features[5][8].stochastic_depth.p == pytest.approx(0.1 * 14 / 17.0)
    assert ConvNeXtBackbone("conv_t", stochastic_depth_prob=0.0).features[7][2].stochastic_depth.p == 0.0
    assert ConvNeXtBackbone("conv_t", return_indices=(0,), layer_scale=0.5).features[1][0].layer_scale.detach()[0].item() == 0.5
    with pytest.raises(ValueError):
        ConvNeXtBackbone("conv_x")
    with pytest.raises(ValueError):
        ConvNeXtBackbone(None)
    with pytest.raises(ValueError):
        ConvNeXtBackbone("conv_t").set_dtype(torch.int32)
    assert ConvNeXtBackbone("conv_t").hip_form()
    assert not ConvNeXtBackbone(None, return_indices=(0,), block_setting=[CNBlockConfig(48, None, 1)]).hip_form()


@pytest.mark.parametrize("name", list(CC.CASES))
def test_composite_is_the_references_network(gold, name):
    m = _model(name).eval()
    canvas, _ = CC.canvas_and_mask(CC.images(name))
    with torch.no_grad():
        out = m.forward_torch(canvas)
    for key, t in out.items():
        ref = gold[f"{name}.ref_{key}"]
        flat = t.reshape(-1).double()
        flat = flat if ref.size == flat.numel() else flat[CC.sub_index(flat.numel())]
        d = (flat - torch.from_numpy(ref).double()).abs().max().item()
        bound = max(2 * gold[f"{name}.d32_{key}"], 1e-5 * np.abs(ref).max())
        assert d <= bound, (key, d, bound)


def test_nonstrict_loading(tmp_path):
    m = _model("cnt4")
    sd = CC.state(m.state_dict(), "cnt4", salt=3)
    full = dict(sd)
    full["classifier.2.weight"], full["classifier.2.bias"] = torch.zeros(1000, 768), torch.zeros(1000)
    wrong = "features.1.0.block.3.weight"
    full[wrong] = torch.zeros(7, 7)
    path = tmp_path / "cn.pth"
    torch.save({"model": full}, path)
    setting = [CNBlockConfig(*r) for r in CC.setting("cnt4")]
    torch.manual_seed(0)
    loaded = ConvNeXtBackbone(None, weights=str(path), block_setting=setting)
    torch.manual_seed(0)
    fresh = ConvNeXtBackbone(None, block_setting=setting)
    for k, v in loaded.state_dict().items():
        assert torch.equal(v, fresh.state_dict()[k] if k == wrong else sd[k]), k
    by_dict = ConvNeXtBackbone(None, weights=sd, block_setting=setting)
    assert all(torch.equal(v, sd[k]) for k, v in by_dict.state_dict().items())
    with pytest.raises(FileNotFoundError):
        ConvNeXtBackbone("conv_t", weights=str(tmp_path / "missing.pth"))


def test_freezing_follows_freeze_indices():
    m = ConvNeXtBackbone(None, freeze_indices=(0, 2), block_setting=[CNBlockConfig(*r) for r in CC.setting("cnt4")])
    frozen = {n.split(".")[1] for n, p in m.named_parameters() if not p.requires_grad}
    assert frozen == {"0", "1", "2", "5", "6"}
    assert {n.split(".")[1] for n, p in m.named_parameters() if p.requires_grad} == {"3", "4", "7"}
    m.train()
    free = ConvNeXtBackbone(None, block_setting=[CNBlockConfig(*r) for r in CC.setting("cnt4")])
    assert all(p.requires_grad for p in free.parameters())
    last = ConvNeXtBackbone(None, freeze_indices=(3,), block_setting=[CNBlockConfig(*r) for r in CC.setting("cnt4")])
    assert {n.split(".")[1] for n, p in last.named_parameters() if not p.requires_grad} == {"0", "7"}


def test_stochastic_depth_in_training():
    setting = [CNBlockConfig(96, None, 2)]
    x = CC.syn.det_randn("convnext.sd.x", (6, 3, 16, 16))
    m = ConvNeXtBackbone(None, return_indices=(0,), block_setting=setting, stochastic_depth_prob=0.0, layer_scale=0.5)
    a = m.eval()(x)["features.1"]
    b = m.train()(x)["features.1"]
    assert b.grad_fn is not None and torch.equal(a, b)
    p = 0.5
    m = ConvNeXtBackbone(None, return_indices=(0,), block_setting=setting, stochastic_depth_prob=p, layer_scale=0.5)
    blk = m.features[1][1].train()
    assert blk.stochastic_depth.p == p
    torch.manual_seed(1)
    with torch.no_grad():
        inp = m.features[0](x)
        branch = blk.layer_scale * blk.block(inp)
        out = blk(inp.clone())
    dropped = kept = 0
    for n in range(x.shape[0]):
        if torch.equal(out[n], inp[n]):
            dropped += 1
        else:
            assert torch.equal(out[n], branch[n] * (1.0 / (1.0 - p)) + inp[n])
            kept += 1
    assert dropped > 0 and kept > 0


def test_hip_form_on_cpu_tensor_raises():
    m = _model("cnt4").eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP"):
        m(torch.zeros(1, 3, 64, 64))


def _op(**kw):
    base = dict(kind=0, x=16, weight=16, bias=16, gamma=16, beta=16, residual=None, out=16, out_nchw=None, batch=2,
                in_channels=64, height=8, width=8, out_channels=64, kernel_size=2, stride=2, x_nchw=0, out_f32=0, splits=0,
                eps=1e-6)
    base.update(kw)
    return (_hip.ConvnextOpStruct * 1)(_hip.ConvnextOpStruct(**base))


def test_abi_entries_reject_bad_arguments():
    for lib in (_hip.lib(), _hip.lib(torch.float16)):
        ok = lambda arr, precision=0: lib.sdetr_convnext_workspace_bytes(arr, 1, precision)
        for kind in (0, 1, 2, 3):
            assert ok(_op(kind=kind, kernel_size=1, stride=1)) >= 0
            assert ok(_op(kind=kind, kernel_size=1, stride=1, x=None)) == -1                 # null pointer
            assert ok(_op(kind=kind, kernel_size=1, stride=1, out=None)) == -1
            assert ok(_op(kind=kind, kernel_size=1, stride=1, in_channels=48)) == -1         # C % 32
            assert "32" in lib.sdetr_last_error().decode()
            assert ok(_op(kind=kind, kernel_size=1, stride=1), 2) == -1                      # precision
        assert ok(_op(kind=0, kernel_size=2, stride=1)) == -1                                # kernel != stride
        assert "stride" in lib.sdetr_last_error().decode()
        assert ok(_op(kind=0, kernel_size=4, stride=4, x_nchw=1, in_channels=3)) >= 0        # the stem
        assert ok(_op(kind=0, kernel_size=5, stride=5)) == -1
        assert ok(_op(kind=1, kernel_size=1, stride=1, residual=16)) == -1                   # GELU takes no residual
        assert ok(_op(kind=2, gamma=None)) == -1 and ok(_op(kind=3, beta=None)) == -1
        assert ok(_op(kind=2, in_channels=3104)) == -1                                       # past the widest tile
        assert ok(_op(kind=7)) == -1
        assert ok(_op(kind=2, x=8)) == -1                                                    # alignment
        assert lib.sdetr_convnext_run(None, _op(kind=7), 1, 0, None, 0) == -1
        assert lib.sdetr_convnext_run(None, None, 0, 0, None, 0) == -1
        assert lib.sdetr_convnext_op_run(None, None, 0, None, 0) == -1
        assert lib.sdetr_convnext_op_run(None, _op(kind=0, kernel_size=3, stride=2), 0, None, 0) == -1
        # a split reduction needs its workspace
        assert lib.sdetr_convnext_op_run(None, _op(kind=0, kernel_size=1, stride=1, in_channels=256, splits=2), 0, None, 0) == -1
        th, cc, sw = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        assert lib.sdetr_convnext_dw_tile(48, None, None, None) == -1
        for c, want in ((96, (16, 64, 8)), (192, (16, 32, 4)), (384, (8, 32, 2)), (768, (4, 64, 2)), (1536, (2, 64, 1))):
            nbytes = lib.sdetr_convnext_dw_tile(c, ctypes.byref(th), ctypes.byref(cc), ctypes.byref(sw))
            assert (th.value, cc.value, sw.value) == want
            assert nbytes == 8 * th.value * c * 4 + cc.value * ((th.value + 6) * 14 * 4 + 196) <= 150000
        for c in range(32, 3073, 32):
            assert 0 < lib.sdetr_convnext_dw_tile(c, None, None, None) <= 150000
