"""CPU: ``SwinBackbone`` as a module (keys, archs, the composite against the imported reference, loading, freezing,
stochastic depth) and the argument checks of the ``sdetr_swin_*`` entry points, which need no GPU."""
import os

import numpy as np
import pytest
import torch

import swin_cases as SC
from salience_detr_amd import _hip
from salience_detr_amd.swin import ARCHS, SwinBackbone

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "swin_cases.npz")


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(G))


def _model(name, **kw):
    m = SwinBackbone(None, return_indices=SC.CASES[name][1], **dict(SC.config(name), **kw))
    m.load_state_dict(SC.state(m.state_dict(), name))
    return m


@pytest.mark.parametrize("name", list(SC.CASES))
def test_state_dict_keys_channels_and_names(gold, name):
    m = _model(name)
    assert list(m.state_dict()) == list(gold[f"{name}.keys"])
    index = m.state_dict()["0.features.1.0.attn.relative_position_index"]
    assert not index.is_floating_point()
    ret = SC.CASES[name][1]
    assert m.num_channels == [SC.CASES[name][0]["embed_dim"] * 2 ** i for i in ret]
    with torch.no_grad():
        out = m.eval().forward_torch(torch.zeros(1, 3, 32, 32))
    assert list(out) == [f"features.{2 * i + 1}" for i in ret]
    assert [t.shape[1] for t in out.values()] == m.num_channels
    assert all(t.is_contiguous() and t.dtype == torch.float32 for t in out.values())


def test_state_keeps_the_index_and_sets_the_table():
    m = SwinBackbone(None, return_indices=(0,), **SC.config("w7"))
    own = m.state_dict()
    sd = SC.state(own, "w7")
    key = "0.features.1.1.attn.relative_position_index"
    assert torch.equal(sd[key], own[key]) and int(sd[key].max()) == 13 * 13 - 1
    table = sd["0.features.1.1.attn.relative_position_bias_table"]
    assert table.abs().max().item() > 0.9 and table.min().item() < -0.5


# arch -> (embed_dim, depths, heads, window, stochastic depth)
TABLE = {
    "swin_t": (96, (2, 2, 6, 2), (3, 6, 12, 24), 7, 0.2),
    "swin_s": (96, (2, 2, 18, 2), (3, 6, 12, 24), 7, 0.3),
    "swin_b": (128, (2, 2, 18, 2), (4, 8, 16, 32), 7, 0.5),
    "swin_l": (192, (2, 2, 18, 2), (6, 12, 24, 48), 7, 0.2),
    "swin_b_384": (128, (2, 2, 18, 2), (4, 8, 16, 32), 12, 0.2),
    "swin_l_384": (192, (2, 2, 18, 2), (6, 12, 24, 48), 12, 0.2),
}


@pytest.mark.parametrize("arch", list(TABLE))
def test_every_arch_of_the_table(arch):
    dim, depths, heads, window, sd = TABLE[arch]
    assert set(TABLE) == set(ARCHS)
    with torch.device("meta"):
        m = SwinBackbone(arch, return_indices=(1, 2))
    assert m.num_channels == [2 * dim, 4 * dim]
    features = m.body.features
    assert len(features) == 6                                       # stem, 3 stages, 2 mergings: the last stage is not held
    total, seen = sum(depths), 0
    for i in range(3):
        blocks = features[2 * i + 1]
        assert len(blocks) == depths[i]
        for j, blk in enumerate(blocks):
            at = blk.attn
            assert at.num_heads == heads[i] and at.qkv.in_features == dim * 2 ** i == 32 * heads[i]
            assert at.window_size == [window, window] and at.shift_size == ([0, 0] if j % 2 == 0 else [window // 2] * 2)
            assert tuple(at.relative_position_bias_table.shape) == ((2 * window - 1) ** 2, heads[i])
            assert blk.mlp[0].out_features == 4 * dim * 2 ** i and blk.mlp[3].out_features == dim * 2 ** i
            assert blk.stochastic_depth.p == pytest.approx(sd * seen / (total - 1))     # counts the whole depths
            seen += 1
    assert tuple(features[2].reduction.weight.shape) == (2 * dim, 4 * dim) and features[2].reduction.bias is None
    assert m.hip_form()


def test_lazy_export_overrides_and_argument_checks():
    import salience_detr_amd
    assert salience_detr_amd.SwinBackbone is SwinBackbone
    m = SwinBackbone("swin_t", return_indices=(0,), stochastic_depth_prob=0.0)
    assert m.body.features[1][1].stochastic_depth.p == 0.0 and not any("url" in k for k in m.config)
    for v2 in ("swin_v2_t", "swin_v2_b"):
        with pytest.raises(ValueError, match="V2 is not built"):
            SwinBackbone(v2)
    with pytest.raises(ValueError):
        SwinBackbone("swin_x")
    with pytest.raises(ValueError):
        SwinBackbone(None)
    with pytest.raises(ValueError):
        SwinBackbone("swin_t", return_indices=(4,))
    with pytest.raises(ValueError):
        SwinBackbone("swin_t", return_indices=())
    with pytest.raises(ValueError):
        SwinBackbone("swin_t", return_indices=(0,)).set_dtype(torch.int32)
    # another window, another head dimension or another norm leave the HIP form: the composite runs them
    base = dict(embed_dim=64, depths=(1,), num_heads=(2,), window_size=(7, 7))
    assert SwinBackbone(None, return_indices=(0,), **base).hip_form()
    assert not SwinBackbone(None, return_indices=(0,), **dict(base, window_size=(8, 8))).hip_form()
    other = SwinBackbone(None, return_indices=(0,), **dict(base, num_heads=(4,))).eval()
    assert not other.hip_form()
    with torch.no_grad():
        assert tuple(other(torch.zeros(1, 3, 32, 32))["features.1"].shape) == (1, 64, 8, 8)
    assert not SwinBackbone(None, return_indices=(0,), norm_layer=torch.nn.Identity, **base).hip_form()


@pytest.mark.parametrize("name", list(SC.CASES))
def test_composite_is_the_references_network(gold, name):
    m = _model(name).eval()
    with torch.no_grad():
        out = m.forward_torch(SC.canvas(name))
    for key, t in out.items():
        ref = gold[f"{name}.ref_{key}"]
        flat = t.reshape(-1).double()
        flat = flat if ref.size == flat.numel() else flat[SC.sub_index(flat.numel())]
        d = (flat - torch.from_numpy(ref).double()).abs().max().item()
        bound = max(2 * gold[f"{name}.d32_{key}"], 1e-5 * np.abs(ref).max())
        assert d <= bound, (key, d, bound)


def test_nonstrict_loading(tmp_path):
    cfg, ret = SC.config("w12"), (0, 1)
    m = SwinBackbone(None, return_indices=ret, **cfg)
    sd = SC.state(m.state_dict(), "w12", salt=3)
    # a full SwinTransformer checkpoint: its own key names, later stages, norm and head
    full = {k[2:]: v for k, v in sd.items()}
    full["features.4.reduction.weight"], full["norm.weight"], full["head.weight"] = torch.zeros(4, 4), torch.zeros(512), torch.zeros(1000, 512)
    wrong = "0.features.1.0.attn.qkv.weight"
    full[wrong[2:]] = torch.zeros(7, 7)
    path = tmp_path / "swin.pth"
    torch.save({"model": full}, path)
    torch.manual_seed(0)
    loaded = SwinBackbone(None, weights=str(path), return_indices=ret, **cfg)
    torch.manual_seed(0)
    fresh = SwinBackbone(None, return_indices=ret, **cfg)
    for k, v in loaded.state_dict().items():
        assert torch.equal(v, fresh.state_dict()[k] if k == wrong else sd[k]), k
    by_dict = SwinBackbone(None, weights=sd, return_indices=ret, **cfg)
    assert all(torch.equal(v, sd[k]) for k, v in by_dict.state_dict().items())
    with pytest.raises(FileNotFoundError):
        SwinBackbone("swin_t", weights=str(tmp_path / "missing.pth"))


def test_freezing_follows_freeze_indices():
    cfg = SC.config("w12")
    m = SwinBackbone(None, freeze_indices=(0, 2), **cfg)
    frozen = {n.split(".")[2] for n, p in m.named_parameters() if not p.requires_grad}
    assert frozen == {"0", "1", "2", "5", "6"}                      # the stem; stage 0 and 2 with their mergings
    free = {n.split(".")[2] for n, p in m.named_parameters() if p.requires_grad}
    assert free == {"3", "4", "7"}
    assert all(p.requires_grad for p in SwinBackbone(None, **cfg).parameters())
    last = SwinBackbone(None, freeze_indices=(3,), return_indices=(0, 1), **cfg)       # a stage that is not held
    assert {n.split(".")[2] for n, p in last.named_parameters() if not p.requires_grad} == {"0"}
    end = SwinBackbone(None, freeze_indices=(3,), **cfg)                                # the last stage has no merging
    assert {n.split(".")[2] for n, p in end.named_parameters() if not p.requires_grad} == {"0", "7"}


def test_stochastic_depth_in_training():
    cfg = dict(embed_dim=32, depths=(2,), num_heads=(1,), window_size=(7, 7))
    x = SC.syn.det_randn("swin.sd.x", (6, 3, 16, 16))
    m = SwinBackbone(None, return_indices=(0,), stochastic_depth_prob=0.0, **cfg)
    a = m.eval()(x)["features.1"]
    b = m.train()(x)["features.1"]
    assert b.grad_fn is not None and torch.equal(a, b)
    p = 0.5
    m = SwinBackbone(None, return_indices=(0,), stochastic_depth_prob=p, **cfg)
    blk = m.body.features[1][1]
    assert blk.stochastic_depth.p == p and m.body.features[1][0].stochastic_depth.p == 0.0
    with torch.no_grad():
        for t in (blk.mlp[3].weight, blk.mlp[3].bias):
            t.zero_()                               # the second branch contributes nothing: one Bernoulli draw shows
        blk.attn.proj.bias.fill_(0.5)
        inp = m.body.features[0](x)
        branch = blk.attn(blk.norm1(inp))
        assert torch.equal(blk.eval()(inp), inp + branch)           # eval: no draw
        torch.manual_seed(1)
        out = blk.train()(inp)
    dropped = kept = 0
    for n in range(x.shape[0]):
        if torch.equal(out[n], inp[n]):
            dropped += 1
        else:
            assert torch.allclose(out[n], inp[n] + branch[n] * (1.0 / (1.0 - p)), rtol=0, atol=1e-6)
            kept += 1
    assert dropped > 0 and kept > 0


def test_hip_form_on_cpu_tensor_raises():
    m = _model("w12").eval()
    with torch.no_grad(), pytest.raises(RuntimeError, match="HIP"):
        m(torch.zeros(1, 3, 64, 64))


def _op(**kw):
    base = dict(kind=0, x=16, weight=16, bias=16, gamma=16, beta=16, residual=None, table=16, out=32, out_nchw=None, batch=2,
                in_channels=64, height=8, width=8, out_channels=64, kernel_size=1, stride=1, x_nchw=0, out_f32=0, window=7,
                shift=3, heads=2, splits=0, eps=1e-5)
    base.update(kw)
    return (_hip.SwinOpStruct * 1)(_hip.SwinOpStruct(**base))


def test_abi_entries_reject_bad_arguments():
    for lib in (_hip.lib(), _hip.lib(torch.float16)):
        err = lambda: lib.sdetr_last_error().decode()
        ok = lambda arr, precision=1: lib.sdetr_swin_workspace_bytes(arr, 1, precision)
        for kind in range(6):
            assert ok(_op(kind=kind)) >= 0, (kind, err())
            assert ok(_op(kind=kind), 0) >= 0, (kind, err())
            assert ok(_op(kind=kind, x=None)) == -1 and "null" in err()                            # null pointer
            assert ok(_op(kind=kind, out=None)) == -1 and "null" in err()
            bad = 44 if kind == 5 else 48                                                          # C % 32 (kind 5: 4 C % 32)
            assert ok(_op(kind=kind, in_channels=bad, heads=1)) == -1 and "32" in err()
            assert ok(_op(kind=kind), 2) == -1 and "precision" in err()                            # precision
            assert ok(_op(kind=kind, x=8)) == -1 and "aligned" in err()                            # alignment
        assert ok(_op(kind=4, heads=4)) == -1 and "head dimension" in err()                        # 64 channels / 4 heads = 16
        assert ok(_op(kind=4, heads=1)) == -1 and "head dimension" in err()
        for window in (0, 6, 8, 14):
            assert ok(_op(kind=4, window=window, shift=0)) == -1 and "window" in err()
        assert ok(_op(kind=4, window=12, shift=6)) == 0 and ok(_op(kind=4, window=7, shift=0)) == 0
        assert ok(_op(kind=4, shift=7)) == -1 and ok(_op(kind=4, shift=-1)) == -1
        assert ok(_op(kind=4, table=None)) == -1 and ok(_op(kind=4, bias=None)) == -1
        assert ok(_op(kind=4, out=16)) == -1 and "alias" in err()
        assert ok(_op(kind=4, table=20)) == -1 and "aligned" in err()
        assert ok(_op(kind=3, gamma=None)) == -1 and ok(_op(kind=5, beta=None)) == -1
        assert ok(_op(kind=3, in_channels=3104)) == -1 and ok(_op(kind=5, in_channels=776)) == -1  # past the widest row
        assert ok(_op(kind=5, in_channels=768)) == 0 and ok(_op(kind=5, in_channels=8)) == 0
        assert ok(_op(kind=1, residual=16)) == -1 and ok(_op(kind=2, out_nchw=16)) == -1
        assert ok(_op(kind=0, residual=16, out_nchw=16)) >= 0
        assert ok(_op(kind=0, x_nchw=1, in_channels=3, height=50, width=120, kernel_size=4, stride=4)) >= 0   # the stem
        assert ok(_op(kind=0, kernel_size=4, stride=2)) == -1 and ok(_op(kind=0, kernel_size=5, stride=5)) == -1
        assert ok(_op(kind=0, x_nchw=1, in_channels=3, height=3, width=8, kernel_size=4, stride=4)) == -1      # empty output
        assert ok(_op(kind=0, in_channels=256, splits=2)) == 2 * 128 * 64 * 4
        assert ok(_op(kind=9)) == -1 and "kind" in err()
        # run / op_run: a plan is validated before any launch, a workspace that is too small is refused
        assert lib.sdetr_swin_run(None, _op(kind=9), 1, 1, None, 0) == -1
        assert lib.sdetr_swin_run(None, None, 0, 1, None, 0) == -1
        assert lib.sdetr_swin_op_run(None, None, 1, None, 0) == -1
        assert lib.sdetr_swin_run(None, _op(kind=0, in_channels=256, splits=2), 1, 1, 16, 512) == -1 and "workspace" in err()
        assert lib.sdetr_swin_run(None, _op(kind=2, in_channels=256, splits=2), 1, 1, None, 0) == -1 and "workspace" in err()
        assert lib.sdetr_swin_op_run(None, _op(kind=0, in_channels=256, splits=2), 1, None, 0) == -1 and "workspace" in err()
        assert lib.sdetr_swin_op_run(None, _op(kind=4, window=9), 1, None, 0) == -1
