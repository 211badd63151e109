"""CPU: the ConvNeXt backbone's training interface (``ConvNeXtBackbone.set_train_form``), the fixture's case list, the
two identities the backward rests on, and the bound struct."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import convnext_train_cases as TC
from salience_detr_amd import _hip
from salience_detr_amd.convnext import CNBlock, CNBlockConfig, ConvNeXtBackbone


def _model(case="ct1", **kw):
    kw.setdefault("freeze_indices", TC.FREEZE)
    return ConvNeXtBackbone(None, return_indices=TC.RETURN, block_setting=[CNBlockConfig(*r) for r in TC.setting(case)], **kw)


def test_fixture_matches_the_case_list():
    gold = np.load(TC.GOLDEN)
    assert os.path.getsize(TC.GOLDEN) <= 1 << 20
    for case in TC.CASES:
        names = [str(n) for n in gold[f"{case}.names"]]
        m = _model(case)
        assert names == [n for n, p in m.named_parameters() if p.requires_grad]
        assert names == TC.trainable_names([n for n, _ in m.named_parameters()])
        shapes = dict((n, p.shape) for n, p in m.named_parameters())
        for n in names:
            assert gold[f"{case}.g:{n}"].shape == (min(shapes[n].numel(), TC.STORE),), n
            assert float(gold[f"{case}.d32:{n}"]) < 1e-4 and float(gold[f"{case}.dbf16:{n}"]) < 0.1, n
    assert {k.split(".")[0] for k in gold.files} == set(TC.CASES)


def test_set_train_form_and_the_reasons():
    m = _model()
    assert m.train_form == "torch" and m.set_train_form("hip") is m and m.train_form == "hip"
    with pytest.raises(ValueError):
        m.set_train_form("cuda")
    assert m.hip_train_reason() is None and m.hip_train_form()
    assert "stem" in _model(freeze_indices=()).hip_train_reason()
    assert "float16" in _model().set_dtype(torch.float16).hip_train_reason()
    assert _model().set_dtype(torch.bfloat16).hip_train_form()
    x = torch.zeros(1, 3, 64, 64, requires_grad=True)
    assert "input requires" in m.hip_train_reason(x) and not m.hip_train_form(x)

    class Other(CNBlock):
        pass
    odd = _model()
    odd.features[3][0] = Other(192, 1e-6, 0.0)
    assert "architecture" in odd.hip_train_reason()
    with pytest.raises(RuntimeError, match="architecture"):
        odd.set_train_form("hip")(torch.zeros(1, 3, 64, 64))
    with pytest.raises(RuntimeError, match="stem"):
        _model(freeze_indices=()).set_train_form("hip")(torch.zeros(1, 3, 64, 64))


def test_the_layer_scale_gradient_identity():
    """dg[c] = sum_k dW2'[c, k] W2[c, k] + db2'[c] b2[c], with dW2' / db2' the gradients of the Linear at its output
    gradient dzs = s[n] dy: what kind 7 computes without u = W2 h + b2."""
    gen = torch.Generator().manual_seed(0)
    rows, c, k = 37, 8, 32
    h, dy = torch.randn(rows, k, dtype=torch.float64, generator=gen), torch.randn(rows, c, dtype=torch.float64, generator=gen)
    s = torch.tensor([0.0, 2.0], dtype=torch.float64)[torch.arange(rows) % 2].view(rows, 1)
    w2 = torch.randn(c, k, dtype=torch.float64, generator=gen, requires_grad=True)
    b2 = torch.randn(c, dtype=torch.float64, generator=gen, requires_grad=True)
    g = torch.rand(c, dtype=torch.float64, generator=gen).requires_grad_(True)
    y = s * (g * F.linear(h, w2, b2))
    dw2, db2, dg = torch.autograd.grad(y, (w2, b2, g), dy)
    dzs = s * dy
    dw2p, db2p = dzs.t() @ h, dzs.sum(0)
    assert torch.allclose(dg, (dw2p * w2).sum(1) + db2p * b2, rtol=1e-12, atol=1e-12)
    assert torch.allclose(dw2, g.view(c, 1) * dw2p, rtol=1e-12, atol=1e-12)
    assert torch.allclose(db2, g * db2p, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("hw", [(6, 8), (13, 19)])
def test_the_down_sampler_as_space_to_depth_rows(hw):
    """The 2x2 stride-2 conv's gradients from Linear gradients over the patch rows (kinds 8, 1, 0, 9), odd sizes included."""
    gen = torch.Generator().manual_seed(1)
    b, c, co, (h, w) = 2, 8, 16, hw
    ho, wo = h // 2, w // 2
    x = torch.randn(b, c, h, w, dtype=torch.float64, generator=gen, requires_grad=True)
    wt = torch.randn(co, c, 2, 2, dtype=torch.float64, generator=gen, requires_grad=True)
    dz = torch.randn(b, co, ho, wo, dtype=torch.float64, generator=gen)
    dx, dw = torch.autograd.grad(F.conv2d(x, wt, None, stride=2), (x, wt), dz)
    rows = x.detach().permute(0, 2, 3, 1)[:, :2 * ho, :2 * wo]
    patches = rows.reshape(b, ho, 2, wo, 2, c).permute(0, 1, 3, 2, 4, 5).reshape(b * ho * wo, 4 * c)
    w2d = wt.detach().permute(0, 2, 3, 1).reshape(co, 4 * c)
    dzr = dz.permute(0, 2, 3, 1).reshape(-1, co)
    dwp = dzr.t() @ patches
    assert torch.allclose(dwp.view(co, 2, 2, c).permute(0, 3, 1, 2), dw, rtol=1e-12, atol=1e-12)
    dpatch = (dzr @ w2d).view(b, ho, wo, 2, 2, c)
    pix = torch.zeros(b, h, w, c, dtype=torch.float64)
    pix[:, :2 * ho, :2 * wo] = dpatch.permute(0, 1, 3, 2, 4, 5).reshape(b, 2 * ho, 2 * wo, c)
    assert torch.allclose(pix.permute(0, 3, 1, 2), dx, rtol=1e-12, atol=1e-12)
    assert (dx[:, :, 2 * ho:] == 0).all() and (dx[:, :, :, 2 * wo:] == 0).all()


def test_the_bound_structs_follow_the_header():
    text = open(_hip.HEADER_PATH).read()
    for name, cls in (("sdetr_convnext_bwd_op", _hip.ConvnextBwdOpStruct), ("sdetr_convnext_op", _hip.ConvnextOpStruct)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        fields = [f.strip() for f in body.split(";") if f.strip()]
        assert [f[0] for f in cls._fields_] == [re.search(r"(\w+)$", f).group(1) for f in fields]
        size = 0
        for f in fields:   # the C layout: natural alignment, pointers 8 bytes, int / float 4
            n = 8 if "*" in f else 4
            size = -(-size // n) * n + n
        assert ctypes.sizeof(cls) == -(-size // 8) * 8, name
    assert [f[0] for f in _hip.ConvnextOpStruct._fields_][-2:] == ["aux", "row_scale"]
