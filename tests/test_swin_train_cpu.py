"""CPU: the Swin backbone's training interface (``SwinBackbone.set_train_form``), the fixture's case list and the bound
structs."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import swin_train_cases as TC
from salience_detr_amd import _hip
from salience_detr_amd.backbone_base import HipBackbone
from salience_detr_amd.focalnet import FocalNetBackbone
from salience_detr_amd.swin import SwinBackbone


def _model(case="w7t", **kw):
    kw.setdefault("freeze_indices", TC.FREEZE)
    return SwinBackbone(None, return_indices=TC.RETURN, **TC.config(case), **kw)


def test_a_frozen_stem_is_served_and_the_reasons():
    m = _model()
    assert m.hip_train_reason() is None and m.hip_train_form()
    assert m.set_train_form("hip") is m and m.train_form == "hip"
    assert "no HIP backward" in _model(freeze_indices=()).hip_train_reason()
    assert "dropout" in _model(attention_dropout=0.1).hip_train_reason()
    assert "dropout" in _model(dropout=0.1).hip_train_reason()
    assert "float16" in _model().set_dtype(torch.float16).hip_train_reason()
    assert _model().set_dtype(torch.bfloat16).hip_train_form()
    x = torch.zeros(1, 3, 64, 64, requires_grad=True)
    assert "input requires" in m.hip_train_reason(x) and not m.hip_train_form(x)
    assert "architecture" in SwinBackbone(None, return_indices=(1,), freeze_indices=(0,), embed_dim=64, depths=(1, 1),
                                          num_heads=(2, 4), window_size=(8, 8)).hip_train_reason()
    # the extra rule is a hook of the base class; the shared method stays the base's
    assert SwinBackbone.hip_train_reason is HipBackbone.hip_train_reason
    assert HipBackbone._extra_train_reason(m) is None and FocalNetBackbone.train_reasons is None


def test_fixture_matches_the_case_list():
    gold = np.load(TC.GOLDEN)
    assert os.path.getsize(TC.GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(TC.GOLDEN), "convnext_train.npz"))
    for case in TC.CASES:
        names = [str(n) for n in gold[f"{case}.names"]]
        m = _model(case)
        assert names == [n for n, _ in m._trainable()]
        assert names == TC.trainable_names([n for n, _ in m.named_parameters()])
        shapes = dict((n, p.shape) for n, p in m.named_parameters())
        for n in names:
            g = gold[f"{case}.g:{n}"]
            assert g.shape == (min(shapes[n].numel(), TC.STORE),) and g.dtype == np.float64 and np.isfinite(g).all(), n
            norm, mx = float(gold[f"{case}.norm:{n}"]), float(gold[f"{case}.max:{n}"])
            assert np.isfinite([norm, mx]).all() and norm >= mx > 0 and np.abs(g).max() <= mx, n
            assert float(gold[f"{case}.d32:{n}"]) < 1e-4 and float(gold[f"{case}.dbf16:{n}"]) < 0.1, n
    assert {k.split(".")[0] for k in gold.files} == set(TC.CASES)


def test_the_bound_structs_follow_the_header():
    text = open(_hip.HEADER_PATH).read()
    for name, cls in (("sdetr_swin_bwd_op", _hip.SwinBwdOpStruct), ("sdetr_swin_op", _hip.SwinOpStruct)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, re.S).group(1)
        fields = [f.strip() for f in body.split(";") if f.strip()]
        assert [f[0] for f in cls._fields_] == [re.search(r"(\w+)$", f).group(1) for f in fields]
        size = 0
        for f in fields:   # the C layout: natural alignment, pointers 8 bytes, int / float 4
            n = 8 if "*" in f else 4
            size = -(-size // n) * n + n
        assert ctypes.sizeof(cls) == -(-size // 8) * 8, name
    assert [f[0] for f in _hip.SwinOpStruct._fields_][-2:] == ["aux", "row_scale"]
    assert [f[0] for f in _hip.SwinBwdOpStruct._fields_] == [
        "kind", "dz", "x", "weight", "scale", "gamma", "add", "bias", "table", "order", "offsets", "out", "dbias", "dgamma",
        "dbeta", "dtable", "batch", "channels", "height", "width", "out_channels", "window", "shift", "heads", "splits", "eps"]
    for fn in ("sdetr_swin_bwd_workspace_bytes", "sdetr_swin_bwd_op_run", "sdetr_swin_bwd_run"):
        assert fn in _hip.SIGNATURES
    assert "sdetr_swin_bwd_run" in _hip.LAUNCHES


def test_a_cpu_tensor_on_the_hip_form_raises():
    m = _model().train().set_train_form("hip")
    with pytest.raises(RuntimeError, match="HIP"):
        m(torch.zeros(1, 3, 64, 64))
