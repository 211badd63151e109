"""GPU: the parameter-derived operands of the bf16 whole transformer (salience_detr_amd/derived.py) follow new weights.

A model that ran a no-grad forward on state dict A, then received state dict B -- through ``p.data.copy_`` +
``invalidate_caches``, or through ``load_state_dict`` alone -- must compute bit for bit what a fresh model loaded with B
computes: no packed weight, fragment order, folded plan, host copy of the filter ratios, ... of A survives."""
import pytest
import torch

from salience_detr_amd import synthetic as syn
from salience_detr_amd.ms_deform_attn import invalidate_caches

pytestmark = pytest.mark.gpu

# every derived operand the no-grad bf16 forward of the transformer with the neck builds
REACHED = {
    "packed_linear", "packed_linear_x3", "layer1_constant", "ffn", "tail_ffn", "tail_ffn_cls", "token_linear",
    "token_linear_512", "fragment_order", "norm_f32", "class_head_fragments", "stacked_value_proj",
    "fused_query_projection", "fused_query_projection_head_major", "flat", "folded", "enc_output_cast", "ratios",
}


def _state_dicts():
    from salience_detr_amd.salience_transformer import build_salience_transformer
    ref = build_salience_transformer(with_neck=True).state_dict()
    a, b = syn.det_state_dict(ref), syn.det_state_dict(ref, salt=1)
    for k in b:                          # (det_state_dict passes the filter ratios through: give B its own)
        if k.endswith("level_filter_ratio"):
            b[k] = torch.tensor([0.3, 0.6, 1.0, 1.0])
        elif k.endswith("layer_filter_ratio"):
            b[k] = torch.tensor([1.0, 0.7, 0.6, 0.5, 0.4, 0.2])
    return a, b


def _model(sd):
    from salience_detr_amd.salience_transformer import build_salience_transformer
    tr = build_salience_transformer(with_neck=True)
    tr.load_state_dict(sd)
    return tr.eval().cuda().set_dtype(torch.bfloat16, torch.float16)


@pytest.fixture(scope="module")
def case():
    a, b = _state_dicts()
    _, masks = syn.make_masks([(800, 1333), (800, 1066)])
    shapes = [tuple(m.shape[-2:]) for m in masks]
    feats = [f.cuda() for f in syn.make_feats(2, shapes, 256, 0)]
    masks = [m.cuda() for m in masks]
    pos = [syn.sine_position_embedding(m, 128).cuda() for m in masks]

    def run(tr):
        with torch.no_grad():
            out = tr(feats, masks, pos)
        torch.cuda.synchronize()
        return [t.clone() for t in out if isinstance(t, torch.Tensor)]
    fresh_b = run(_model(b))
    return a, b, run, fresh_b


def _cached_names(model):
    names = set()
    for m in model.modules():
        for o in [m] + list(m.parameters(recurse=False)) + list(m.buffers(recurse=False)):
            names |= set(o.__dict__.get("_sdetr_derived", {}))
    return names


def _assert_equal(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), (i, (g.float() - w.float()).abs().max().item())


def test_forward_fills_every_converted_cache(case):
    a, _, run, _ = case
    tr = _model(a)
    run(tr)
    missing = REACHED - _cached_names(tr)
    assert not missing, missing
    invalidate_caches(tr)
    assert not _cached_names(tr)


def test_write_through_data_then_invalidate_equals_fresh_model(case):
    a, b, run, fresh_b = case
    tr = _model(a)
    out_a = run(tr)
    with torch.no_grad():
        for name, t in tr.state_dict(keep_vars=True).items():
            t.data.copy_(b[name])
    invalidate_caches(tr)
    out = run(tr)
    assert any(not torch.equal(x, y) for x, y in zip(out_a, fresh_b))     # A and B do differ
    _assert_equal(out, fresh_b)


def test_load_state_dict_equals_fresh_model(case):
    a, b, run, fresh_b = case
    tr = _model(a)
    run(tr)
    tr.load_state_dict(b)
    _assert_equal(run(tr), fresh_b)
