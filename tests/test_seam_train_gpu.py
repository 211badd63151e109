"""GPU: a backbone and the ChannelMapper trained together, in every pair of training forms (tests/seam_train_cases.py).

The per-module training tests hold each autograd node to float64 on synthetic contiguous inputs and cotangents; this file
holds the seam where the two nodes meet: the mapper's egest hands the backbone node its cotangent (the last map's is the
sum of two backward-data results), the backbone's ingest reads what the other side produced, the mapper reads what a
torch-form backbone produced (the ConvNeXt composite's maps are channels-last in memory), and inside the detector both
get their maps and cotangents from the real consumers.

Reference and bar: the float64 CPU pair of the case helper; every gradient within ``max(4 * d, GRAD_FLOOR)`` of it in both
measures of ``seam_train_cases.distance`` (max|got - ref| over max|ref|, relative difference of the norms), ``d`` being the
``own`` distance ``d32`` (fp32) or ``dbf16`` (bf16) of the reference's own fp32 / bf16-autocast run for that tensor: the
bar, the factor and the floor of the per-module training tests.  Every test prints its worst value / bar; the figures of
the first MI355X run are in CHANGELOG.md.
"""
from functools import partial

import pytest
import torch

import seam_train_cases as S
from salience_detr_amd import graph_guard
from salience_detr_amd.channel_mapper import ChannelMapper

pytestmark = pytest.mark.gpu
GRAD_FLOOR = 5e-6   # as tests/test_frontend_train_gpu.py
DTYPES = [torch.float32, torch.bfloat16]
PAIRS = [("hip", "hip"), ("hip", "torch"), ("torch", "hip")]     # (backbone form, neck form)
FORM_CASES = [(name,) + pair for name in S.HIP_BACKBONES for pair in PAIRS] + [("focalnet", "torch", "hip")]


def _pair(name, backbone_form, neck_form, dtype):
    backbone = S.build_backbone(name).cuda().set_dtype(dtype).set_train_form(backbone_form)
    neck = S.build_neck(backbone).cuda().set_dtype(dtype).set_train_form(neck_form)
    return backbone, neck


_inputs = {}


def _canvas():
    if not _inputs:
        _inputs["canvas"], _inputs["cots"] = S.canvas().cuda(), [c.cuda() for c in S.cotangents()]
    return _inputs["canvas"]


def _cots():
    _canvas()
    return _inputs["cots"]


def _step(backbone, neck, seam=None, keep=None):
    """One forward + backward of the case's loss.  ``seam`` (a dict) receives the cotangent the neck hands every backbone
    map (a hook on the map itself would see, in the torch form, the next stage's share too), ``keep`` the maps and the outputs; nothing of the step's graph is returned otherwise (a live graph would carry
    its stream into a later capture)."""
    maps = [m.view_as(m) for m in backbone(_canvas()).values()]   # aliases only the neck reads, in the maps' own strides
    if seam is not None:
        for l, m in enumerate(maps):
            m.register_hook(partial(seam.__setitem__, f"seam.{l}"))
    outs = neck(maps)
    if keep is not None:
        keep["maps"], keep["outs"] = [m.detach() for m in maps], [o.detach() for o in outs]
    sum((o * c).sum() for o, c in zip(outs, _cots())).backward()


def _grads(backbone, neck):
    return {n: p.grad for n, p in S.trainable(backbone, neck)}


def _assert_frozen_untouched(backbone):
    frozen = [n for n, p in backbone.named_parameters() if not p.requires_grad]
    assert frozen and all(dict(backbone.named_parameters())[n].grad is None for n in frozen)


def _hold(what, got, ref, dtype):
    """Every tensor of ``got`` against ``ref["g64"]`` at the bar of the module docstring; returns the worst value / bar."""
    key = "d32" if dtype == torch.float32 else "dbf16"
    worst, where, failures = 0.0, None, []
    for n, g in got.items():
        assert g is not None and g.dtype == torch.float32 and torch.isfinite(g).all(), n
        assert tuple(g.shape) == tuple(ref["g64"][n].shape), n
        own, norm = S.distance(g, ref["g64"][n])
        bar = max(4 * ref[key][n], GRAD_FLOOR)
        if max(own, norm) / bar > worst:
            worst, where = max(own, norm) / bar, n
        failures.extend((n, measure, v, bar) for measure, v in (("own", own), ("norm", norm)) if not v <= bar)
    print(f"{what}: worst value / bar {worst:.2f} ({where})")
    for f in failures:
        print("  over the bar:", f)
    assert not failures, failures
    return worst


# ---- a. gradients of every form pair ---------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,backbone_form,neck_form", FORM_CASES)
def test_gradients_of_every_form_pair_within_the_reference_error(name, backbone_form, neck_form, dtype):
    backbone, neck = _pair(name, backbone_form, neck_form, dtype)
    seam = {}
    _step(backbone, neck, seam)
    torch.cuda.synchronize()
    ref = S.reference(name)
    grads = _grads(backbone, neck)
    assert list(grads) + sorted(seam) == list(ref["g64"])
    for (n, p), g in zip(S.trainable(backbone, neck), grads.values()):
        assert g is not None and g.dtype == torch.float32 and g.shape == p.shape, n
    _assert_frozen_untouched(backbone)
    what = f"{name} ({backbone_form}, {neck_form}) {dtype}"
    _hold(what + " parameters", grads, ref, dtype)
    _hold(what + " seam", seam, ref, dtype)


# ---- b. the seam itself ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", S.HIP_BACKBONES)
def test_the_backbone_node_receives_the_mapper_nodes_input_gradients(name, dtype):
    """(hip, hip): what reaches each backbone map is the float64 seam gradient within the bar, and bit for bit what the
    mapper alone returns for detached copies of the same maps under the same output cotangents."""
    backbone, neck = _pair(name, "hip", "hip", dtype)
    seam, keep = {}, {}
    _step(backbone, neck, seam, keep)
    assert sorted(seam) == S.seam_names()
    _hold(f"{name} (hip, hip) {dtype} seam", seam, S.reference(name), dtype)
    alone = [m.clone().requires_grad_(True) for m in keep["maps"]]
    outs = neck(alone)
    sum((o * c).sum() for o, c in zip(outs, _cots())).backward()
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(outs, keep["outs"]))
    for l, x in enumerate(alone):
        assert x.grad.shape == x.shape and torch.equal(x.grad, seam[f"seam.{l}"]), l


# ---- c. forward ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", S.HIP_BACKBONES)
def test_training_forward_of_the_pair_equals_the_inference_forward(name, dtype):
    backbone, neck = _pair(name, "hip", "hip", dtype)
    outs = neck(list(backbone(_canvas()).values()))
    with torch.no_grad():
        ref = neck.forward_hip(list(backbone.forward_hip(_canvas()).values()))
    torch.cuda.synchronize()
    assert [tuple(o.shape) for o in outs] == S.level_shapes()
    for a, b in zip(outs, ref):
        assert a.requires_grad and a.dtype == torch.float32 and torch.equal(a, b)


# ---- d. strided inputs to the mapper ---------------------------------------------------------------------------------

def _layouts(maps):
    """The same values as contiguous NCHW, as channels_last-strided tensors and as permuted views of NHWC tensors."""
    dense = [m.contiguous() for m in maps]
    out = {"contiguous": dense,
           "channels_last": [m.contiguous(memory_format=torch.channels_last) for m in dense],
           "nhwc_view": [m.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for m in dense]}
    assert all(m.is_contiguous() for m in out["contiguous"])
    assert all(not m.is_contiguous() for k in ("channels_last", "nhwc_view") for m in out[k])
    return out


@pytest.mark.parametrize("dtype", DTYPES)
def test_mapper_takes_strided_maps_and_computes_the_same_bits(dtype):
    """The ConvNeXt composite's own maps (channels-last in memory) in three layouts: outputs, parameter gradients and
    input gradients are those of the contiguous maps, bit for bit, in the inference and in the training form."""
    backbone = S.build_backbone("convnext").cuda()
    with torch.no_grad():
        produced = list(backbone.forward_torch(_canvas()).values())
    got = {}
    for layout, maps in _layouts(produced).items():
        neck = S.build_neck(backbone).cuda().set_dtype(dtype).set_train_form("hip")
        with torch.no_grad():
            inference = neck(maps)
        xs = [m.requires_grad_(True) for m in maps]
        outs = neck(xs)
        acts = neck.saved_activations()
        for l, x in enumerate(xs):
            stored = acts[f"input.{l}"]
            assert stored.is_contiguous() and stored.dtype == torch.float32 and torch.equal(stored, x), (layout, l)
            assert (stored.data_ptr() == x.data_ptr()) == (layout == "contiguous"), (layout, l)   # copied only where needed
        sum((o * c).sum() for o, c in zip(outs, _cots())).backward()
        torch.cuda.synchronize()
        for l, x in enumerate(xs):
            assert x.grad is not None and x.grad.shape == x.shape and x.grad.dtype == torch.float32, (layout, l)
        got[layout] = dict(inference=inference, outs=[o.detach() for o in outs], inputs=[x.grad for x in xs],
                           params=[p.grad for p in neck.parameters()])
    base = got.pop("contiguous")
    for layout, other in got.items():
        for key, tensors in base.items():
            assert len(tensors) == len(other[key])
            for l, (a, b) in enumerate(zip(tensors, other[key])):
                assert torch.equal(a, b), (layout, key, l)


# ---- e. stability of the pair ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", S.HIP_BACKBONES)
def test_pair_two_runs_bit_identical_accumulation_and_graph_replay(name, dtype):
    backbone, neck = _pair(name, "hip", "hip", dtype)

    def clear():
        backbone.zero_grad(set_to_none=True)
        neck.zero_grad(set_to_none=True)

    def zero():
        for g in _grads(backbone, neck).values():
            g.zero_()
    _step(backbone, neck)
    first = {n: g.clone() for n, g in _grads(backbone, neck).items()}
    _step(backbone, neck)                         # a second backward() accumulates
    torch.cuda.synchronize()
    for n, g in _grads(backbone, neck).items():
        assert torch.equal(g, first[n] + first[n]), n
    clear()
    _step(backbone, neck)
    for n, g in _grads(backbone, neck).items():
        assert torch.equal(g, first[n]), n        # two steps from cleared gradients, bit for bit
    graph = graph_guard.new_graph()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        _step(backbone, neck)                     # eager warm-up on the side stream
        torch.cuda.synchronize()
        zero()
        with torch.cuda.graph(graph, stream=stream):
            _step(backbone, neck)
    torch.cuda.current_stream().wait_stream(stream)
    print(name, dtype, "captured step:", graph_guard.assert_replay_safe(graph, "captured backbone + neck step"), "nodes")
    for replay in range(2):
        zero()
        graph.replay()
        torch.cuda.synchronize()
        for n, g in _grads(backbone, neck).items():
            assert torch.equal(g, first[n]), (replay, n)


# ---- f. a request that is not eligible -------------------------------------------------------------------------------

def test_focalnet_hip_request_raises_at_forward_with_its_reason():
    backbone = S.build_backbone("focalnet").cuda().set_train_form("hip")
    with pytest.raises(RuntimeError, match="no HIP backward"):
        backbone(_canvas())
    # (the neck in "hip" form over the FocalNet's torch form is a case of test a)


# ---- g. inside the detector ------------------------------------------------------------------------------------------

def _detector(name):
    """The detector of the ``test_detector_trains_*`` tests over the case's backbone."""
    import test_detector_train_gpu as T
    from salience_detr_amd import synthetic as syn
    from salience_detr_amd.detector import SalienceDETR
    from salience_detr_amd.position_encoding import PositionEmbeddingSine
    from salience_detr_amd.post_process import PostProcess
    from salience_detr_amd.salience_criterion import SalienceCriterion
    from salience_detr_amd.salience_transformer import build_salience_transformer
    from salience_detr_amd.set_criterion import HungarianMatcher, HybridSetCriterion

    tr = build_salience_transformer(embed_dim=256, num_heads=8, d_ffn=64, num_encoder_layers=2,
                                    num_decoder_layers=T.DEC_LAYERS, num_classes=T.C, topk_sa=6, max_num_embedding=20,
                                    two_stage_num_proposals=T.PROPOSALS)
    tr.static_proposals = True
    crit = HybridSetCriterion(T.C, HungarianMatcher(cost_class=2, cost_bbox=5, cost_giou=2), T.weight_dict())
    backbone = S.build_backbone(name)
    det = SalienceDETR(backbone, ChannelMapper(backbone.num_channels, 256, 4), PositionEmbeddingSine(128, 10000, True, offset=-0.5),
                       tr, PostProcess(5), criterion=crit, focus_criterion=SalienceCriterion(noise_scale=0.0),
                       num_classes=T.C, num_queries=T.PROPOSALS, denoising_nums=12)
    sd = syn.det_state_dict(det.state_dict(), salt=9)
    sd.update({"backbone." + k: v for k, v in backbone.state_dict().items()})
    det.load_state_dict(sd)
    return det.cuda().train(), T


def _own_relu_pattern(backbone, canvas):
    """The ReLU sign pattern of the ResNet's live "hip" training forward, as the float64 pair's ``forward``.  On the
    detector's batch one pre-activation of layer4.0 lies within rounding of zero: the HIP fp32 forward and the float64
    composite put it on different sides (1 of 17 masks' elements on the MI355X; the CPU fp32 composite happens to agree
    with float64, so ``d32`` does not show it), and the two then differentiate different functions: every gradient below
    that block moved by 1e-4 .. 2e-3 of its scale.  As tests/test_backbone_train_gpu.py does, the reference takes the HIP
    run's own pattern, and the pattern is first held to the float64 composite's (at most 16 elements differ), so that a
    wrong stored activation cannot pass against itself."""
    import backbone_train_cases as BT
    masks = [(t > 0).permute(0, 3, 1, 2).cpu() for _, t in backbone.saved_activations()]
    ref, record = S.build_backbone("resnet").double(), []
    with torch.no_grad():
        BT.walk(ref, canvas.cpu().double(), ref.num_stages, ref.return_indices, record=record)
    assert [tuple(m.shape) for m in masks] == [tuple(m.shape) for m in record]
    flips = sum(int((a != b).sum()) for a, b in zip(masks, record))
    print("resnet in the detector: mask elements that differ from the float64 composite's:", flips)
    assert flips <= 16
    return S.masked_resnet_forward(masks)


@pytest.mark.parametrize("name", S.HIP_BACKBONES)
def test_inside_the_detector_both_nodes_get_what_autograd_would_give_them(name, monkeypatch):
    """One training step of the detector, (hip, hip), fp32.  The recorded canvas and the cotangents that reached the neck's
    outputs are replayed through the float64 CPU pair; every backbone and neck gradient and the seam cotangents are held
    to the bar of test a.  Taking the cotangents as captured keeps the transformer's atomics and top-k ties out of the
    comparison.  The ResNet's float64 pair runs at the HIP forward's own ReLU pattern (``_own_relu_pattern``)."""
    det, T = _detector(name)
    det.backbone.set_train_form("hip")
    det.neck.set_train_form("hip")
    rec = {"seam": {}, "cots": {}}
    forward = det.neck.forward

    def recording_forward(inputs):
        maps = [m.view_as(m) for m in (inputs.values() if isinstance(inputs, dict) else inputs)]
        for l, m in enumerate(maps):
            m.register_hook(partial(rec["seam"].__setitem__, f"seam.{l}"))
        outs = forward(maps)
        for l, o in enumerate(outs):
            o.register_hook(partial(rec["cots"].__setitem__, l))
        return outs
    monkeypatch.setattr(det.neck, "forward", recording_forward)
    handle = det.backbone.register_forward_pre_hook(lambda module, args: rec.__setitem__("canvas", args[0].detach()))
    images, targets = T.batch()
    losses = det(images, targets, noise=T.noise_for(det, (3, 2)))
    handle.remove()
    forward = None
    if name == "resnet":
        forward = _own_relu_pattern(det.backbone, rec["canvas"])
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    assert sorted(rec["cots"]) == list(range(len(det.neck.convs))) and sorted(rec["seam"]) == S.seam_names()
    grads = _grads(det.backbone, det.neck)
    _assert_frozen_untouched(det.backbone)
    # the float64 CPU pair on the recorded canvas and the captured output cotangents
    backbone = S.build_backbone(name)
    neck = ChannelMapper(backbone.num_channels, 256, 4).train()
    neck.load_state_dict({k: v.cpu() for k, v in det.neck.state_dict().items()})
    ref = S.yardsticks(backbone, neck, rec["canvas"].cpu(), [rec["cots"][l].cpu() for l in range(len(det.neck.convs))], forward)
    assert list(grads) + S.seam_names() == list(ref["g64"])
    for n, g in ref["g64"].items():
        assert g.abs().max().item() > 0, n
    _hold(f"{name} in the detector, parameters", grads, ref, torch.float32)
    _hold(f"{name} in the detector, seam", rec["seam"], ref, torch.float32)
