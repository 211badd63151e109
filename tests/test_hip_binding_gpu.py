"""GPU: the contract of `_hip.launch` -- the error text comes from the library that was called, and a launch goes to
the device (and that device's stream) of its operands, whichever device is current."""
import pytest
import torch

import backbone_cases as BC
import frontend_cases as FC
from salience_detr_amd import _hip
from salience_detr_amd.backbone import ResNetBackbone, batch_images
from salience_detr_amd.position_encoding import PositionEmbeddingSine, level_masks_and_positions

pytestmark = pytest.mark.gpu


def test_error_text_comes_from_the_library_called():
    """A call rejected by the fp16 library right after the bf16 library was selected: the message is the fp16 library's
    (the argument list of tests/test_abi_cpu.py: rejected on the host, nothing is launched)."""
    dev = torch.device("cuda", torch.cuda.current_device())
    _hip.lib()
    with pytest.raises(RuntimeError, match="bad dims"):
        _hip.launch("sdetr_msda_bordered_forward", torch.float16, dev, None, 2, None, None, 2, 0, None, None, 0, 1, -1, 8, 4,
                    None, 1, 0)


def _three_operators(dev):
    """batch_images on two small images, the sine positions of one level and ResNetBackbone.forward_hip (the smallest
    shapes of tests/test_backbone_gpu.py and tests/test_frontend_gpu.py) with everything on ``dev``; results on the CPU."""
    canvas, mask = batch_images([i.to(dev) for i in BC.images("r18")])
    kw, padding, shapes = FC.position_inputs("unnormalized")
    masks, pos = level_masks_and_positions(padding.to(dev), shapes[:1], PositionEmbeddingSine(**kw).to(dev))
    arch, ret, _ = BC.CASES["r18"]
    m = ResNetBackbone(arch, return_indices=ret)
    m.load_state_dict(BC.state(m.state_dict(), "r18"))
    with torch.no_grad():
        feats = m.eval().to(dev).forward_hip(canvas)
    torch.cuda.synchronize(dev)
    return [t.cpu() for t in (canvas, mask, masks[0], pos[0], *feats.values())]


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_operands_decide_the_device():
    """Device 0 stays current while tensors and modules live on device 1: the three operators that used to take the
    current device's stream give bit for bit what they give on device 0 (all three sum in a fixed order)."""
    torch.cuda.set_device(0)
    want = _three_operators(torch.device("cuda", 0))
    got = _three_operators(torch.device("cuda", 1))
    assert torch.cuda.current_device() == 0
    assert len(got) == len(want) == 7
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and torch.equal(a, b)
