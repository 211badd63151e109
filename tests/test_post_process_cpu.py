"""CPU: argument rejection of the detection post-processing, through the C ABI (before any launch) and the Python
wrapper (no CPU fallback)."""
import pytest
import torch

from salience_detr_amd import _hip


def call(k=300, dtype=_hip.F32, stride=900 * 91, batch=2, nq=900, c=91, sizes_dtype=_hip.I64, boxes_stride=3600):
    L = _hip.lib()
    code = L.sdetr_detection_postprocess(None, None, dtype, stride, None, boxes_stride, None, sizes_dtype, batch, nq, c,
                                         k, -1.0, -1.0, None, None, None, None)
    return code, L.sdetr_last_error().decode()


@pytest.mark.parametrize("k", [0, -1, 1025, 2000])
def test_bad_k_is_rejected(k):
    code, msg = call(k=k)
    assert code == _hip.EINVAL and "k =" in msg


def test_k_above_the_row_is_rejected():
    code, msg = call(k=71, nq=10, c=7, stride=70, boxes_stride=40)
    assert code == _hip.EINVAL and "k = 71" in msg


def test_bad_dtypes_are_rejected():
    code, msg = call(dtype=_hip.F16)                 # the bf16 library's 16-bit type is bf16
    assert code == _hip.EINVAL and "dtype" in msg
    code, msg = call(dtype=7)
    assert code == _hip.EINVAL and "dtype" in msg
    code, msg = call(sizes_dtype=_hip.BF16)
    assert code == _hip.EINVAL and "target sizes" in msg
    L = _hip.lib(torch.float16)                      # ... and the fp16 flavour's is fp16
    assert L.sdetr_detection_postprocess(None, None, _hip.BF16, 900 * 91, None, 3600, None, _hip.I64, 2, 900, 91, 300,
                                         -1.0, -1.0, None, None, None, None) == _hip.EINVAL


def test_small_strides_and_bad_sizes_are_rejected():
    code, msg = call(stride=900 * 91 - 1)
    assert code == _hip.EINVAL and "logits batch stride" in msg
    code, msg = call(boxes_stride=3599)
    assert code == _hip.EINVAL and "boxes batch stride" in msg
    for kw in (dict(batch=0), dict(nq=0), dict(c=0)):
        code, msg = call(**kw)
        assert code == _hip.EINVAL and "bad sizes" in msg
    code, msg = call(nq=1 << 20, c=17, stride=17 << 20)
    assert code == _hip.EINVAL and "2^24" in msg


def test_valid_arguments_get_as_far_as_the_pointer_check():
    code, msg = call()
    assert code == _hip.EINVAL and "null pointer" in msg


def test_wrapper_refuses_cpu_tensors_and_16bit_boxes():
    from salience_detr_amd.post_process import PostProcess, detections_padded
    logits, boxes, sizes = torch.zeros(2, 10, 5), torch.zeros(2, 10, 4), torch.tensor([[10, 10], [10, 10]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detections_padded(logits, boxes, sizes, 10)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        PostProcess(10)({"pred_logits": logits, "pred_boxes": boxes}, sizes)
    # the box dtype is checked before the device (the GPU file repeats this with device tensors)
    with pytest.raises(RuntimeError, match="pred_boxes must be float32"):
        detections_padded(logits, boxes.half(), sizes, 10)
