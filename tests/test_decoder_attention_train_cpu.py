"""CPU: the masked training attention (csrc/attention_train_masked.hip) refuses bad arguments on the host, reports a tile
that fits the LDS, `applies_masked` refuses what the kernel does not serve, and the decoder's training-form switch."""
import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from salience_detr_amd.csrc import build
    build.build()
    from salience_detr_amd import _hip
    return _hip.lib()


def _forward_args(N=300, B=2, H=8, hd=32, rs=512, q=8, mask=None, mask_rs=0):
    return (None, q, 300 * 512, rs, 8, 300 * 512, 512, 8, 300 * 256, 256, B, H, N, hd, 0.17, mask, mask_rs, 8, 8)


def test_masked_attention_forward_rejects_bad_arguments(lib):
    from salience_detr_amd import _hip
    f = lib.sdetr_attention_train_masked_forward_f32
    assert f(*_forward_args(hd=16)) == _hip.EINVAL and b"32-channel" in lib.sdetr_last_error()
    assert f(*_forward_args(rs=130)) == _hip.EINVAL and b"strides" in lib.sdetr_last_error()
    assert f(*_forward_args(rs=128)) == _hip.EINVAL and b"strides" in lib.sdetr_last_error()      # does not cover 8 heads
    assert f(*_forward_args(mask=8, mask_rs=299)) == _hip.EINVAL and b"mask" in lib.sdetr_last_error()
    assert f(*_forward_args(N=-1)) == _hip.EINVAL and b"bad sizes" in lib.sdetr_last_error()
    assert f(*_forward_args(B=-1)) == _hip.EINVAL and b"bad sizes" in lib.sdetr_last_error()
    assert f(*_forward_args(H=0)) == _hip.EINVAL and b"bad sizes" in lib.sdetr_last_error()
    assert f(*_forward_args(q=None)) == _hip.EINVAL and b"null" in lib.sdetr_last_error()
    # nothing to do: no launch, whatever the pointers are; no row limit in the argument check
    assert f(*_forward_args(N=0)) == 0
    assert f(*_forward_args(B=0)) == 0
    assert f(*_forward_args(N=0, mask=8, mask_rs=0)) == 0
    assert f(*_forward_args(N=100000, B=0)) == 0


def test_masked_attention_backward_rejects_bad_arguments(lib):
    from salience_detr_amd import _hip
    g = lib.sdetr_attention_train_masked_backward_f32

    def args(N=300, hd=32, rs=512, mask=None, mask_rs=0, gk=8):
        return (None, 8, 300 * 512, rs, 8, 300 * 512, 512, 8, 300 * 256, 256, 2, 8, N, hd, 0.17, mask, mask_rs, 8, 8, 8, 8, gk, 8)
    assert g(*args(hd=16)) == _hip.EINVAL and b"32-channel" in lib.sdetr_last_error()
    assert g(*args(rs=130)) == _hip.EINVAL and b"strides" in lib.sdetr_last_error()
    assert g(*args(mask=8, mask_rs=10)) == _hip.EINVAL and b"mask" in lib.sdetr_last_error()
    assert g(*args(N=-5)) == _hip.EINVAL and b"bad sizes" in lib.sdetr_last_error()
    assert g(*args(gk=None)) == _hip.EINVAL and b"null" in lib.sdetr_last_error()
    assert g(*args(N=0)) == 0


def test_masked_attention_tile_fits_the_lds(lib):
    T = lib.sdetr_attention_train_masked_tile_rows()
    assert T > 0
    assert 2 * T * 36 * 4 <= 160 * 1024


def test_applies_masked_refuses_what_the_kernel_does_not_serve():
    from salience_detr_amd import attention_train as A
    qk, v = torch.zeros(1, 10, 512), torch.zeros(1, 10, 256)
    assert not A.applies_masked(qk, v, 8, None)                                             # CPU tensors
    assert not A.applies_masked(qk, v, 8, torch.zeros(10, 10, dtype=torch.bool))
    assert not A.applies_masked(qk, v, 8, torch.zeros(10, 10))                              # float (additive) mask
    assert not A.applies_masked(qk, v, 8, torch.zeros(8, 10, 10, dtype=torch.bool))         # [B * H, N, N]
    assert not A.applies_masked(qk.bfloat16(), v.bfloat16(), 8, None)
    # (what it accepts, and the same refusals on the device, are in the GPU suite)


def _decoder(num_layers=3):
    from salience_detr_amd.salience_decoder import SalienceTransformerDecoder, SalienceTransformerDecoderLayer
    layer = SalienceTransformerDecoderLayer(embed_dim=64, d_ffn=32, n_heads=2, dropout=0.0, n_levels=1, n_points=1)
    return SalienceTransformerDecoder(layer, num_layers, num_classes=3)


def test_decoder_train_form_switch():
    dec = _decoder()
    assert dec.train_form == "torch" and all(l.train_form == "torch" for l in dec.layers)
    assert dec.set_train_form("hip") is dec
    assert dec.train_form == "hip" and len(dec.layers) == 3 and all(l.train_form == "hip" for l in dec.layers)
    for bad in ("HIP", "", None, "native"):
        with pytest.raises(ValueError):
            dec.set_train_form(bad)
    assert dec.train_form == "hip" and all(l.train_form == "hip" for l in dec.layers)    # a refused value changes nothing
    dec.set_train_form("torch")
    assert all(l.train_form == "torch" for l in dec.layers)
    assert not any("train_form" in k for k in dec.state_dict())                            # checkpoints are unaffected
