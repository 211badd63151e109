"""Shared builders of the deformable-conv tests (test_deform_conv_cpu.py, test_deform_conv_gpu.py): closed forms against
``F.conv2d``, the op-level cases of the HIP deformable product with their planted offsets, and the float64 yardstick.
Everything here runs on the CPU."""
import math

import torch
import torch.nn.functional as F

from salience_detr_amd.deform_conv import deform_conv2d

# Precision-0 bar of the HIP deformable product: the project's bar for op 0, 2e-6 x max|ref|.  The fallback the bilinear
# sum's extra roundings would justify is 4 x the distance of the float32 composite from the float64 composite on the same
# case.  Measured on the CPU over every OP_CASES entry (run this file): that distance is 2.6e-7 .. 5.0e-7 of max|ref| at
# W = 17 and 1.2e-6 .. 3.4e-6 at W = 69 (the composite adds the offset to the pixel coordinate in fp32; at x = 64 one ulp is
# 7.6e-6 px), so the fallback bar would be 4 x 3.41e-6 = 1.4e-5.  The kernel keeps the offset's own fraction (no rounding of
# that sum) and is held to the project's 2e-6; the fallback constant is recorded, not used.
F32_COMPOSITE_DISTANCE = 3.41e-6
PRECISION0_BAR = 2e-6
PRECISION1_BAR = 2e-2

SIGMA = 2.0     # px, of the random offsets
SEED = 11


def translate(x, dy, dx):
    """``out[.., y, x] = x[.., y + dy, x + dx]`` with zero fill (integer ``dy``, ``dx`` of any size)."""
    h, w = x.shape[-2:]
    out = torch.zeros_like(x)
    if abs(dy) >= h or abs(dx) >= w:
        return out
    ys, xs = slice(max(0, -dy), min(h, h - dy)), slice(max(0, -dx), min(w, w - dx))
    yt, xt = slice(max(0, dy), min(h, h + dy)), slice(max(0, dx), min(w, w + dx))
    out[..., ys, xs] = x[..., yt, xt]
    return out


def out_hw(n, k, s, p, d=1):
    return (n + 2 * p - d * (k - 1) - 1) // s + 1


# ---- the op-level cases of the HIP deformable product ---------------------------------------------------------------
# (ci, co, stride, W, residual + relu, nchw output).  H = 13.  W = 17, and W = 69: M = 2 * 13 * 69 = 7 * 256 + 2 rows, so
# the 256-pixel tile edge is crossed by the smallest amount an even row count allows.
OP_H = 13
OP_CASES = [
    (32, 8, 1, 17, False, True),
    (32, 8, 2, 17, True, False),
    (64, 64, 1, 17, True, True),
    (64, 64, 2, 17, False, False),
    (96, 72, 1, 17, True, False),
    (96, 72, 2, 17, True, True),
    (64, 64, 1, 69, True, True),
    (96, 72, 2, 69, False, True),
    (32, 8, 1, 69, False, False),
]


def border_fraction(offset, height, width, stride):
    """The share of (pixel, tap) samples of a 3x3 / padding-1 deformable conv with at least one bilinear corner outside the map."""
    b, _, ho, wo = offset.shape
    off = offset.double().reshape(b, 9, 2, ho, wo)
    ky, kx = torch.arange(3).repeat_interleave(3), torch.arange(3).repeat(3)
    y = (torch.arange(ho)[None, :] * stride - 1 + ky[:, None]).double()[None, :, :, None] + off[:, :, 0]
    x = (torch.arange(wo)[None, :] * stride - 1 + kx[:, None]).double()[None, :, None, :] + off[:, :, 1]
    y0, x0 = y.floor(), x.floor()
    outside = (y0 < 0) | (y0 + 1 > height - 1) | (x0 < 0) | (x0 + 1 > width - 1)
    return outside.double().mean().item()


def op_case(index):
    """Operands of OP_CASES[index] as fp32 CPU tensors: x NCHW, the conv weight, the offsets (given, not computed), the
    mask in (0, 1) and its logits (what the op reads), the residual or None."""
    ci, co, stride, width, with_res, _ = OP_CASES[index]
    height = OP_H
    g = torch.Generator().manual_seed(SEED + index)
    ho, wo = out_hw(height, 3, stride, 1), out_hw(width, 3, stride, 1)
    x = torch.randn(2, ci, height, width, generator=g)
    w = torch.randn(co, ci, 3, 3, generator=g) / math.sqrt(ci * 9)
    offset = SIGMA * torch.randn(2, 18, ho, wo, generator=g)
    # planted taps: far outside, past int32, exactly y = -1, exactly y = H - 1, exactly integer positions
    offset[0, 0, 0, 0], offset[0, 2, 0, 1] = height + 2.0, -(height + 2.0)
    offset[0, 5, 1, 0], offset[0, 7, 1, 1] = 3e9, -3e9
    offset[1, 4, 2, 2], offset[1, 5, 2, 2] = 3e9, 3e9
    for oy, target in ((2, -1.0), (3, height - 1.0)):            # tap 4 (ky = kx = 1): the row is oy * stride + dy
        offset[1, 8, oy, 3], offset[1, 9, oy, 3] = target - oy * stride, 0.0
    offset[1, :, 4, 4] = torch.tensor([2.0, -1.0] * 9)
    offset[0, :, 4, 2] = 0.0
    mask = torch.rand(2, 9, ho, wo, generator=g).clamp(1e-3, 1 - 1e-3)
    logits = torch.log(mask / (1 - mask))
    res = torch.randn(2, co, ho, wo, generator=g) if with_res else None
    share = border_fraction(offset, height, width, stride)
    assert 0.05 <= share <= 0.50, (index, share)
    return dict(x=x, w=w, offset=offset, logits=logits, res=res, stride=stride, share=share)


def op_reference(case, w64, b64, relu, dtype=torch.float64):
    """The composite on the operands the kernel sees: the folded weight ``w64`` / bias ``b64``, sigmoid of the fp32 logits."""
    mask = torch.sigmoid(case["logits"].to(dtype))
    ref = deform_conv2d(case["x"].to(dtype), case["offset"].to(dtype), w64.to(dtype), b64.to(dtype), stride=case["stride"],
                        padding=1, mask=mask)
    if case["res"] is not None:
        ref = ref + case["res"].to(dtype)
    return ref.clamp_min(0) if relu else ref


def dcn_state(model, seed, offset_px=1.0):
    """A state dict for a DCN backbone: deterministic values everywhere, the offset / mask convs random and scaled so that
    typical offsets are about ``offset_px`` pixels (the activations in front of them are O(1) after a ReLU)."""
    from salience_detr_amd import synthetic as syn
    sd = syn.det_state_dict(model.state_dict(), salt=seed)
    g = torch.Generator().manual_seed(seed)
    for k, v in sd.items():
        if ".conv2.conv_offset." in k or ".conv2.conv_mask." in k:
            fan = v[0].numel() if v.dim() == 4 else 1
            sd[k] = torch.randn(v.shape, generator=g) * (offset_px / math.sqrt(fan) if v.dim() == 4 else 0.3 * offset_px)
    return sd


if __name__ == "__main__":   # the measurement behind F32_COMPOSITE_DISTANCE
    for i in range(len(OP_CASES)):
        c = op_case(i)
        w64, b64 = c["w"].double(), torch.zeros(c["w"].shape[0], dtype=torch.float64)
        r64 = op_reference(c, w64, b64, False)
        r32 = op_reference(c, w64, b64, False, torch.float32)
        print(OP_CASES[i], f"border share {c['share']:.3f}",
              f"fp32 composite distance {(r32.double() - r64).abs().max().item() / r64.abs().max().item():.2e}")
