"""Modulated deformable convolution (DCN v2): what the reference's ResNet builds its ``stage_with_dcn`` stages on
(reference ``models/bricks/deform_conv2d_pack.py`` over ``torchvision.ops.DeformConv2d``; this package has no
torchvision).

``deform_conv2d`` / ``DeformConv2d`` follow torchvision's signature and semantics, written from that contract:

  * ``offset`` ``[B, 2 * OG * kh * kw, Ho, Wo]`` (``OG`` offset groups): channel ``2 * (g * kh * kw + t)`` is dy of tap
    ``t = ky * kw + kx``, the next one dx; ``mask`` ``[B, OG * kh * kw, Ho, Wo]`` (or ``None``: ones);
  * tap ``t`` of output pixel ``(oy, ox)`` samples the input at ``(oy * stride - pad + ky * dil + dy, ox * stride - pad +
    kx * dil + dx)``, bilinear; the sample is zero when ``y <= -1``, ``y >= H``, ``x <= -1`` or ``x >= W``, otherwise
    every corner outside the map contributes zero;
  * the sample times the mask enters the ordinary grouped product with ``weight`` ``[out, in / groups, kh, kw]``.

``deform_conv2d`` here is the differentiable plain-torch composite (index arithmetic + ``gather``): any dtype (float64
included), CPU or device, any kernel size, stride, padding, dilation, groups and offset groups.  It is what
``ResNetBackbone.forward_torch`` and autograd go through, and the CPU-side yardstick of the HIP form.  The HIP form of a
DCN ``conv2`` is two ops of the backbone's forward plan (``backbone.py`` ``build_plan``, ``csrc/backbone_conv_core.h``
``ALoadDeform``): the offset and mask convs as one exact conv, then the deformable product.

``DeformConv2dPack`` has the reference's constructor, submodule names (``conv_offset``, ``conv_mask``,
``deform_conv2d``) and initialisation.
"""
import math
from typing import Optional, Tuple, Union

import torch
from torch import Tensor, nn


def _pair(v) -> Tuple[int, int]:
    return (int(v[0]), int(v[1])) if isinstance(v, (tuple, list)) else (int(v), int(v))


def deform_conv2d(input: Tensor, offset: Tensor, weight: Tensor, bias: Optional[Tensor] = None,
                  stride: Union[int, Tuple[int, int]] = 1, padding: Union[int, Tuple[int, int]] = 0,
                  dilation: Union[int, Tuple[int, int]] = 1, mask: Optional[Tensor] = None) -> Tensor:
    """See the module docstring.  ``input`` ``[B, C, H, W]`` -> ``[B, out, Ho, Wo]``."""
    (sh, sw), (ph, pw), (dh, dw) = _pair(stride), _pair(padding), _pair(dilation)
    batch, channels, height, width = input.shape
    out_channels, group_channels, kh, kw = weight.shape
    taps = kh * kw
    if channels % group_channels or out_channels % (channels // group_channels):
        raise RuntimeError(f"deform_conv2d: weight {tuple(weight.shape)} does not group {channels} input channels")
    groups = channels // group_channels
    ho = (height + 2 * ph - dh * (kh - 1) - 1) // sh + 1
    wo = (width + 2 * pw - dw * (kw - 1) - 1) // sw + 1
    if offset.dim() != 4 or offset.shape[0] != batch or tuple(offset.shape[2:]) != (ho, wo) or offset.shape[1] % (2 * taps) \
            or offset.shape[1] == 0:
        raise RuntimeError(f"deform_conv2d: offset {tuple(offset.shape)} is not [B, 2 * offset_groups * {taps}, {ho}, {wo}]")
    og = offset.shape[1] // (2 * taps)
    if channels % og:
        raise RuntimeError(f"deform_conv2d: {og} offset groups do not divide {channels} input channels")
    if mask is not None and tuple(mask.shape) != (batch, og * taps, ho, wo):
        raise RuntimeError(f"deform_conv2d: mask {tuple(mask.shape)} is not [{batch}, {og * taps}, {ho}, {wo}]")

    dt, dev = input.dtype, input.device
    ky = torch.arange(kh, device=dev).repeat_interleave(kw)
    kx = torch.arange(kw, device=dev).repeat(kh)
    base_y = (torch.arange(ho, device=dev)[None, :] * sh - ph + ky[:, None] * dh).to(dt)     # [taps, Ho]
    base_x = (torch.arange(wo, device=dev)[None, :] * sw - pw + kx[:, None] * dw).to(dt)     # [taps, Wo]
    off = offset.to(dt).reshape(batch, og, taps, 2, ho, wo)
    # clamped to [-1, H] x [-1, W] before the floor: a sample there is zero anyway, and no offset overflows the index
    y = (base_y[None, None, :, :, None] + off[:, :, :, 0]).clamp(-1, height)
    x = (base_x[None, None, :, None, :] + off[:, :, :, 1]).clamp(-1, width)
    inside = (y > -1) & (y < height) & (x > -1) & (x < width)
    y0f, x0f = y.detach().floor(), x.detach().floor()
    ly, lx = y - y0f, x - x0f
    y0, x0 = y0f.long(), x0f.long()
    rows = input.reshape(batch, og, channels // og, height * width)
    sampled = None
    for yi, wy in ((y0, 1 - ly), (y0 + 1, ly)):
        for xi, wx in ((x0, 1 - lx), (x0 + 1, lx)):
            valid = inside & (yi >= 0) & (yi <= height - 1) & (xi >= 0) & (xi <= width - 1)
            w = torch.where(valid, wy * wx, torch.zeros((), dtype=dt, device=dev))
            idx = (yi.clamp(0, height - 1) * width + xi.clamp(0, width - 1)).reshape(batch, og, 1, -1)
            vals = rows.gather(3, idx.expand(-1, -1, channels // og, -1)).reshape(batch, og, channels // og, taps, ho, wo)
            term = vals * w[:, :, None]
            sampled = term if sampled is None else sampled + term
    if mask is not None:
        sampled = sampled * mask.to(dt).reshape(batch, og, 1, taps, ho, wo)
    cols = sampled.reshape(batch, groups, group_channels, taps, ho * wo)
    wg = weight.to(dt).reshape(groups, out_channels // groups, group_channels, taps)
    out = torch.einsum("bgckp,gock->bgop", cols, wg).reshape(batch, out_channels, ho, wo)
    if bias is not None:
        out = out + bias.to(dt).reshape(1, -1, 1, 1)
    return out


class DeformConv2d(nn.Module):
    """torchvision's ``DeformConv2d``: the weight (and optional bias) of ``deform_conv2d``; ``forward(input, offset,
    mask=None)``."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size, stride=1, padding=0, dilation=1, groups: int = 1,
                 bias: bool = True):
        super().__init__()
        if in_channels % groups != 0:
            raise ValueError("in_channels must be divisible by groups")
        if out_channels % groups != 0:
            raise ValueError("out_channels must be divisible by groups")
        self.in_channels, self.out_channels, self.groups = in_channels, out_channels, groups
        self.kernel_size, self.stride, self.padding, self.dilation = _pair(kernel_size), _pair(stride), _pair(padding), \
            _pair(dilation)
        self.weight = nn.Parameter(torch.empty(out_channels, in_channels // groups, *self.kernel_size))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self) -> None:
        nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
        if self.bias is not None:
            fan_in = self.weight.shape[1] * self.kernel_size[0] * self.kernel_size[1]
            bound = 1 / math.sqrt(fan_in)
            nn.init.uniform_(self.bias, -bound, bound)

    def forward(self, input: Tensor, offset: Tensor, mask: Optional[Tensor] = None) -> Tensor:
        return deform_conv2d(input, offset, self.weight, self.bias, stride=self.stride, padding=self.padding,
                             dilation=self.dilation, mask=mask)

    def __repr__(self) -> str:
        return (f"{self.__class__.__name__}({self.in_channels}, {self.out_channels}, kernel_size={self.kernel_size}, "
                f"stride={self.stride}, padding={self.padding}, dilation={self.dilation}, groups={self.groups}, "
                f"bias={self.bias is not None})")


class DeformConv2dPack(nn.Module):
    """A deformable convolution used as a normal one (reference ``models/bricks/deform_conv2d_pack.py``): ``conv_offset``
    and ``conv_mask`` (sigmoid) compute the offsets and the modulation from the input itself."""

    def __init__(self, in_channels: int, out_channels: int, kernel_size, stride: int = 1, padding: int = 0,
                 dilation: int = 1, groups: int = 1, bias: bool = True):
        super().__init__()
        kernel_size = _pair(kernel_size)
        self.in_channels, self.kernel_size, self.groups = in_channels, kernel_size, groups
        taps = kernel_size[0] * kernel_size[1]
        self.conv_offset = nn.Conv2d(in_channels, groups * 2 * taps, kernel_size=kernel_size, stride=stride, padding=padding,
                                     dilation=dilation, groups=groups, bias=True)
        self.conv_mask = nn.Conv2d(in_channels, groups * taps, kernel_size=kernel_size, stride=stride, padding=padding,
                                   dilation=dilation, groups=groups, bias=True)
        self.deform_conv2d = DeformConv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding,
                                          dilation=dilation, groups=groups, bias=bias)
        self.init_weights()

    def init_weights(self) -> None:
        for conv in (self.conv_offset, self.conv_mask):
            nn.init.zeros_(conv.weight)
            nn.init.zeros_(conv.bias)
        bound = 1.0 / math.sqrt(self.in_channels * self.kernel_size[0] * self.kernel_size[1])
        nn.init.uniform_(self.deform_conv2d.weight, -bound, bound)
        if self.deform_conv2d.bias is not None:
            nn.init.zeros_(self.deform_conv2d.bias)

    def forward(self, x: Tensor) -> Tensor:
        return self.deform_conv2d(x, self.conv_offset(x), torch.sigmoid(self.conv_mask(x)))
