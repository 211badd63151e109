"""``EvalResize`` (reference ``models/detectors/base_detector.py:20-53``): the resize the reference detector applies to
every eval image inside ``forward`` -- the smaller side to ``min_size`` unless that pushes the larger one past
``max_size`` -- with the antialiased bilinear filter of ``F.interpolate(..., antialias=True)``.

``eval_resize_size`` is the reference's size rule bit for bit (host arithmetic, no device work); ``EvalResize`` is the
reference class's constructor and ``forward(image) -> image`` (same dtype, resized) running ``csrc/eval_resize.hip``;
``resize_images`` is the same launch for a list of images.  ``backbone.batch_images(..., resize=(min_size, max_size))``
is the fused form (resize + convert + normalise + pad + mask in one launch, no resized image in memory).  Only bilinear
with antialiasing is a HIP path; every other setting raises, and so does a CPU tensor: there is no fallback.
"""
import ctypes
from enum import Enum
from typing import List, Optional, Sequence, Tuple, Union

import numpy as np
import torch
from torch import Tensor, nn

from . import _hip

MAX_IMAGES = 64   # images per launch (csrc/eval_resize.hip, csrc/backbone.hip)


class InterpolationMode(Enum):
    """The interpolation names of the reference's ``transforms.functional.InterpolationMode``."""
    NEAREST = "nearest"
    NEAREST_EXACT = "nearest-exact"
    BILINEAR = "bilinear"
    BICUBIC = "bicubic"
    BOX = "box"
    HAMMING = "hamming"
    LANCZOS = "lanczos"


_PIL_BILINEAR = 2   # PIL.Image.BILINEAR, which the reference accepts in place of the enum


def eval_resize_size(h: int, w: int, min_size: int, max_size: Optional[int] = None) -> Tuple[int, int]:
    """``(new_height, new_width)`` of ``EvalResize(min_size, max_size)`` on an ``h x w`` image, bit for bit.

    The reference computes it with 0-dim tensors: ``r = min_size / torch.min(h, w)`` is ``Tensor.__rtruediv__``, i.e.
    ``reciprocal() * min_size`` in float32 (NOT ``min_size / m``), ``r = torch.min(r, max_size / torch.max(h, w))`` the
    same way, and ``(orig * r).to(int64)`` a float32 product truncated.  Restated with numpy float32 scalars."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"eval_resize_size: image size must be positive, got {h} x {w}")
    one = np.float32(1)
    r = one / np.float32(min(h, w)) * np.float32(min_size)
    if max_size is not None:
        r = min(r, one / np.float32(max(h, w)) * np.float32(max_size))
    return int(np.float32(h) * r), int(np.float32(w) * r)


def _check_images(what: str, images: Sequence[Tensor]):
    """The checks every image-list entry point shares; returns ``(device, dtype)``."""
    if len(images) == 0:
        raise ValueError(f"{what}: no images")
    if len(images) > MAX_IMAGES:
        raise ValueError(f"{what}: at most {MAX_IMAGES} images per call, got {len(images)}")
    dev, dt = images[0].device, images[0].dtype
    if dt not in (torch.float32, torch.uint8):
        raise RuntimeError(f"{what}: images must be float32 or uint8, got {dt}")
    for im in images:
        if im.dim() != 3 or im.shape[0] != 3 or im.dtype != dt or im.device != dev:
            raise RuntimeError(f"{what}: every image must be [3, h, w] of one dtype on one device")
        _hip.require_device(what, image=im)
    return dev, dt


def _int_pairs(pairs):
    return (ctypes.c_int * (2 * len(pairs)))(*[int(v) for p in pairs for v in p])


def resize_images(images: Sequence[Tensor], sizes: Sequence[Tuple[int, int]]) -> List[Tensor]:
    """ONE launch: every ``images[i]`` ``[3, h_i, w_i]`` (float32, or uint8) resized to ``sizes[i] = (nh_i, nw_i)`` with
    the antialiased bilinear filter, same dtype (uint8: rounded half to even, as the reference's cast round trip)."""
    dev, dt = _check_images("resize_images", images)
    if len(sizes) != len(images):
        raise ValueError("resize_images: one (height, width) per image expected")
    sizes = [(int(nh), int(nw)) for nh, nw in sizes]
    if any(nh < 1 or nw < 1 for nh, nw in sizes):
        raise ValueError(f"resize_images: output sizes must be positive, got {sizes}")
    outs = [torch.empty(3, nh, nw, device=dev, dtype=dt) for nh, nw in sizes]
    ptrs = (ctypes.c_void_p * len(images))(*[im.data_ptr() for im in images])
    out_ptrs = (ctypes.c_void_p * len(images))(*[o.data_ptr() for o in outs])
    _hip.launch("sdetr_backbone_resize_images", None, dev, ptrs, _int_pairs([im.shape[1:] for im in images]),
                _int_pairs(sizes), len(images), 1 if dt == torch.uint8 else 0, out_ptrs, what="resize_images")
    return outs


class EvalResize(nn.Module):
    """The reference's ``EvalResize(min_size, max_size=None, interpolation=BILINEAR, antialias=True)``: ``forward(image)``
    returns ``image`` ``[3, h, w]`` resized to ``eval_resize_size(h, w, min_size, max_size)`` in its own dtype.  No
    parameters or buffers."""

    def __init__(self, min_size: int, max_size: Optional[int] = None,
                 interpolation: Union[InterpolationMode, int, str] = InterpolationMode.BILINEAR,
                 antialias: Optional[Union[str, bool]] = True):
        super().__init__()
        if not isinstance(min_size, int) or not (max_size is None or isinstance(max_size, int)):
            raise ValueError(f"EvalResize: min_size and max_size must be ints, got {min_size!r}, {max_size!r}")
        if min_size < 1 or (max_size is not None and max_size < 1):
            raise ValueError(f"EvalResize: sizes must be positive, got {min_size}, {max_size}")
        bilinear = interpolation in (InterpolationMode.BILINEAR, _PIL_BILINEAR, "bilinear") or \
            getattr(interpolation, "value", None) == "bilinear"
        if not bilinear or antialias is not True:
            raise ValueError("EvalResize: only interpolation=BILINEAR with antialias=True has a HIP kernel (got "
                             f"interpolation={interpolation!r}, antialias={antialias!r}); there is no fallback")
        self.min_size = min_size
        self.max_size = max_size
        self.interpolation = InterpolationMode.BILINEAR
        self.antialias = True

    def output_size(self, h: int, w: int) -> Tuple[int, int]:
        return eval_resize_size(h, w, self.min_size, self.max_size)

    def forward(self, image: Tensor) -> Tensor:
        if not torch.is_tensor(image):
            raise RuntimeError("EvalResize: only one image Tensor is supported")
        return resize_images([image], [self.output_size(image.shape[-2], image.shape[-1])])[0]

    def extra_repr(self) -> str:
        return f"min_size={self.min_size}, max_size={self.max_size}, interpolation=bilinear, antialias=True"
