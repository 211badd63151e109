"""The reference's training transform (``transforms/presets.py``: ``detr``, ``multiscale``, ``hflip``) from decoded images
to the detector's padded canvas: ``RandomHorizontalFlip`` -> ``RandomChoice(RandomShortestSize | RandomShortestSize ->
RandomSizeCrop -> RandomShortestSize)`` -> ``ConvertImageDtype`` -> ``Normalize`` -> ``SanitizeBoundingBox``, then the
batching (zero padding to a multiple of 32, the padding mask).  The image half is ONE launch per batch
(``csrc/train_transform.hip``, built on the routine ``EvalResize`` is pinned with); the draws and the boxes are host
arithmetic.

Scope of the parity.  The presets as shipped apply these steps to PIL images, before ``PILToTensor``, and PIL's resize is
a different, fixed-point filter.  What is pinned here is the reference's transform classes applied to TENSORS
(``F.interpolate(..., mode="bilinear", antialias=True)``, uint8 rounded after every resize): the path that exists on a
device, and the one ``EvalResize`` is pinned to as well.  The draws, the sizes and the boxes do not depend on that choice.

* ``shortest_size`` is ``RandomShortestSize``'s size rule (Python double arithmetic; NOT ``eval_resize_size``'s float32
  rule).
* ``sample_params`` consumes ``torch``'s and ``random``'s global generators with the reference's calls in the reference's
  order, so after ``torch.manual_seed(s); random.seed(s)`` it returns what the reference's ``Compose`` would draw.
* ``transform_targets`` is the boxes' half in the reference's fp32 arithmetic, bit for bit, with ``SanitizeBoundingBox``.
* ``TrainTransform`` (``.detr()``, ``.multiscale()``, ``.hflip()``) is the callable: images and targets in,
  ``TrainBatch(canvas, mask, image_sizes, targets)`` out, which ``SalienceDETR.forward_batch`` takes.

A CPU tensor raises: there is no fallback.
"""
import ctypes
import random
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor

from . import _hip
from .eval_resize import MAX_IMAGES, _check_images, _int_pairs

# transforms/presets.py
SCALES = tuple(range(480, 801, 32))
MAX_SIZE = 1333
CROP_SCALES = (400, 500, 600)
CROP_RANGE = (384, 600)
P_FLIP = 0.5


def shortest_size(h: int, w: int, min_size: int, max_size: Optional[int] = None) -> Tuple[int, int]:
    """``(new_height, new_width)`` of ``RandomShortestSize`` for the drawn ``min_size`` on an ``h x w`` image
    (transforms/v2/_geometry.py:1351-1362): the ratio and both products in Python floats (double), truncated."""
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"shortest_size: image size must be positive, got {h} x {w}")
    r = min_size / min(h, w)
    if max_size is not None:
        r = min(r, max_size / max(h, w))
    return int(h * r), int(w * r)


@dataclass(frozen=True)
class AugmentParams:
    """One image's augmentation: ``flip``; ``n_stages`` resizes (0, 1 or 2); with two, ``size1 = (h1, w1)`` after the first
    and ``crop = (top, left, height, width)`` inside it; ``size = (nh, nw)`` of the result.  ``flip_last``: the flip comes
    after the (one) resize, as in the ``multiscale`` preset, instead of first."""
    flip: bool
    n_stages: int
    size1: Optional[Tuple[int, int]]
    crop: Optional[Tuple[int, int, int, int]]
    size: Tuple[int, int]
    flip_last: bool = False

    def plan(self) -> List[int]:
        """The ten ints of this image in ``sdetr_backbone_train_batch_images``'s plan."""
        h1, w1 = self.size1 if self.n_stages == 2 else (0, 0)
        top, left, ch, cw = self.crop if self.n_stages == 2 else (0, 0, 0, 0)
        flip = (2 if self.flip_last else 1) if self.flip else 0
        return [flip, self.n_stages, h1, w1, top, left, ch, cw, self.size[0], self.size[1]]


def _draw_flip(p_flip: float) -> bool:
    return bool(torch.rand(1) < p_flip)          # taken even when the flip is not applied (_transform.py:155)


def _draw_scale(scales: Sequence[int]) -> int:
    return scales[int(torch.randint(len(scales), ()))]


def sample_params(h: int, w: int, *, scales: Optional[Sequence[int]] = SCALES, max_size: Optional[int] = MAX_SIZE,
                  crop_scales: Optional[Sequence[int]] = CROP_SCALES, crop_range: Optional[Tuple[int, int]] = CROP_RANGE,
                  p_flip: float = P_FLIP, branch: Union[bool, int] = True, flip_last: bool = False) -> AugmentParams:
    """Draw one image's augmentation from ``torch``'s and ``random``'s global generators, with the reference's calls in
    the reference's order:

    * the flip, ``torch.rand(1) < p_flip``;
    * the branch, ``torch.multinomial(tensor([.5, .5]), 1)`` (``branch=True``; ``branch=0`` / ``branch=1`` force the plain
      / the crop branch without that draw; there is no choice, and no draw, without ``crop_scales``);
    * per ``RandomShortestSize`` ``torch.randint(len(scales), ())``;
    * for the crop two ``random.randint`` (height, then width, each in ``[min, min(side, max)]``), then
      ``torch.randint(0, side - crop + 1, (1,))`` for the top, then for the left.

    ``scales=None``: no resize at all (the ``hflip`` preset).  ``flip_last``: the flip is drawn and applied after the
    resize (the ``multiscale`` preset's order)."""
    h, w = int(h), int(w)
    if scales is None:
        return AugmentParams(_draw_flip(p_flip), 0, None, None, (h, w))
    if flip_last:
        if crop_scales is not None:
            raise ValueError("sample_params: flip_last goes with a single resize (the multiscale preset)")
        size = shortest_size(h, w, _draw_scale(scales), max_size)
        return AugmentParams(_draw_flip(p_flip), 1, None, None, size, flip_last=True)
    flip = _draw_flip(p_flip)
    if crop_scales is None:
        crop_branch = False
    elif branch is True:
        crop_branch = int(torch.multinomial(torch.tensor([0.5, 0.5]), 1)) == 1
    else:
        crop_branch = int(branch) == 1
    if not crop_branch:
        return AugmentParams(flip, 1, None, None, shortest_size(h, w, _draw_scale(scales), max_size))
    h1, w1 = shortest_size(h, w, _draw_scale(crop_scales))
    lo, hi = crop_range
    ch = random.randint(lo, min(h1, hi))
    cw = random.randint(lo, min(w1, hi))
    top = int(torch.randint(0, h1 - ch + 1, (1,)))
    left = int(torch.randint(0, w1 - cw + 1, (1,)))
    size = shortest_size(ch, cw, _draw_scale(scales), max_size)
    return AugmentParams(flip, 2, (h1, w1), (top, left, ch, cw), size)


def _flip_boxes(boxes: Tensor, width: int) -> Tensor:
    x0, y0, x1, y1 = boxes.unbind(-1)
    return torch.stack(((x1 - width).neg(), y0, (x0 - width).neg(), y1), -1)


def _scale_boxes(boxes: Tensor, old: Tuple[int, int], new: Tuple[int, int]) -> Tensor:
    # the ratios are Python floats rounded to fp32 by the tensor that holds them (functional/_geometry.py:230-234)
    rw, rh = new[1] / old[1], new[0] / old[0]
    return boxes * torch.tensor([rw, rh, rw, rh], dtype=torch.float32, device=boxes.device)


def transform_targets(target: Dict[str, Tensor], params: AugmentParams, h: int, w: int,
                      sanitize: bool = True) -> Dict[str, Tensor]:
    """The target of an ``h x w`` image after ``params``: ``boxes`` ``[n, 4]`` (xyxy pixels, float32) through the flip
    (``-(x - W)``), every resize (times the fp32 ratios ``new / old``) and the crop (minus ``[left, top, left, top]``,
    clamped to the crop), in the reference's fp32 arithmetic bit for bit; with ``sanitize`` (``SanitizeBoundingBox``,
    _misc.py:382-388) ``boxes`` and ``labels`` keep the boxes at least 1 px wide and high with every coordinate inside
    ``[0, size]``.  Every other key is passed through untouched; ``target`` is not modified.  Host tensors cost no device
    sync (device tensors pay one for the mask, when sanitising)."""
    boxes = target["boxes"]
    if boxes.dim() != 2 or boxes.shape[-1] != 4 or boxes.dtype != torch.float32:
        raise RuntimeError(f"transform_targets: boxes must be float32 [n, 4], got {boxes.dtype} {tuple(boxes.shape)}")
    size = (int(h), int(w))
    if params.flip and not params.flip_last:
        boxes = _flip_boxes(boxes, size[1])
    if params.n_stages == 2:
        boxes = _scale_boxes(boxes, size, params.size1)
        top, left, ch, cw = params.crop
        boxes = boxes - torch.tensor([left, top, left, top], dtype=torch.float32, device=boxes.device)
        x0, y0, x1, y1 = boxes.unbind(-1)
        boxes = torch.stack((x0.clamp(0, cw), y0.clamp(0, ch), x1.clamp(0, cw), y1.clamp(0, ch)), -1)
        size = (ch, cw)
    if params.n_stages >= 1:
        boxes = _scale_boxes(boxes, size, params.size)
        size = tuple(params.size)
    if params.flip and params.flip_last:
        boxes = _flip_boxes(boxes, size[1])
    out = dict(target)
    if sanitize:
        nh, nw = size
        x0, y0, x1, y1 = boxes.unbind(-1)
        valid = (x1 - x0 >= 1) & (y1 - y0 >= 1) & (boxes >= 0).all(-1) & (x0 <= nw) & (x1 <= nw) & (y0 <= nh) & (y1 <= nh)
        boxes = boxes[valid]
        if "labels" in target:
            out["labels"] = target["labels"][valid]
    elif boxes is target["boxes"]:
        boxes = boxes.clone()
    out["boxes"] = boxes
    return out


class TrainBatch(NamedTuple):
    """What ``TrainTransform`` returns and ``SalienceDETR.forward_batch`` takes: ``canvas`` ``[B, 3, Hp, Wp]`` float32
    (normalised, 0 on padding), ``mask`` ``[B, Hp, Wp]`` bool (True on padding), ``image_sizes`` the ``(h, w)`` of every
    transformed image, ``targets`` the transformed target dicts (boxes in xyxy pixels of the transformed image)."""
    canvas: Tensor
    mask: Tensor
    image_sizes: List[Tuple[int, int]]
    targets: Optional[List[Dict[str, Tensor]]]


def _plan_arrays(sizes: Sequence[Tuple[int, int]], params: Sequence[AugmentParams]):
    plan = [v for p in params for v in p.plan()]
    return _int_pairs(sizes), (ctypes.c_int * len(plan))(*plan)


def plan_stats(sizes: Sequence[Tuple[int, int]], params: Sequence[AugmentParams]) -> Tuple[int, int]:
    """``(staged, recomputed)``: of the workgroups that own pixels of the two-resize images of this batch, how many stage
    their window of the intermediate image in LDS and how many recompute it tap by tap (host arithmetic, no launch)."""
    hw, plan = _plan_arrays(sizes, params)
    staged, recomputed = ctypes.c_int64(0), ctypes.c_int64(0)
    _hip.check(_hip.lib().sdetr_backbone_train_plan_stats(hw, plan, len(params), ctypes.byref(staged),
                                                          ctypes.byref(recomputed)), "plan_stats")
    return staged.value, recomputed.value


class TrainTransform:
    """The training transform as one callable (module docstring).  ``scales`` / ``max_size``: the ``RandomShortestSize``
    every branch ends with (``scales=None``: no resize); ``crop_scales`` / ``crop_range``: the crop branch's pre-resize
    sizes and ``RandomSizeCrop(min, max)`` (``None``: no ``RandomChoice``); ``p_flip``; ``flip_last``: resize, then flip
    (``multiscale``); ``sanitize``: the preset ends with ``SanitizeBoundingBox``.

    ``__call__(images, targets, params=None)``: ``images`` a list of ``[3, h, w]`` tensors on the device, all uint8 or all
    float32 in [0, 1]; ``targets`` one dict per image (``boxes`` xyxy pixels float32, ``labels``; host tensors) or None;
    ``params`` one ``AugmentParams`` per image, default: sampled per image in batch order.  ONE launch, no device sync."""

    def __init__(self, scales: Optional[Sequence[int]] = SCALES, max_size: Optional[int] = MAX_SIZE,
                 crop_scales: Optional[Sequence[int]] = CROP_SCALES, crop_range: Optional[Tuple[int, int]] = CROP_RANGE,
                 p_flip: float = P_FLIP, flip_last: bool = False, sanitize: bool = True, size_divisible: int = 32):
        if (crop_scales is None) != (crop_range is None):
            raise ValueError("TrainTransform: crop_scales and crop_range go together")
        if not 0.0 <= p_flip <= 1.0:
            raise ValueError(f"TrainTransform: p_flip must be in [0, 1], got {p_flip}")
        self.scales = None if scales is None else tuple(int(s) for s in scales)
        self.max_size = max_size
        self.crop_scales = None if crop_scales is None else tuple(int(s) for s in crop_scales)
        self.crop_range = None if crop_range is None else (int(crop_range[0]), int(crop_range[1]))
        self.p_flip = float(p_flip)
        self.flip_last = bool(flip_last)
        self.sanitize = bool(sanitize)
        self.size_divisible = int(size_divisible)

    @classmethod
    def detr(cls) -> "TrainTransform":
        """``presets.detr``: flip, then one resize or resize -> crop -> resize; sanitised."""
        return cls()

    @classmethod
    def multiscale(cls) -> "TrainTransform":
        """``presets.multiscale``: one resize, then the flip; no ``SanitizeBoundingBox``."""
        return cls(crop_scales=None, crop_range=None, flip_last=True, sanitize=False)

    @classmethod
    def hflip(cls) -> "TrainTransform":
        """``presets.hflip``: the flip only; no ``SanitizeBoundingBox``."""
        return cls(scales=None, max_size=None, crop_scales=None, crop_range=None, sanitize=False)

    def sample(self, h: int, w: int, branch: Union[bool, int] = True) -> AugmentParams:
        return sample_params(h, w, scales=self.scales, max_size=self.max_size, crop_scales=self.crop_scales,
                             crop_range=self.crop_range, p_flip=self.p_flip, branch=branch, flip_last=self.flip_last)

    def __call__(self, images: Sequence[Tensor], targets: Optional[Sequence[Dict[str, Tensor]]] = None,
                 params: Optional[Sequence[AugmentParams]] = None) -> TrainBatch:
        if torch.is_tensor(images):
            images = list(images.unbind(0))
        dev, dt = _check_images("TrainTransform", images)
        sizes = [(int(im.shape[1]), int(im.shape[2])) for im in images]
        if targets is not None and len(targets) != len(images):
            raise RuntimeError("TrainTransform: one target dict per image expected")
        if params is None:
            params = [self.sample(h, w) for h, w in sizes]
        elif len(params) != len(images):
            raise ValueError("TrainTransform: one AugmentParams per image expected")
        out_sizes = [(int(p.size[0]), int(p.size[1])) for p in params]
        div = self.size_divisible
        hp = -(-max(nh for nh, _ in out_sizes) // div) * div
        wp = -(-max(nw for _, nw in out_sizes) // div) * div
        canvas = torch.empty(len(images), 3, hp, wp, device=dev, dtype=torch.float32)
        mask = torch.empty(len(images), hp, wp, device=dev, dtype=torch.bool)
        ptrs = (ctypes.c_void_p * len(images))(*[im.data_ptr() for im in images])
        hw, plan = _plan_arrays(sizes, params)
        _hip.launch("sdetr_backbone_train_batch_images", None, dev, ptrs, hw, plan, len(images),
                    1 if dt == torch.uint8 else 0, hp, wp, canvas.data_ptr(), mask.data_ptr(), what="TrainTransform")
        new_targets = None
        if targets is not None:
            new_targets = [transform_targets(t, p, h, w, sanitize=self.sanitize)
                           for t, p, (h, w) in zip(targets, params, sizes)]
        return TrainBatch(canvas, mask, out_sizes, new_targets)

    def __repr__(self) -> str:
        return (f"TrainTransform(scales={self.scales}, max_size={self.max_size}, crop_scales={self.crop_scales}, "
                f"crop_range={self.crop_range}, p_flip={self.p_flip}, flip_last={self.flip_last}, sanitize={self.sanitize})")
