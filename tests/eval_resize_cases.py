"""Inputs of the ``EvalResize`` cases: shared by tests/golden/make_eval_resize_golden.py (which runs the imported
reference ``EvalResize`` on them) and the tests.  Images come from ``synthetic.det_rand`` (bit-identical on every machine)
or are closed-form gradients; nothing here is stored in the fixture."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from salience_detr_amd import synthetic as syn  # noqa: E402

MIN_SIZE, MAX_SIZE = 64, 96      # the resize of every image case
# name -> ((h, w), (nh, nw) the reference gives, kind)
IMAGES = {
    "stretch": ((37, 53), (64, 91), "noise"),
    "shrink": ((301, 500), (57, 96), "noise"),        # non-integer factor > 2, max_size binds
    "portrait": ((150, 97), (96, 62), "noise"),
    "identity": ((64, 80), (64, 80), "noise"),
    "extreme": ((20, 300), (6, 96), "noise"),         # one axis shrinks 3.3x to six rows
    "gradient": ((301, 500), (57, 96), "gradient"),   # smooth: the reference's fp32 sum lands within 1e-7
}
MIXED = ("stretch", "portrait", "shrink")             # the batch of the canvas test: three different sizes
MIXED_CANVAS = (96, 96)
DTYPES = ("f32", "u8")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
EXCLUDED_CAP = 0.02              # share of pixels of one image that may sit inside the rounding window


def image(name, dtype):
    """The case's image ``[3, h, w]``: float32 in [0, 1], or (``"u8"``) that image times 255, rounded."""
    (h, w), _, kind = IMAGES[name]
    if kind == "noise":
        img = syn.det_rand(f"eval_resize.{name}", (3, h, w))
    else:
        y = torch.arange(h, dtype=torch.float32).view(1, h, 1) / (h - 1)
        x = torch.arange(w, dtype=torch.float32).view(1, 1, w) / (w - 1)
        c = torch.tensor([0.2, 0.5, 0.8]).view(3, 1, 1)
        img = (0.6 * x + 0.4 * y) * c + (1 - c) * (x * y)
    if dtype == "u8":
        return (img * 255).round().to(torch.uint8)
    return img


def size_grid():
    """``(h, w, min_size, max_size)`` rows of the size fixture: (800, 1333) over a grid of sizes, every image case, and
    two more (min, max) pairs on a coarser grid."""
    rows = [(h, w, 800, 1333) for h in range(97, 4100, 89) for w in range(101, 4100, 97)]
    rows += [(h, w, 800, 1333) for h, w in ((480, 640), (640, 480), (3000, 4000), (4000, 3000), (800, 1333), (800, 1066),
                                            (1, 1), (1, 5000), (5000, 1), (799, 1334), (427, 640), (333, 500))]
    for mn, mx in ((480, 800), (MIN_SIZE, MAX_SIZE)):
        rows += [(h, w, mn, mx) for h in range(13, 1500, 61) for w in range(17, 1500, 67)]
    rows += [(h, w, MIN_SIZE, MAX_SIZE) for (h, w), _, _ in IMAGES.values()]
    return np.array(rows, dtype=np.int64)


def exact_size(h, w, mn, mx):
    """The size rule in exact rational arithmetic (what the float32 rule is compared with)."""
    from fractions import Fraction
    r = min(Fraction(mn, min(h, w)), Fraction(mx, max(h, w)))
    return int(h * r), int(w * r)


def round_half_even(x):
    return np.rint(x)


def excluded(pre_rounding, tau):
    """Pixels of a uint8 image whose float64 value is closer than ``tau`` to a ``.5`` rounding boundary."""
    frac = pre_rounding - np.floor(pre_rounding)
    return np.abs(frac - 0.5) < tau


def tau_u8(d_ref):
    return max(4.0 * float(d_ref), 1e-3)


def normalize64(img01):
    """``Normalize`` in float64 on ``[3, h, w]`` values in [0, 1] (numpy)."""
    mean, std = np.array(MEAN, dtype=np.float64).reshape(3, 1, 1), np.array(STD, dtype=np.float64).reshape(3, 1, 1)
    return (img01.astype(np.float64) - mean) / std


def canvas64(resized01, canvas_hw=MIXED_CANVAS):
    """The float64 canvas and the mask of the eval preprocessing from resized images in [0, 1] (numpy, float64):
    Normalize, then zero padding to the canvas; the mask is True on padding."""
    canvas = np.zeros((len(resized01), 3) + tuple(canvas_hw), dtype=np.float64)
    mask = np.ones((len(resized01),) + tuple(canvas_hw), dtype=bool)
    for b, im in enumerate(resized01):
        canvas[b, :, :im.shape[1], :im.shape[2]] = normalize64(im)
        mask[b, :im.shape[1], :im.shape[2]] = False
    return canvas, mask
