"""Shared by tests/test_msda_gpu.py, tests/test_msda_backward_lds_gpu.py and tests/test_zero_arena_gpu.py: the cases of the
MSDA backward parity checks against the plain-C oracle (oracle/msda_oracle.c), how a kernel is forced, and the bars."""
import contextlib

import numpy as np
import torch

from oracle import msda_c
from salience_detr_amd import ms_deform_attn as M
from salience_detr_amd import synthetic as syn

LEVELS_SMALL = [(20, 30), (10, 15), (5, 8), (3, 4)]
LEVELS_FULL = [(100, 168), (50, 84), (25, 42), (13, 21)]
LEVELS_TILED = [(40, 70), (33, 40), (5, 8)]     # two tiled levels (2800 and 1320 pixels) and one held whole

# (B, Nq, levels, M, D, P) of test_forward_backward_vs_c_oracle (seed 1, spread 6 px, the library's own dispatch)
ORACLE_CASES = [
    (2, 333, LEVELS_SMALL, 8, 32, 4),
    (1, 77, LEVELS_SMALL, 4, 16, 3),
    (3, 50, LEVELS_SMALL[:2], 2, 64, 5),   # L*P = 10
    (1, 40, LEVELS_SMALL, 2, 8, 9),        # L*P = 36 > one LDS chunk
    (2, 2272, LEVELS_FULL, 8, 32, 4),      # encoder layer 5 at the benchmark shape
    (2, 11363, LEVELS_FULL, 8, 32, 4),     # encoder layer 0 at the benchmark shape: the largest call of the step
]
# (B, Nq, levels, M, spread) of test_lds_backward_vs_c_oracle (seed 3, D = 32, P = 4, the LDS kernel forced)
LDS_CASES = [
    (2, 333, LEVELS_SMALL, 8, 4.0),      # every level held whole
    (1, 700, LEVELS_TILED, 3, 4.0),      # tiled levels, 3 heads
    (2, 1500, LEVELS_TILED, 8, 12.0),    # offsets beyond the halo: per-sample fallback to global atomics
    (2, 2272, LEVELS_FULL, 8, 6.0),      # encoder layer 5 at the benchmark shape
]
BAR = 2e-4   # of max(1, the oracle gradient's largest magnitude)


def smooth_mask(loc, shapes):
    # d(out)/d(loc) jumps where a sample sits on a pixel boundary; 1 ulp in loc*size-0.5 (fma contraction on the GPU) flips
    # floor() there.  Those samples are excluded.
    px = loc * torch.stack([shapes[:, 1], shapes[:, 0]], -1).float()[None, None, None, :, None, :] - 0.5
    return ((px - px.round()).abs() > 1e-3).all(-1, keepdim=True).expand_as(loc).numpy()


class Case:
    """Inputs of one backward call and the oracle's three gradients."""

    def __init__(self, value, shapes, lsi, loc, aw, go):
        self.value, self.shapes, self.lsi, self.loc, self.aw, self.go = value, shapes, lsi, loc, aw, go
        self.rgv, self.rgl, self.rga = msda_c.msda_backward(value.numpy(), shapes.numpy(), lsi.numpy(), loc.numpy(),
                                                            aw.numpy(), go.numpy())
        self.smooth = smooth_mask(loc, shapes)

    def on(self, device):
        return [t.to(device) for t in (self.value, self.shapes, self.lsi, self.loc, self.aw, self.go)]

    def assert_within_bar(self, gv, gl, ga):
        """The three gradients (numpy) within 2e-4 of the oracle's; returns the worst error / bar."""
        assert self.smooth.mean() > 0.99
        worst = 0.0
        for got, want, mask in ((gv, self.rgv, 1.0), (gl, self.rgl, self.smooth), (ga, self.rga, 1.0)):
            e, bar = np.abs((got - want) * mask).max(), BAR * max(1.0, np.abs(want).max())
            assert e < bar
            worst = max(worst, float(e / bar))
        return worst


def oracle_case(B, Nq, levels, M_, D, P, seed, spread, gout_name, loc_map=None):
    value, shapes, lsi, loc, aw = syn.make_msda_inputs(B, Nq, levels, M_, D, P, seed=seed, spread_px=spread)
    if loc_map is not None:
        loc = loc_map(loc).contiguous()
    return Case(value, shapes, lsi, loc, aw, syn.det_randn(gout_name, (B, Nq, M_ * D)))


@contextlib.contextmanager
def forced_backward_kernel(lds):
    """The LDS-accumulating (``lds``) or the direct global-atomic backward kernel, whatever the query count."""
    old = M.lds_backward, M.lds_backward_min_queries
    M.lds_backward, M.lds_backward_min_queries = lds, 1
    try:
        yield
    finally:
        M.lds_backward, M.lds_backward_min_queries = old
