"""MSDA backward with grad_value accumulated in LDS windows (msda_backward_tiled.hip) against the C oracle and the
direct global-atomic kernel.  Reference arithmetic: models/bricks/ops/cuda/ms_deform_im2col_cuda.cuh:76-148,290-392.
The test asserts which kernel ran (``last_backward_kernel``)."""
import numpy as np
import pytest
import torch

import msda_cases as MC

from oracle import msda_c
from salience_detr_amd import ms_deform_attn as M
from salience_detr_amd import synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda"
LEVELS_SMALL, LEVELS_FULL, LEVELS_TILED = MC.LEVELS_SMALL, MC.LEVELS_FULL, MC.LEVELS_TILED
_smooth_mask = MC.smooth_mask


def _run(lds, value, shapes, lsi, loc, aw, go):
    with MC.forced_backward_kernel(lds):    # the kernel under test, whatever the query count
        out = M.ms_deform_attn_backward(value, shapes, lsi, loc, aw, go, 64)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in out], M.last_backward_kernel()


@pytest.mark.parametrize("B,Nq,levels,M_,spread", MC.LDS_CASES)
def test_lds_backward_vs_c_oracle(B, Nq, levels, M_, spread):
    case = MC.oracle_case(B, Nq, levels, M_, 32, 4, seed=3, spread=spread, gout_name="gout_lds")
    (gv, gl, ga), which = _run(True, *case.on(DEV))
    assert which == M.KERNEL_BWD_LDS
    case.assert_within_bar(gv, gl, ga)


@pytest.mark.parametrize("Nq", [257, 11363])
def test_lds_backward_matches_direct_kernel_full_size(Nq):
    """Full benchmark size (B = 2, layer 0): the two kernels agree; the LDS one is the tighter of the two against a
    float64 accumulation of the same contributions (its window sums are exact integers)."""
    B, M_ = 2, 8
    value, shapes, lsi, loc, aw = syn.make_msda_inputs(B, Nq, LEVELS_FULL, M_, 32, 4, seed=5, spread_px=4.0)
    go = syn.det_randn("gout_full", (B, Nq, M_ * 32))
    dev = [t.to(DEV) for t in (value, shapes, lsi, loc, aw, go)]
    (gv1, gl1, ga1), k1 = _run(True, *dev)
    (gv0, gl0, ga0), k0 = _run(False, *dev)
    assert (k1, k0) == (M.KERNEL_BWD_LDS, M.KERNEL_BWD_DIRECT)
    scale = max(1.0, np.abs(gv0).max())
    assert np.abs(gv1 - gv0).max() < 1e-4 * scale
    smooth = _smooth_mask(loc, shapes)
    assert np.abs((gl1 - gl0) * smooth).max() < 1e-4 * max(1.0, np.abs(gl0).max())
    assert np.abs(ga1 - ga0).max() < 1e-4 * max(1.0, np.abs(ga0).max())
    # linearity in grad_output (a size-independent property): backward(2 g) = 2 backward(g) exactly for grad_loc /
    # grad_aw (powers of two), and to fixed-point resolution for grad_value
    dev2 = list(dev)
    dev2[5] = dev[5] * 2
    (gv2, gl2, ga2), _ = _run(True, *dev2)
    assert np.array_equal(gl2, 2 * gl1) and np.array_equal(ga2, 2 * ga1)
    assert np.abs(gv2 - 2 * gv1).max() < 1e-5 * scale


def test_lds_backward_extreme_gradients():
    """Gradient magnitudes far from 1 (loss scaling, vanishing gradients) and all-zero gradients: the per-window
    scale follows the data; out-of-range bounds take the global-atomic path."""
    B, Nq, M_ = 1, 400, 8
    value, shapes, lsi, loc, aw = syn.make_msda_inputs(B, Nq, LEVELS_SMALL, M_, 32, 4, seed=7, spread_px=3.0)
    go = syn.det_randn("gout_x", (B, Nq, M_ * 32))
    base = msda_c.msda_backward(value.numpy(), shapes.numpy(), lsi.numpy(), loc.numpy(), aw.numpy(), go.numpy())[0]
    for factor in (0.0, 2.0 ** -60, 2.0 ** 40, 2.0 ** 100):
        dev = [t.to(DEV) for t in (value, shapes, lsi, loc, aw, go * factor)]
        (gv, _, _), which = _run(True, *dev)
        assert which == M.KERNEL_BWD_LDS
        if factor == 0.0:
            assert not gv.any()
        else:
            assert np.abs(gv / factor - base).max() < 2e-4 * max(1.0, np.abs(base).max())


def test_lds_backward_heavy_tailed_gradients_keep_the_small_ones():
    """the window's fixed-point quantum follows the LARGEST row bound of a (level, image, head).  One
    outlier query (here 2^28 times the others) must not round everybody else's contributions away: rows far below the
    bound take the fp32 path.  Checked on pixels the outlier's samples do not touch, against the C oracle."""
    B, Nq, M_ = 1, 600, 8
    value, shapes, lsi, loc, aw = syn.make_msda_inputs(B, Nq, LEVELS_SMALL, M_, 32, 4, seed=11, spread_px=2.0)
    go = syn.det_randn("gout_tail", (B, Nq, M_ * 32))
    base = msda_c.msda_backward(value.numpy(), shapes.numpy(), lsi.numpy(), loc.numpy(), aw.numpy(), go.numpy())[0]
    go_tail = go.clone()
    go_tail[0, 17] *= 2.0 ** 28
    only = torch.zeros_like(go)
    only[0, 17] = go_tail[0, 17]
    spike = msda_c.msda_backward(value.numpy(), shapes.numpy(), lsi.numpy(), loc.numpy(), aw.numpy(), only.numpy())[0]
    untouched = spike == 0            # grad_value entries that receive nothing from the outlier row
    assert untouched.mean() > 0.5
    dev = [t.to(DEV) for t in (value, shapes, lsi, loc, aw, go_tail)]
    (gv, _, _), which = _run(True, *dev)
    assert which == M.KERNEL_BWD_LDS
    # without query 17 the oracle's sum on those entries is the sum of the ordinary rows (query 17 adds exact zeros)
    rest = go.clone()
    rest[0, 17] = 0
    want = msda_c.msda_backward(value.numpy(), shapes.numpy(), lsi.numpy(), loc.numpy(), aw.numpy(), rest.numpy())[0]
    err = np.abs(gv - want)[untouched].max()
    assert err < 2e-4 * max(1.0, np.abs(base).max()), err
    # and the spike itself arrives
    assert np.abs(gv - (want + spike))[~untouched].max() < 1e-5 * np.abs(spike).max()
