"""CPU: the set criterion's argument rejection (Python layer and C ABI, before any launch), the host-side target staging
and the denoising assignment against the reference's meshgrid pattern (tests/golden/set_criterion_cases.npz)."""
import os

import numpy as np
import pytest
import torch

from salience_detr_amd import _hip
from salience_detr_amd import set_criterion as S

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(G, "set_criterion_cases.npz"))


def _targets(counts, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [{"boxes": torch.rand(n, 4, generator=g), "labels": torch.randint(0, 91, (n,), generator=g)} for n in counts]


def _outputs(B=2, Nq=10, C=91, aux=1):
    out = {"pred_logits": torch.randn(B, Nq, C), "pred_boxes": torch.rand(B, Nq, 4)}
    out["aux_outputs"] = [{"pred_logits": torch.randn(B, Nq, C), "pred_boxes": torch.rand(B, Nq, 4)} for _ in range(aux)]
    out["enc_outputs"] = {"pred_logits": torch.randn(B, Nq, C), "pred_boxes": torch.rand(B, Nq, 4)}
    return out


def test_mixed_match_is_not_implemented():
    with pytest.raises(NotImplementedError):
        S.HungarianMatcher(2, 5, 2, mixed_match=True)


def test_cpu_tensors_are_rejected():
    matcher = S.HungarianMatcher(2, 5, 2)
    crit = S.HybridSetCriterion(91, matcher, {})
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        crit(_outputs(), _targets((3, 4)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        matcher(torch.rand(10, 4), torch.randn(10, 91), torch.rand(3, 4), torch.tensor([1, 2, 3]))
    staged = S.stage_targets(_targets((3, 4)))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.match_outputs([torch.randn(2, 10, 91)], [torch.rand(2, 10, 4)], staged, 2, 5, 2, 0.25, 2.0)
    with pytest.raises(RuntimeError, match="HIP device"):
        S.dn_match(staged, 30, 5, 6)


def test_more_targets_than_queries_is_rejected():
    crit = S.HybridSetCriterion(91, S.HungarianMatcher(2, 5, 2), {})
    with pytest.raises(RuntimeError, match="T > Nq"):
        crit(_outputs(Nq=10), _targets((3, 11)))


def test_abi_rejects_capacity_above_queries():
    L = _hip.lib()
    table = (_hip.SetOutputStruct * 1)()
    table[0].logits, table[0].boxes = 256, 256
    table[0].logits_batch_stride, table[0].boxes_batch_stride = 10 * 91, 40
    dummy = 256   # never dereferenced: the call is rejected before any launch
    code = L.sdetr_set_match(None, table, 1, _hip.F32, 2, 10, 91, dummy, dummy, dummy, 11, 2.0, 5.0, 2.0, 0.25, 2.0, 0, 0,
                             dummy, 1 << 20, dummy, None, None)
    assert code == _hip.EINVAL and "exceeds 10 queries" in L.sdetr_last_error().decode()
    code = L.sdetr_set_match(None, table, 17, _hip.F32, 2, 10, 91, dummy, dummy, dummy, 5, 2.0, 5.0, 2.0, 0.25, 2.0, 0, 0,
                             dummy, 1 << 20, dummy, None, None)
    assert code == _hip.EINVAL
    code = L.sdetr_set_match(None, None, 1, _hip.F32, 2, 10, 1, None, None, dummy, 0, 0.0, 0.0, 0.0, 0.0, 0.0, 3, 4,
                             None, 0, dummy, None, None)
    assert code == _hip.EINVAL and "do not fit" in L.sdetr_last_error().decode()
    code = L.sdetr_set_loss(None, table, 1, _hip.F16, 2, 10, 91, dummy, dummy, dummy, dummy, None, 1.0, 0.25, 2.0,
                            dummy, 1 << 20, dummy)
    assert code == _hip.EINVAL and "dtype" in L.sdetr_last_error().decode()


def test_workspace_sizes():
    L = _hip.lib()
    assert L.sdetr_set_match_workspace_bytes(14, 100, 900) == 14 * 100 * 900 * 4
    assert L.sdetr_set_loss_workspace_bytes(7, 2, 900, 91) == 7 * 2 * ((900 * 91 + 2047) // 2048) * 3 * 8


def test_staging_packs_and_pads():
    tg = _targets((0, 3, 5), seed=4)
    st = S.stage_targets(tg, capacity=6)
    assert st.capacity == 6 and st.counts == [0, 3, 5] and st.batch == 3
    assert st.offsets.dtype == torch.int32 and st.offsets.tolist() == [0, 0, 3, 8]
    assert st.boxes.shape == (18, 4) and st.labels.shape == (18,) and st.labels.dtype == torch.int32
    assert torch.equal(st.boxes[0:3], tg[1]["boxes"]) and torch.equal(st.boxes[3:8], tg[2]["boxes"])
    assert torch.equal(st.labels[3:8], tg[2]["labels"].int())
    assert not st.boxes[8:].any() and not st.labels[8:].any()
    assert S.stage_targets(tg).capacity == 5
    assert S.stage_targets(_targets((0, 0))).capacity == 1
    with pytest.raises(RuntimeError, match="capacity"):
        S.stage_targets(tg, capacity=4)
    with pytest.raises(RuntimeError, match="do not match"):
        S.stage_targets([{"boxes": torch.rand(3, 4), "labels": torch.zeros(2, dtype=torch.int64)}])


def test_staged_copy_replaces_contents():
    a = S.stage_targets(_targets((2, 6), seed=1), capacity=8)
    b = S.stage_targets(_targets((7, 1), seed=2), capacity=8)
    c = a.copy_(b)
    assert c.counts == [7, 1] and c.boxes is a.boxes
    assert torch.equal(a.boxes, b.boxes) and torch.equal(a.offsets, b.offsets) and torch.equal(a.labels, b.labels)
    with pytest.raises(RuntimeError):
        a.copy_(S.stage_targets(_targets((2, 6)), capacity=9))


def test_dn_pattern_matches_reference(gold):
    groups, max_gt, nq, _ = gold["dn_params"].tolist()
    counts = gold["dn_counts"].tolist()
    pattern = S.dn_match_pattern(counts, nq, groups, max_gt)
    np.testing.assert_array_equal(pattern.numpy(), gold["dn_match"])
    # the reference's (src, tgt) pairs, image by image in meshgrid order
    src, tgt = [], []
    for b, n in enumerate(counts):
        q = torch.nonzero(pattern[b] >= 0).flatten()
        src.append(q)
        tgt.append(pattern[b][q].long())
    assert sorted(zip(torch.cat(src).tolist(), torch.cat(tgt).tolist())) == \
        sorted(zip(gold["dn_src"].tolist(), gold["dn_tgt"].tolist()))


def test_indices_round_trip(gold):
    match = gold["main_match"][0]      # [B, Nq] of the main output
    indices = []
    for row in match:
        src = np.nonzero(row >= 0)[0]
        indices.append((torch.from_numpy(src), torch.from_numpy(row[src].astype(np.int64))))
    back = S.indices_to_match(indices, match.shape[0], match.shape[1], "cpu")
    np.testing.assert_array_equal(back.numpy(), match)
