"""CPU: the one cache of parameter-derived kernel operands (salience_detr_amd/derived.py) -- what its key holds, that
names on one owner keep their own entries, and that ``invalidate_caches`` reaches modules, parameters and buffers."""
import pytest
import torch
from torch import nn

from salience_detr_amd.derived import derived, invalidate_caches


class _Builds:
    """A ``build`` that counts its calls and returns a fresh object each time."""

    def __init__(self):
        self.calls = 0

    def __call__(self):
        self.calls += 1
        return object()


def test_hit_when_nothing_changed():
    w, b = torch.ones(4, 3), torch.zeros(4)
    build = _Builds()
    first = derived(w, "op", (w, b), build, extra=(1, torch.float32))
    assert derived(w, "op", (w, b), build, extra=(1, torch.float32)) is first
    assert build.calls == 1


def _rebuilt(change):
    """Fill a cache on ``w`` keyed on (w, b, extra), apply ``change`` (-> new sources, new extra) and report whether the
    next call rebuilds."""
    w, b = torch.ones(4, 3), torch.zeros(4)
    build = _Builds()
    first = derived(w, "op", (w, b), build, extra=("a",))
    sources, extra = change(w, b)
    return derived(w, "op", sources, build, extra=extra) is not first and build.calls == 2


def _bump_version(w, b):
    with torch.no_grad():
        w.add_(0.0)
    return (w, b), ("a",)


@pytest.mark.parametrize("change", [
    pytest.param(_bump_version, id="version"),
    pytest.param(lambda w, b: ((w, b.clone()), ("a",)), id="storage"),
    pytest.param(lambda w, b: ((w, b.double()), ("a",)), id="dtype"),
    pytest.param(lambda w, b: ((w, b.view(2, 2)), ("a",)), id="shape"),
    pytest.param(lambda w, b: ((w, b), ("b",)), id="extra"),
    pytest.param(lambda w, b: ((w, None), ("a",)), id="tensor-to-none"),
])
def test_rebuild_on_each_key_component(change):
    assert _rebuilt(change)


def test_rebuild_from_none_to_tensor():
    w = torch.ones(4, 3)
    build = _Builds()
    first = derived(w, "op", (w, None), build)
    assert derived(w, "op", (w, None), build) is first
    assert derived(w, "op", (w, torch.zeros(4)), build) is not first and build.calls == 2


def test_rebuild_on_a_write_through_data_only_after_invalidate():
    lin = nn.Linear(3, 4)
    build = _Builds()
    first = derived(lin.weight, "op", (lin.weight,), build)
    lin.weight.data.add_(1.0)                                   # version unchanged: the key cannot see it
    assert derived(lin.weight, "op", (lin.weight,), build) is first
    invalidate_caches(lin)
    assert derived(lin.weight, "op", (lin.weight,), build) is not first and build.calls == 2


def test_two_names_on_one_owner_keep_their_own_entries():
    w = torch.ones(4, 3)
    a, b = _Builds(), _Builds()
    va = derived(w, "a", (w,), a)
    vb = derived(w, "b", (w, None), b, extra=7)
    for _ in range(3):
        assert derived(w, "a", (w,), a) is va
        assert derived(w, "b", (w, None), b, extra=7) is vb
    assert a.calls == b.calls == 1


def test_invalidate_caches_reaches_modules_parameters_and_buffers():
    bn = nn.BatchNorm1d(4)
    model = nn.Sequential(nn.Linear(3, 4), bn)
    owners = [model, model[0], bn, model[0].weight, model[0].bias, bn.weight, bn.running_mean, bn.num_batches_tracked]
    build = _Builds()
    for o in owners:
        derived(o, "op", (), build)
    assert all("_sdetr_derived" in o.__dict__ for o in owners)
    invalidate_caches(model)
    assert not any("_sdetr_derived" in o.__dict__ for o in owners)
    for o in owners:
        derived(o, "op", (), build)
    assert build.calls == 2 * len(owners)


def test_invalidate_caches_is_importable_from_ms_deform_attn():
    """INTEGRATION.md documents this import path."""
    from salience_detr_amd import ms_deform_attn
    assert ms_deform_attn.invalidate_caches is invalidate_caches
