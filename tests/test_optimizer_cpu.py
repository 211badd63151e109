"""CPU: the optimizer step's host side (salience_detr_amd/optimizer.py) -- the reference's parameter groups, the
plain-torch statement of clip + AdamW against the reference's float64 trajectories, torch.optim.AdamW's state-dict format
in both directions, torch's schedulers, the refusals, the reducer path on two gloo ranks, and the new C-ABI symbols."""
import copy
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from torch import nn

import optimizer_cases as OC
from salience_detr_amd.optimizer import POLICIES, ClippedAdamW, build_tables, param_groups


@pytest.fixture(scope="module")
def fx():
    return OC.Fixture()


# ---- parameter groups -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("policy", sorted(POLICIES))
def test_param_groups_reproduce_the_reference_assignment(fx, policy):
    d = fx.d
    names = d[f"groups.{policy}.names"].tolist()
    index = d[f"groups.{policy}.index"].tolist()
    norm_names = ()
    if policy == "backbone_no_norm_weight_decay":      # the module policy asks for the class: the reference's norm leaves
        norm_names = [n for n, g in zip(names, index) if g in (1, 2)]
    model = OC.module_tree(d["model_names"].tolist(), norm_names)
    name_of = {id(p): n for n, p in model.named_parameters()}
    groups = param_groups(model, 1e-4, policy)
    got_names = [name_of[id(p)] for g in groups for p in g["params"]]
    got_index = [gi for gi, g in enumerate(groups) for _ in g["params"]]
    assert got_names == names and got_index == index
    opt = ClippedAdamW(groups, lr=1e-4, weight_decay=1e-4)
    lr = [g["lr"] for g in opt.param_groups for _ in g["params"]]
    wd = [g["weight_decay"] for g in opt.param_groups for _ in g["params"]]
    assert np.array_equal(np.array(lr), d[f"groups.{policy}.lr"])
    assert np.array_equal(np.array(wd, dtype=np.float64), d[f"groups.{policy}.weight_decay"])


def test_param_groups_on_the_projects_detector():
    import detector_train_cases as DT
    case = DT.Case("small")
    det = case.detector(case.stored_maps())
    det.backbone = nn.Sequential(nn.Conv2d(3, 4, 3, bias=True), nn.BatchNorm2d(4))     # parameters under "backbone."
    tr = det.transformer
    assert tr.encoder_class_head.weight is tr.encoder.enhance_mcsp.weight               # the shared head
    name_of = {}
    for n, p in det.named_parameters(remove_duplicate=False):
        name_of.setdefault(id(p), n)
    groups = param_groups(det, 1e-4)
    listed = [p for g in groups for p in g["params"]]
    assert len({id(p) for p in listed}) == len(listed) == len(list(det.parameters()))  # once each, the shared head once
    assert sum(p is tr.encoder_class_head.weight for p in listed) == 1
    assert [g.get("lr", 1e-4) for g in groups] == [1e-4, 1e-5, 1e-5, 1e-5, 1e-5, 1e-4]
    assert [g.get("weight_decay", None) for g in groups] == [None, None, 0, None, 0, 0]
    seen = set()
    for gi, g in enumerate(groups):
        for p in g["params"]:
            n = name_of[id(p)]
            backbone = "backbone" in n
            projection = "sampling_offsets" in n or "reference_points" in n
            no_decay = "norm" in n or "bias" in n
            want = (1 + no_decay) if backbone and not projection else (3 + no_decay) if projection and not backbone \
                else (5 if no_decay else 0)
            assert gi == want, (n, gi, want)
            seen.add(gi)
    assert seen == {0, 1, 2, 3, 4, 5}
    with pytest.raises(ValueError):
        param_groups(det, 1e-4, "no_such_policy")
    for policy in POLICIES:
        listed = [p for g in param_groups(det, 1e-4, policy) for p in g["params"]]
        assert len({id(p) for p in listed}) == len(listed) == len(list(det.parameters())), policy


def test_module_and_backbone_policies_on_the_projects_detector():
    """The two policies that the fixture test cannot decide on its own: which leaves are normalisation layers is read
    here from the project's detector itself (by exact type), and the expected groups are written out per parameter."""
    import detector_train_cases as DT
    case = DT.Case("small")
    det = case.detector(case.stored_maps())
    det.backbone = nn.Sequential(nn.Conv2d(3, 4, 3, bias=True), nn.BatchNorm2d(4))
    names = {}
    for n, p in det.named_parameters(remove_duplicate=False):
        names.setdefault(id(p), n)
    norm_owned, kinds = set(), set()
    for m in det.modules():
        if type(m) in (nn.LayerNorm, nn.GroupNorm, nn.BatchNorm2d):
            kinds.add(type(m))
            norm_owned.update(id(p) for p in m.parameters(recurse=False))
    assert kinds == {nn.LayerNorm, nn.GroupNorm, nn.BatchNorm2d}        # all three occur in the detector
    groups = param_groups(det, 1e-4, "backbone_no_norm_weight_decay")
    assert [(g.get("lr"), g.get("weight_decay")) for g in groups] == [(None, None), (1e-5, 0), (None, 0), (1e-5, None)]
    where = {id(p): gi for gi, g in enumerate(groups) for p in g["params"]}
    assert len(where) == len(list(det.parameters()))
    for i, n in names.items():
        want = (1 if i in norm_owned else 3) if "backbone" in n else (2 if i in norm_owned else 0)
        assert where[i] == want, (n, where[i], want)
    by_name = {n: where[i] for i, n in names.items()}
    assert by_name["backbone.0.weight"] == 3 and by_name["backbone.0.bias"] == 3      # a bias decays under this policy
    assert by_name["backbone.1.weight"] == 1 and by_name["backbone.1.bias"] == 1
    assert by_name["transformer.encoder.layers.0.norm1.weight"] == 2
    assert by_name["transformer.encoder.layers.0.linear1.bias"] == 0
    assert by_name["transformer.enc_output_norm.bias"] == 2 and by_name["transformer.enc_output.bias"] == 0
    assert all(len(g["params"]) > 0 for g in groups)
    groups = param_groups(det, 1e-4, "backbone")
    assert [(g.get("lr"), g.get("weight_decay")) for g in groups] == [(None, None), (1e-5, None)]
    assert [names[id(p)] for p in groups[1]["params"]] == [n for n in names.values() if "backbone" in n]
    assert [names[id(p)] for p in groups[0]["params"]] == [n for n in names.values() if "backbone" not in n]


# ---- the trajectories -------------------------------------------------------------------------------------------------
def test_cpu_path_follows_the_reference_trajectories(fx):
    params = fx.params()
    opt = ClippedAdamW(fx.groups(params), max_norm=fx.max_norm)
    advance = fx.schedulers(opt)
    worst = []
    for k in range(fx.steps):
        for i, p in enumerate(params):
            p.grad = fx.gradient(k, i)
        assert [g["lr"] for g in opt.param_groups] == fx.lrs[k].tolist()      # torch's schedulers drive it
        versions = [p._version for p in params]
        opt.step()
        advance(k)
        for i, p in enumerate(params):
            assert (p._version > versions[i]) == (p.grad is not None)
        fx.check_step(k, OC.state_triples(opt, params), float(opt.last_grad_norm), worst=worst)
    print("worst error / bound per step (tensors, norm):", worst)
    assert float(fx.d["norms"][3]) < fx.max_norm        # the clip-inactive step is in the run


def _pair(fx, cls_a, cls_b):
    pa, pb = fx.params(), fx.params()

    def make(cls, ps):
        if cls is ClippedAdamW:
            return ClippedAdamW(fx.groups(ps), max_norm=fx.max_norm)
        return torch.optim.AdamW(fx.groups(ps))
    return pa, make(cls_a, pa), pb, make(cls_b, pb)


def _run(fx, opt, params, steps):
    for k in steps:
        for i, p in enumerate(params):
            p.grad = fx.gradient(k, i) if (k, i) != fx.none_grad else torch.zeros_like(p)     # every step, every tensor
        if not isinstance(opt, ClippedAdamW):
            torch.nn.utils.clip_grad_norm_(params, fx.max_norm)
        opt.step()


@pytest.mark.parametrize("direction", ["torch_to_clipped", "clipped_to_torch"])
def test_state_dict_round_trip(fx, direction):
    first, second = (torch.optim.AdamW, ClippedAdamW) if direction == "torch_to_clipped" else (ClippedAdamW, torch.optim.AdamW)
    pa, a, pb, b = _pair(fx, first, second)
    pc, c, _, _ = _pair(fx, torch.optim.AdamW, torch.optim.AdamW)          # torch all the way
    _run(fx, a, pa, range(3))
    _run(fx, c, pc, range(3))
    sd = copy.deepcopy(a.state_dict())
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][0]["step"]) == 3.0
    with torch.no_grad():
        for q, p in zip(pb, pa):
            q.copy_(p)
    b.load_state_dict(sd)
    _run(fx, b, pb, range(3, 6))
    _run(fx, c, pc, range(3, 6))
    # Same operations in the same order; the one difference is the total norm, which this class sums in double and torch
    # in float32, so the clip coefficient may differ by one float32 rounding.  The scaled gradient then differs by one
    # rounding, its square (exp_avg_sq) by two, and re-rounding the sum adds one: three roundings of the largest element
    # per step, over the three steps after the hand-over.
    def close(x, y):
        err, bar = float((x - y).abs().max()), 3 * 3 * OC.ulp32(float(y.abs().max()))
        print("round trip: error", err, "bar", bar)
        return err <= bar
    for q, p in zip(pb, pc):
        assert close(q.detach(), p.detach())
    for k, s in c.state_dict()["state"].items():
        t = b.state_dict()["state"][k]
        assert float(t["step"]) == float(s["step"]) == 6.0
        assert close(t["exp_avg"], s["exp_avg"]) and close(t["exp_avg_sq"], s["exp_avg_sq"])


def test_loading_differing_steps_and_unsupported_options_raise(fx):
    params = fx.params()
    ref = torch.optim.AdamW(fx.groups(params))
    for k in range(3):                      # tensor 6 has no gradient at step 2: its step count lags
        for i, p in enumerate(params):
            p.grad = fx.gradient(k, i)
        ref.step()
    opt = ClippedAdamW(fx.groups(params))
    with pytest.raises(ValueError, match="steps differ"):
        opt.load_state_dict(ref.state_dict())
    p = [nn.Parameter(torch.zeros(3))]
    with pytest.raises(ValueError, match="amsgrad"):
        ClippedAdamW(p, amsgrad=True)
    with pytest.raises(ValueError, match="maximize"):
        ClippedAdamW(p, maximize=True)
    with pytest.raises(ValueError, match="float32"):
        ClippedAdamW([nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    with pytest.raises(ValueError, match="float32"):
        ClippedAdamW([nn.Parameter(torch.zeros(3, dtype=torch.bfloat16))])
    opt = ClippedAdamW(p)
    opt.add_param_group({"params": [nn.Parameter(torch.zeros(2))], "lr": 1e-5})       # before the first step: fine
    for g in opt.param_groups:
        for q in g["params"]:
            q.grad = torch.ones_like(q)
    opt.step()
    with pytest.raises(RuntimeError, match="before the first step"):
        opt.add_param_group({"params": [nn.Parameter(torch.zeros(2))]})
    opt.zero_grad()
    assert all(q.grad is None for g in opt.param_groups for q in g["params"])


def test_max_norm_zero_and_none_gradients_on_cpu():
    torch.manual_seed(1)
    pa = [nn.Parameter(torch.randn(5)), nn.Parameter(torch.randn(3, 3))]
    pb = [nn.Parameter(p.detach().clone()) for p in pa]
    a, b = ClippedAdamW(pa, lr=1e-2, max_norm=0.0), torch.optim.AdamW(pb, lr=1e-2, weight_decay=1e-4)
    for k in range(3):
        for p, q in zip(pa, pb):
            p.grad = torch.randn_like(p) * 5
            q.grad = p.grad.clone()
        if k == 1:
            pa[0].grad = pb[0].grad = None
        before = pa[0].detach().clone()
        a.step()
        b.step()
        if k == 1:
            assert torch.equal(pa[0], before)
        for p, q in zip(pa, pb):
            assert torch.equal(p, q)       # no clip: plain AdamW, the lagging step count of the skipped tensor included


# ---- tables -----------------------------------------------------------------------------------------------------------
def test_chunk_tables_cover_every_element_once():
    lengths = [1, 5, 1024, 2048, 3000, 7, 1000, 30, 1, 524288] + [3] * 400
    chunks, wave_first = build_tables(lengths)
    assert wave_first[0] == 0 and wave_first[-1] == chunks.size and (np.diff(wave_first) >= 1).all()
    covered = [np.zeros(n, dtype=np.int32) for n in lengths]
    for c in chunks:
        assert 1 <= c["count"] <= 1024 and c["start"] % 1024 == 0
        covered[c["record"]][c["start"]:c["start"] + c["count"]] += 1
    assert all((c == 1).all() for c in covered)
    per_item = [int(chunks["count"][a:b].sum()) for a, b in zip(wave_first[:-1], wave_first[1:])]
    assert max(per_item) <= 1024
    assert len(per_item) <= 512 + 8 + 4           # the 400 three-element tensors share two wave items, not 400 workgroups
    assert sum(1 for n in per_item if n == 1024) >= 512 + 1 + 2 + 2       # the big matrix spreads: one item per chunk


# ---- two gloo ranks ---------------------------------------------------------------------------------------------------
def _model():
    torch.manual_seed(5)
    return nn.Sequential(nn.Linear(6, 5), nn.Tanh(), nn.Linear(5, 3))


def _loss(model, seed):
    g = torch.Generator().manual_seed(seed)
    return model(torch.randn(7, 6, generator=g)).square().sum()


def _reducer_worker(rank, world, port, out_dir):
    from salience_detr_amd.data_parallel import StaticGradAllReducer
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        model = _model()
        red = StaticGradAllReducer(model.parameters())
        opt = ClippedAdamW.from_reducer(red, lr=1e-2, max_norm=0.1)
        assert opt.grad_scale == 0.5
        for step in range(3):
            model.zero_grad(set_to_none=True)
            _loss(model, 10 * step + rank).backward()
            red.pack()
            red.all_reduce(average=False)
            opt.step()
        torch.save({"params": [p.detach().clone() for p in model.parameters()], "norm": opt.last_grad_norm.clone()},
                   os.path.join(out_dir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


def test_reducer_path_on_two_gloo_ranks(tmp_path):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_reducer_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (torch.load(os.path.join(tmp_path, f"r{r}.pt")) for r in range(2))
    # one process: the summed gradients divided by two, then the same step
    model = _model()
    opt = ClippedAdamW(model.parameters(), lr=1e-2, max_norm=0.1)
    for step in range(3):
        grads = []
        for rank in range(2):
            model.zero_grad(set_to_none=True)
            _loss(model, 10 * step + rank).backward()
            grads.append([p.grad.clone() for p in model.parameters()])
        for p, a, b in zip(model.parameters(), *grads):
            p.grad = (a + b) / 2
        opt.step()
    for p, a, b in zip(model.parameters(), r0["params"], r1["params"]):
        assert torch.equal(a, b)
        assert torch.allclose(a, p.detach(), rtol=1e-6, atol=1e-7)
    assert torch.allclose(r0["norm"], opt.last_grad_norm, rtol=1e-6)


# ---- C ABI ------------------------------------------------------------------------------------------------------------
def test_new_symbols_exist_in_both_libraries():
    from salience_detr_amd import _hip
    from salience_detr_amd.csrc import build
    build.build()
    new = ["sdetr_adamw_chunk_elements", "sdetr_adamw_max_partials", "sdetr_adamw_grad_sumsq", "sdetr_adamw_clip_step"]
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "salience_hip.h")).read()
    for path in (build.LIB, build.F16_LIB):
        cdll = ctypes.CDLL(path)
        for name in new:
            assert hasattr(cdll, name), (path, name)
            assert name in _hip.SIGNATURES and name + "(" in header
    lib = _hip.lib()
    assert lib.sdetr_abi_version() == 1
    assert lib.sdetr_adamw_chunk_elements() == 1024 and lib.sdetr_adamw_max_partials() == 1024
    # host-side argument checks: nothing is launched
    assert lib.sdetr_adamw_grad_sumsq(None, 8, 0, 8, 1, 8, 1, 1, 8, 8) == _hip.EINVAL
    assert b"table sizes" in lib.sdetr_last_error()
    assert lib.sdetr_adamw_grad_sumsq(None, 8, 1, 8, 4, 8, 2, 3, 8, 8) == _hip.EINVAL and b"num_partials" in lib.sdetr_last_error()
    assert lib.sdetr_adamw_grad_sumsq(None, None, 1, 8, 4, 8, 2, 2, 8, 8) == _hip.EINVAL and b"null" in lib.sdetr_last_error()
    assert lib.sdetr_adamw_clip_step(None, 8, 1, 8, 4, 8, 2, 2, 8, 8, None, 0, 16, 16, 0.9, 0.999, 1e-8, 0.1, 1.0, 8) == _hip.EINVAL
    assert lib.sdetr_adamw_clip_step(None, 8, 1, 8, 4, 8, 2, 2, 8, 8, 8, 1, 16, 20, 0.9, 0.999, 1e-8, 0.1, 1.0, 8) == _hip.EINVAL
    assert b"16-byte" in lib.sdetr_last_error()
    assert lib.sdetr_adamw_clip_step(None, 8, 1, 8, 4, 8, 2, 2, 8, 8, 8, 1, 16, 16, 1.0, 0.999, 1e-8, 0.1, 1.0, 8) == _hip.EINVAL
    assert b"betas" in lib.sdetr_last_error()
