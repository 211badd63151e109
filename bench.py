#!/usr/bin/env python
"""Benchmark of the Salience-DETR encoder hot path on MI355X (contract: see task / DESIGN.md section 6).

    python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]   (N > 1: launched by torch.distributed.run)

One "step" = one pass of the hot path (F0 pyramid plumbing -> F1-F3 hierarchical salience filtering ->
6-layer salience encoder, i.e. reference SalienceTransformer.forward lines 97-183) over ONE batch of
synthetic 800x1333 4-level pyramids resident in HBM, batch-per-GPU = 2, bf16 encoder
(BASELINE.json configs[1]).  Images are independent, so N GPUs run N replicas of the path on their own
batches with no data-path collective (weak scaling); the timed region is bracketed by
barrier + synchronize on both sides and the MAX over ranks is reported.

Rank 0 prints ONE JSON line.  A plain run sets up, warms up, times the K steps and prints whole-job images/s
and `ms_per_step`; `--dump-outputs DIR` first writes what the last timed step returned (`memory`, the salience
maps) as float32 .npy files.  `--full` adds everything else: ms per encoder layer, the `roofline` object of the
dominant kernel (the fused MSDA gather, measured live with stream events around every launch of an
instrumented pass), batches in flight, the `train_step` and `configs` sub-records and, at N=1, the
`cpu_baseline` (the oracle's CPU port of the same path, timed on the host cores).
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
PROFILE_ROUND = "r06"   # profiles/<round>_msda_{traffic,rocprof,clock,bwd_traffic}.json: the source-tagged counter / trace records the line quotes
sys.path.insert(0, ROOT)

from salience_detr_amd import ms_deform_attn as msda_mod  # noqa: E402
from salience_detr_amd import pyramid, synthetic as syn  # noqa: E402
from salience_detr_amd.hot_path import build_hot_path  # noqa: E402

DEFAULT_THREADS = torch.get_num_threads()
HBM_PEAK_GBPS = 8000.0  # MI355X HBM3E spec peak (/opt/skills/guides/MI355X_MICROARCH.md)
MSDA_REPEATS = 8
CUT_PAIRS, CUT_REPLAYS = 30, 20   # in-step MSDA timing: paired cut-graph measurements
DUMP_BUDGET_BYTES = 60 << 20      # --dump-outputs: payload of all files together (64 MB less room for the .npy headers)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=2, help="images per GPU")
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--mode", choices=["infer", "train"], default="infer",
                    help="infer (default, BASELINE.json configs[1]) or train: fp32 forward+backward of the hot path, "
                         "bucketed RCCL gradient all-reduce overlapped with backward, AdamW step (configs[2])")
    ap.add_argument("--x3-linear", dest="x3_linear", action="store_true", default=True,
                    help="train mode: weight gradients of the nn.Linear layers through sdetr_gemm_x3_f32 (default)")
    ap.add_argument("--no-x3-linear", dest="x3_linear", action="store_false")
    ap.add_argument("--no-zero-arena", dest="zero_arena", action="store_false", default=True,
                    help="training step: every zero-initialised buffer its own fill launch (the state before round 6), for A/B runs")
    ap.add_argument("--force-dist-path", action="store_true",
                    help="train mode, one process: take the N > 1 execution path anyway (captured forward + backward + "
                         "gradient pack, eager flat all-reduce + optimizer) -- how that path is exercised on a 1-GPU box")
    ap.add_argument("--train-steps", type=int, default=5,
                    help="the --full line's `train_step` sub-record: this many timed training steps (0: skip)")
    ap.add_argument("--config-steps", type=int, default=10,
                    help="the --full line's `configs` sub-records (fp32 path, BASELINE configs[3] and configs[4] at N = 1): "
                         "timed steps each (0: skip)")
    ap.add_argument("--in-flight", dest="in_flight", type=int, default=1,
                    help="without --full only, informational: this many independent batches (own inputs, own graph, own "
                         "stream) replayed side by side; the official line is 1")
    ap.add_argument("--in-flight-report", dest="in_flight_report", type=int, default=3,
                    help="the full line's informational `batches_in_flight` object: this many lanes (0/1: skip)")
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--width", type=int, default=1333)
    ap.add_argument("--value-dtype", choices=["same", "fp16"], default="fp16",
                    help="storage type of the head-major value maps sampled by the MSDA kernel in bf16 mode: fp16 "
                         "(default; 11-bit mantissa, gather via v_fma_mix_f32) or the activation dtype (bf16)")
    ap.add_argument("--no-graph", action="store_true", help="time eager launches instead of a hipGraph replay")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    depth = ap.add_mutually_exclusive_group()
    depth.add_argument("--full", action="store_true",
                       help="after the headline measurement: ms per encoder layer, the MSDA roofline (instrumented pass, "
                            "cut graphs), batches in flight, the train_step and configs sub-records and the CPU baseline "
                            "with its parity check")
    depth.add_argument("--plain", action="store_true",
                       help="the default without --full: only the timed loop and the headline JSON line (what the "
                            "rocprofv3 counter passes wrap); kept for the scripts that name it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last one returned as DIR/<name>.npy (float32, a training "
                         "loss float64; at most %d MiB in all, larger outputs as a fixed seeded sample of their elements)"
                         % (DUMP_BUDGET_BYTES >> 20))
    ap.add_argument("--cpu-protocol", choices=["bounded", "full"], default="bounded",
                    help="--full only: bounded (default): batch 2, all cores, 1 warm-up + 3 passes; full: SURVEY.md 8(d) -- 3 warm-ups + "
                         "10 passes at all cores and at 8 threads, batch 1 and 2 (minutes)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.in_flight > 1:
        ap.error("--dump-outputs times one batch at a time: drop --in-flight")
    return args


def make_inputs(batch, h, w, device, seed):
    sizes = [(h, w)] * batch
    canvas = syn.pad_to_32(h, w)
    _, masks = syn.make_masks(sizes)
    shapes = pyramid.level_shapes_of(masks)
    feats = syn.make_feats(batch, shapes, 256, seed=seed)
    pos = [syn.sine_position_embedding(m, 128) for m in masks]
    cpu = (feats, masks, pos)
    dev = tuple([t.to(device) for t in ts] for ts in cpu)
    return sizes, canvas, shapes, cpu, dev


def dump_outputs(directory, arrays):
    """--dump-outputs: each named tensor as DIR/<name>.npy in float32 (float64 stays float64).  When the outputs
    together exceed DUMP_BUDGET_BYTES, each is replaced by the same share of its elements, picked by a fixed seed and
    kept in flat-index order: the same positions on every run, so two builds compare element for element."""
    import numpy as np
    arrays = {k: v.detach().cpu() for k, v in arrays.items()}
    arrays = {k: v if v.dtype == torch.float64 else v.float() for k, v in arrays.items()}
    total = sum(v.numel() * v.element_size() for v in arrays.values())
    os.makedirs(directory, exist_ok=True)
    for name, a in arrays.items():
        if total > DUMP_BUDGET_BYTES:
            keep = a.numel() * DUMP_BUDGET_BYTES // total
            pick = torch.randperm(a.numel(), generator=torch.Generator().manual_seed(0))[:keep].sort().values
            a = a.flatten()[pick]
        np.save(os.path.join(directory, name + ".npy"), a.numpy())


def algorithmic_bytes(B, Nv, Nq, M, D, L, P, value_bytes, proj_bytes, out_bytes, ref_dim=2):
    """Each input and output of the fused MSDA launch touched exactly once (SURVEY.md 8(d) formula with the
    fused kernel's actual operands: 3 projection values per sample instead of loc(2)+weight(1), plus the
    fp32 reference points)."""
    return B * (Nv * M * D * value_bytes + Nq * M * L * P * 3 * proj_bytes + Nq * L * ref_dim * 4
                + Nq * M * D * out_bytes)


def train_record(args, model, device, rank, world, dist, steps, warmup, force_dist_path=False):
    """configs[2]: one training step of the hot-path modules per batch of 2 images per GPU -- fp32 forward
    through the autograd path (HIP MSDA forward/backward op), the salience criterion (row N4: targets + focal loss
    on the salience maps, synthetic ground-truth boxes) plus a synthetic loss on `memory`, backward, gradient
    all-reduce over RCCL, AdamW.  Returns the result record (every rank; rank 0 prints it).

    Execution: forward + backward (+ the pack of the gradients into one flat buffer) is ONE replayed hipGraph at every
    world size.  A single process also captures the optimizer step; with ranks, the replay is followed by one all-reduce
    of the flat gradient buffer and the fused AdamW step, both eager (3 host calls per step: the step stays
    device-bound, and N = 1 and N > 1 run the same captured kernels)."""
    from salience_detr_amd.data_parallel import StaticGradAllReducer, broadcast_parameters
    from salience_detr_amd.salience_criterion import SalienceCriterion
    from salience_detr_amd.salience_filtering import replay_safe_mean
    sizes, canvas, level_shapes, _, (feats, masks, pos) = make_inputs(args.batch, args.height, args.width, device,
                                                                      seed=rank)
    model.train()
    if args.x3_linear:
        from salience_detr_amd.linear_x3 import use_x3_linear_
        use_x3_linear_(model)   # weight gradients of the Linear layers on the bf16 matrix cores at fp32 accuracy
        if os.environ.get("SDETR_X3_ALL"):   # A/B: every forward / input-gradient product on the x3 kernel too
            from salience_detr_amd import linear_x3
            linear_x3.X3_WIDE_FEATURES, linear_x3.X3_WIDE_OUT_ROWS, linear_x3.X3_LONG_REDUCTION_ROWS = 1, 1, 1
    if dist is not None:
        broadcast_parameters(model)
    params = [p for p in model.parameters() if p.requires_grad]
    # one fused multi-tensor update for the ~300 parameter tensors (the single-tensor path is ~10 tiny launches per
    # parameter: ~3000 per step); capturable: the step lives in a hipGraph
    try:
        opt = torch.optim.AdamW(params, lr=1e-4, weight_decay=1e-4, capturable=True, fused=True)
    except (RuntimeError, TypeError, ValueError):
        opt = torch.optim.AdamW(params, lr=1e-4, weight_decay=1e-4, capturable=True, foreach=True)
    use_ranks_path = dist is not None or force_dist_path
    reducer = StaticGradAllReducer(params) if use_ranks_path else None
    w = None
    criterion = SalienceCriterion()
    strides = [(canvas[0] / h, canvas[1] / w_) for h, w_ in level_shapes]
    targets = []
    for i in range(args.batch):   # 12 deterministic boxes per image over all four scale ranges
        c = syn.det_rand(f"bench.box.c{i}", (12, 2), salt=rank) * 0.8 + 0.1
        wh = 0.02 + syn.det_rand(f"bench.box.wh{i}", (12, 2), salt=rank) ** 2 * 0.9
        targets.append({"boxes": torch.cat([c, wh], -1).to(device)})

    # ground-truth boxes staged on the device once (the data loader's side); the target maps are built every step
    staged = criterion.stage_boxes(targets, sizes, device)

    # every zero-initialised fp32 buffer of the step's autograd nodes (split-reduction outputs, weight / bias gradients,
    # LayerNorm's dw | db, the MSDA backward's grad_value: ~150 per step) is a slice of ONE buffer cleared by ONE fill
    # kernel at the start of the step (salience_detr_amd/zero_arena.py); the first warm-up step measures the demand
    from salience_detr_amd.zero_arena import ZeroArena
    import contextlib
    arena = ZeroArena(device) if getattr(args, "zero_arena", True) else None

    def forward_backward():
        nonlocal w
        opt.zero_grad(set_to_none=True)
        with (arena.step() if arena is not None else contextlib.nullcontext()):
            memory, score_maps = model(feats, masks, pos, image_sizes=sizes, canvas=canvas)
            if w is None:   # fixed weights of the synthetic loss on `memory` (name-seeded: the same on every run and rank)
                w = syn.det_randn("bench.train.memory_weights", tuple(memory.shape)).to(memory.device)
            # (the mean over `memory` as per-image column means + a 512-element mean: the framework's one-kernel reduction
            # of 11 M elements clears its semaphores with a hipMemsetAsync that a replayed hipGraph does not reproduce here)
            loss = replay_safe_mean(memory * w) + criterion(score_maps, targets, strides, sizes, staged=staged)["loss_salience"]
            loss.backward()
            if reducer is not None:
                reducer.pack()
        # (detached: a loss that keeps its autograd graph alive across iterations keeps the AccumulateGrad nodes of the
        # first iteration -- created on the default stream -- alive too, and the capture then records the gradient
        # accumulation on another stream than the kernels that produce the gradients)
        return loss.detach()

    def finish():   # what follows the captured region when there are ranks
        reducer.all_reduce(average=True)
        opt.step()

    def finish_single():   # one process: the fused AdamW step, eager, behind the replayed forward + backward
        opt.step()

    def step():
        loss = forward_backward()
        if reducer is not None:
            finish()
        else:
            finish_single()
        return loss

    # the timed steps start from the INITIAL parameters and optimizer state whatever the warm-up and the capture did
    # (the single-process capture runs the optimizer, the N > 1 capture does not): the loss after K steps is then the same
    # number on every execution path -- tests/test_rccl_path_gpu.py compares them
    initial = [p.detach().clone() for p in params]

    def reset_training_state():
        with torch.no_grad():
            torch._foreach_copy_(params, initial)
            for st in opt.state.values():
                for v in st.values():
                    if torch.is_tensor(v):
                        v.zero_()

    for _ in range(max(warmup, 2)):
        step()

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # the eager step issues ~1600 launches from Python and is host-bound as soon as the kernels get faster
    graph = None
    graph_note = "eager"
    capture_kw = {"capture_error_mode": "thread_local"} if dist is not None else {}
    if not args.no_graph:
        try:
            # The optimizer step stays OUTSIDE the captured region at every world size (round 4).  Captured together with
            # forward + backward (rounds 2-3, single process) the fused AdamW kernels did not reproduce the eager update on
            # this stack: same first-step gradients, a different second-step loss (4.58 against 4.39; 5.22 with the library's
            # Linear products) -- the loss trace of SDETR_BENCH_LOSS_TRACE=1 shows it.  Replayed forward + backward followed
            # by the eager fused step reproduces the eager trajectory to the last digit (tests/test_rccl_path_gpu.py).
            graph, loss_static = capture(forward_backward, capture_kw, strict=True)
            if reducer is not None:
                finish()      # (capture() replays once: complete that step)
                graph_note = ("hipGraph replay of forward + backward + gradient pack, then one eager all-reduce of the "
                              "flat gradient buffer and the fused AdamW step")
            else:
                finish_single()
                graph_note = "hipGraph replay of forward + backward, then the eager fused AdamW step"
        except Exception as e:   # a host synchronisation inside the autograd path: report it, time the eager step
            graph = None
            graph_note = "eager (capture failed: %s)" % str(e).split("\n")[0][:120]
            if os.environ.get("SDETR_BENCH_TRACEBACK"):
                import traceback
                traceback.print_exc()
            torch.cuda.synchronize()
            for _ in range(2):
                step()

    def timed_step():
        if graph is not None:
            graph.replay()
            if reducer is not None:
                finish()
            else:
                finish_single()
            return loss_static
        return step()

    for _ in range(2):   # (two more steps in their final form before the state is reset and the clock starts)
        timed_step()
    reset_training_state()
    fence()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = timed_step()
    fence()
    elapsed = time.perf_counter() - t0
    final_loss = float(loss.detach())
    if dist is not None:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    loss_trace = None
    if os.environ.get("SDETR_BENCH_LOSS_TRACE"):
        # debugging / tests: the loss of every one of 4 steps from the initial state (host read-back per step)
        reset_training_state()
        loss_trace = []
        for i in range(4):
            loss_trace.append(float(timed_step().detach()))
            if i == 0:   # gradients behind the first update: how many parameter tensors have one, their L1 norms
                torch.cuda.synchronize()
                gs = [p.grad for p in params]
                norms = [0.0 if g_ is None else float(g_.abs().sum()) for g_ in gs]
                if os.environ.get("SDETR_BENCH_GRAD_DUMP"):
                    names = [n for n, p in model.named_parameters() if p.requires_grad]
                    json.dump(dict(zip(names, norms)), open(os.environ["SDETR_BENCH_GRAD_DUMP"], "w"), indent=0)
                loss_trace.append({"no_grad": sum(g_ is None for g_ in gs), "zero_grad": sum(n == 0.0 for n in norms),
                                   "l1_total": sum(norms), "l1_first10": [round(n, 4) for n in norms[:10]],
                                   "param_l1": float(sum(p.detach().abs().sum() for p in params))})
    if loss_trace is not None and graph is not None:
        # the same parameters through the replayed graph and through an eager forward: must give the same loss
        snap = [p.detach().clone() for p in params]
        replay_loss = float(timed_step().detach())
        with torch.no_grad():
            torch._foreach_copy_(params, snap)
        eager_loss = float(forward_backward().detach())
        rec = {"same_parameters": {"replayed": replay_loss, "eager": eager_loss}}
        loss_trace.append(rec)
    # dominant kernel of the training step: the MSDA backward op (grad_value scatter + grad_loc / grad_aw gather;
    # LDS-accumulating kernel from 1200 queries up, direct global-atomic kernel below); timed with stream events
    # around the op (bucketing launches and the zero fill of grad_value included)
    evs, nbytes = [], []
    real_bwd = msda_mod.ms_deform_attn_backward

    def timed_bwd(value, shapes, lsi, loc, aw, grad_out, step_):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = real_bwd(value, shapes, lsi, loc, aw, grad_out, step_)
        e1.record()
        evs.append((e0, e1))
        B, Nv, M, D = value.shape
        Nq, L, P = loc.shape[1], loc.shape[3], loc.shape[4]
        nbytes.append(4 * B * (2 * Nv * M * D + 2 * Nq * M * L * P * 3 + Nq * M * D))  # SURVEY.md 8(d) backward
        return r

    msda_mod.ms_deform_attn_backward = timed_bwd
    try:
        for _ in range(2):
            step()
        torch.cuda.synchronize()
    finally:
        msda_mod.ms_deform_attn_backward = real_bwd
    tot_us = sum(e0.elapsed_time(e1) for e0, e1 in evs) * 1e3
    achieved = sum(nbytes) / tot_us / 1e3
    # HBM bytes of the op at the LARGEST layer (11 363 queries, batch 2) from committed counter passes, reported only while
    # the backward kernels' sources are the ones the passes ran on
    bwd_traffic, bwd_traffic_at, bwd_traffic_src = None, None, "null: no committed counter passes (profiles/%s_msda_bwd_traffic.json)" % PROFILE_ROUND
    try:
        import hashlib
        tj = json.load(open(os.path.join(ROOT, "profiles", PROFILE_ROUND + "_msda_bwd_traffic.json")))
        h = hashlib.sha256()
        for f in tj["sources"]:
            h.update(open(os.path.join(ROOT, f), "rb").read())
        if h.hexdigest()[:16] == tj["source_tag"] and tj["batch"] == args.batch:
            bwd_traffic = int(tj["hbm_bytes_per_op"])
            bwd_traffic_at = {"num_query": tj["num_query"], "algorithmic_bytes": max(nbytes) if nbytes else None}
            bwd_traffic_src = "profiles/%s_msda_bwd_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes over the op at %d queries, sources %s)" % (PROFILE_ROUND, tj["num_query"], tj["source_tag"])
        else:
            bwd_traffic_src = "null: committed passes were measured on other kernel sources or another batch size"
    except (OSError, KeyError, ValueError):
        pass
    return {
        "metric": "images/s (whole node) + ms/encoder-layer, ResNet50 800x1333",
        "value": round(world * args.batch * steps / elapsed, 2), "unit": "images/s", "n_gpus": world,
        "steps": steps, "warmup": warmup, "ms_per_step": round(elapsed * 1e3 / steps, 4),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "fp32", "data": "synthetic",
        "config": {"workload": "salience_detr_resnet50_800_1333 training step of the hot path (filtering + 6-layer "
                               "encoder fwd+bwd, salience focal loss + synthetic memory loss, AdamW), batch=%d per MI355X" % args.batch,
                   "batch_per_gpu": args.batch, "global_batch": args.batch * world,
                   "parallelism": "data parallel, one all-reduce of the flat gradient buffer over RCCL after the replayed "
                                  "forward + backward" if use_ranks_path else "single GPU",
                   "grad_bytes": reducer.num_bytes if reducer is not None else sum(p.numel() * 4 for p in params),
                   "execution": graph_note, "x3_linear": bool(args.x3_linear), "world_size": world,
                   "hipgraph_nodes": CAPTURE_INFO.get("graph_nodes") if graph is not None else None,
                   "zero_arena": (None if arena is None else
                                  {"bytes": 0 if arena.buf is None else int(arena.buf.numel() * 4),
                                   "buffers_served_per_step": int(arena.fills_saved)}),
                   "backend": (dist.get_backend() if dist is not None else "none (single process)")},
        "roofline": {"kernel": "MSDA backward op: sdetr::bt_main_kernel (fixed-point LDS windows) + bucketing, "
                               "sdetr::msda_col2im_chan_kernel below 1200 queries", "bound": "hbm",
                     "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": bwd_traffic, "traffic_at": bwd_traffic_at, "traffic_source": bwd_traffic_src,
                     "avg_launch_us": round(tot_us / max(1, len(evs)), 1)},
        "loss": final_loss,   # of the last timed step, `steps` AdamW updates after the initial state
        "loss_trace": loss_trace,
    }


def train_main(args, model, device, rank, world, dist):
    result = train_record(args, model, device, rank, world, dist, args.steps, args.warmup,
                          force_dist_path=args.force_dist_path)
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, {"loss": torch.tensor([result["loss"]], dtype=torch.float64)})
    if rank == 0:
        print(json.dumps(result))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


def spawn_ranks_if_needed(args):
    """`python bench.py --gpus N` (N > 1) without a launcher environment runs itself under torch.distributed.run
    with N ranks on this node, in a child process, and exits with its status, so the printed `n_gpus` is always the
    number of ranks that actually ran (the reference launches its ranks with `accelerate launch`, main.py:94-103,144)."""
    if args.gpus <= 1 or "WORLD_SIZE" in os.environ:
        return
    import socket
    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    import subprocess
    sys.exit(subprocess.call(cmd))


def kernel_source_tag():
    """sha256 over the MSDA forward kernel sources: the identity the committed PMC traffic numbers are tagged with
    (there is no .git on the benchmark box)."""
    import hashlib
    h = hashlib.sha256()
    for name in ("msda_resident.hip", "msda_forward.hip", "common.h"):
        with open(os.path.join(ROOT, "salience_detr_amd", "csrc", name), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def graph_time_us(fn, reps):
    """Mean device time of `fn`'s launches: `reps` repetitions captured in a hipGraph and replayed between two
    events -- device time without host launch gaps (the python wrapper of a launch costs more host time than the
    small layers' kernels run)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


CAPTURE_INFO = {}     # node statistics of the most recent capture() (salience_detr_amd/graph_guard.py)


def capture(step, capture_kw, strict=False):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    from salience_detr_amd import graph_guard
    g = graph_guard.new_graph()
    dump = os.environ.get("SDETR_BENCH_GRAPH_DOT")
    if dump:
        g.enable_debug_mode()
    with torch.cuda.graph(g, **capture_kw):
        out = step()
    if dump:
        g.debug_dump(dump)
    # a memset node would not be reproduced by the replays that are timed (CHANGELOG round 4): the training step refuses
    # to time such a graph (`strict`), every capture records what was found
    types = graph_guard.node_types(g)
    CAPTURE_INFO["graph_nodes"] = len(types)
    CAPTURE_INFO["memset_nodes"] = graph_guard.memset_nodes(g) if types else None
    if strict:
        graph_guard.assert_replay_safe(g, "bench.py capture")
    elif CAPTURE_INFO["memset_nodes"]:
        print("bench.py: captured graph holds %d memset node(s)" % CAPTURE_INFO["memset_nodes"], file=sys.stderr)
    g.replay()
    torch.cuda.synchronize()
    return g, out


def make_lanes(model, args, device, rank, first, n, capture_kw, sizes, canvas):
    """`n` independent batches of the workload, each with its own inputs, hipGraph and stream (the first is the bench's
    own).  They share the model -- weights and packed operands, all read-only -- and nothing else.  Each entry keeps
    its step function, which owns the lane's inputs: the graph only has their addresses."""
    g, out, step = first
    lanes = [(torch.cuda.current_stream(), g, out, step)]
    for i in range(1, n):
        _, _, _, _, (f2, m2, p2) = make_inputs(args.batch, args.height, args.width, device, seed=rank + 100 * i)

        def step_i(f2=f2, m2=m2, p2=p2):
            with torch.no_grad():
                return model(f2, m2, p2, image_sizes=sizes, canvas=canvas)[0]
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            gi, oi = capture(step_i, capture_kw)
        lanes.append((st, gi, oi, step_i))
    torch.cuda.synchronize()
    return lanes


def lane_runner(lanes):
    """One call = one step (one batch through the hot path); the lanes take turns, each on its own stream."""
    def run():
        st, gi, _, _ = lanes[run.n % len(lanes)]
        run.n += 1
        with torch.cuda.stream(st):
            gi.replay()
    run.n = 0
    return run


def lanes_match_solo(lanes):
    """Side by side the lanes must produce the bits they produce alone."""
    for st, gi, _, _ in lanes:
        with torch.cuda.stream(st):
            gi.replay()
    torch.cuda.synchronize()
    together = [o.clone() for _, _, o, _ in lanes]
    same = True
    for (st, gi, o, _), ref in zip(lanes, together):
        with torch.cuda.stream(st):
            gi.replay()
        torch.cuda.synchronize()
        same = same and bool(torch.equal(o, ref))
    return same


def time_replays(g, n):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


STRESS_LEVELS = [(200, 336), (100, 168), (50, 84), (25, 42)]   # the reference's 5scale pyramid (strides 4-32)


def _first_tensor(o):
    while isinstance(o, (list, tuple)):
        o = o[0]
    return o


def _graph_ms(step, steps, warmup=3, check=None):
    """ms per call of `step` under hipGraph replay (eager launches if the capture fails).  ``check`` (a dict) receives
    ``replay_vs_eager_max_abs``: the replayed graph's first output against the eager call's on the same inputs."""
    for _ in range(warmup):
        eager_out = step()
    torch.cuda.synchronize()
    try:
        g, out = capture(step, {})
        time_replays(g, 3)
        if check is not None:
            a, b = _first_tensor(out), _first_tensor(eager_out)
            check["replay_vs_eager_max_abs"] = float((a.float() - b.float()).abs().max())
        return time_replays(g, steps), True
    except Exception:
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps, False


def config_records(args, device, steps=10):
    """Sub-records of the default line for the other BASELINE.json configurations / arithmetic modes on ONE GPU
    (VERDICT r3 item 3): each its own model instance and inputs, `steps` timed steps under hipGraph replay.

    * ``fp32``     the parity-bar path: fp32 inference of the hot path, batch 2, 800x1333 -- with the 1e-3 check against
                   the reference's fp32 fixture (tests/golden/hotpath_full_digest.npz, single-image case) inline;
    * ``config4``  BASELINE configs[3] at N = 1: bf16, batch 1 per GPU on the large 4-level pyramid of the reference's
                   5scale configuration (salience_detr_resnet50_5scale_800_1333.py:33-36: 89 250 tokens, 45 330 queries);
    * ``config5``  BASELINE configs[4] at N = 1: the whole SalienceTransformer (neck, encoder, two-stage proposals + NMS,
                   6 decoder layers at 900 queries; salience_transformer.py:97-226,552-674) on 800x1333 + 800x1066,
                   in fp16: IEEE-half activations since round 5 (libsalience_hip_f16.so, ``resolve_activation_dtype``;
                   the record states what ran and which library served it);
    * ``config5_fp32`` the same whole transformer in fp32 arithmetic (the figure rounds 2-4 had to quote for this
                   configuration, kept for the trend)."""
    import numpy as np
    from salience_detr_amd.hot_path import resolve_activation_dtype
    out = {}

    def guarded(name, fn):
        try:
            out[name] = fn()
        except Exception as e:   # a sub-record must not take the line down
            out[name] = {"error": str(e).split("\n")[0][:200]}
        torch.cuda.empty_cache()

    def fp32():
        m = build_hot_path()
        m.load_state_dict(syn.det_state_dict(m.state_dict()))
        m = m.to(device).eval()
        sizes, canvas, level_shapes, _, (feats, masks, pos) = make_inputs(args.batch, args.height, args.width, device, seed=0)

        def step():
            with torch.no_grad():
                return m(feats, masks, pos, image_sizes=sizes, canvas=canvas)[0]
        chk = {}
        ms, graphed = _graph_ms(step, steps, check=chk)
        rec = {"workload": "salience_detr_resnet50_800_1333 fp32 inference, batch=%d: the path that carries the 1e-3 parity "
                           "claim" % args.batch, "dtype": "fp32", "ms_per_step": round(ms, 4),
               "images_per_s": round(args.batch * 1e3 / ms, 1), "steps": steps, "hipgraph": graphed, **chk}
        fixture = os.path.join(ROOT, "tests", "golden", "hotpath_full_digest.npz")
        if os.path.exists(fixture) and (args.height, args.width) == (800, 1333):
            d = np.load(fixture)
            s1, c1, _, _, (f1, m1, p1) = make_inputs(1, 800, 1333, device, seed=0)
            with torch.no_grad():
                mem = m(f1, m1, p1, image_sizes=s1, canvas=c1)[0]
            err = float((mem.float().cpu()[:, ::41, ::3] - torch.from_numpy(d["single.memory_sub"])).abs().max())
            rec["parity"] = {"max_abs_err_vs_reference_fp32": round(err, 6), "bar": 1e-3, "ok": err < 1e-3,
                             "against": "tests/golden/hotpath_full_digest.npz single.memory_sub (the imported reference's fp32 "
                                        "run of one 800x1333 image, every 41st token x every 3rd channel)"}
        return rec

    def config4():
        m = build_hot_path(max_num_embedding=500)
        m.load_state_dict(syn.det_state_dict(m.state_dict()))
        m = m.to(device).eval()
        m.set_encoder_dtype(torch.bfloat16, torch.float16)
        sizes = [(800, 1333)]
        _, masks = syn.make_masks(sizes, STRESS_LEVELS)
        feats = [f.to(device) for f in syn.make_feats(1, STRESS_LEVELS, 256, seed=0)]
        pos = [syn.sine_position_embedding(x, 128).to(device) for x in masks]
        masks = [x.to(device) for x in masks]
        canvas = syn.pad_to_32(800, 1333)
        holder = {}

        def step():
            with torch.no_grad():
                r = m(feats, masks, pos, image_sizes=sizes, canvas=canvas, return_aux=("nq" not in holder))
            if "nq" not in holder:
                holder["nq"] = [int(t.shape[1]) for t in r[2]["foreground_inds"]]
            return r[0]
        step()
        chk = {}
        ms, graphed = _graph_ms(step, steps, check=chk)
        return {**chk, "workload": "BASELINE configs[3] at N=1: bf16 inference, batch=1 per GPU, large 4-level pyramid "
                            "(200x336 .. 25x42, 89 250 tokens: the reference's 5scale configuration)",
                "dtype": "bf16", "value_map_storage": "fp16", "ms_per_step": round(ms, 4),
                "images_per_s": round(1e3 / ms, 1), "steps": steps, "hipgraph": graphed,
                "levels": [list(x) for x in STRESS_LEVELS], "num_queries_per_layer": holder.get("nq")}

    def config5(fp32_arithmetic=False):
        from salience_detr_amd.salience_transformer import build_salience_transformer
        sizes = [(800, 1333), (800, 1066)]
        tr = build_salience_transformer(with_neck=True)
        tr.load_state_dict(syn.det_state_dict(tr.state_dict()))
        tr = tr.eval().to(device)
        act, vdt = resolve_activation_dtype(torch.float16)
        if fp32_arithmetic:
            act, vdt = torch.float32, torch.float32   # (the module's default: nothing to set)
        else:
            tr.set_dtype(torch.float16, None)
        tr.static_proposals = True
        img_mask, masks = syn.make_masks(sizes)
        canvas = tuple(img_mask.shape[-2:])
        shapes = [tuple(x.shape[-2:]) for x in masks]
        feats = [f.to(device) for f in syn.make_feats(2, shapes, 256, 0)]
        pos = [syn.sine_position_embedding(x, 128).to(device) for x in masks]
        masks = [x.to(device) for x in masks]

        def step():
            with torch.no_grad():
                return tr(feats, masks, pos, image_sizes=sizes, canvas=canvas)
        chk = {}
        ms, graphed = _graph_ms(step, steps, check=chk)
        from salience_detr_amd import _hip
        ran = str(tr.decoder.layers[0].linear1.weight.dtype).replace("torch.", "")
        return {**chk, "workload": "BASELINE configs[4] at N=1: whole SalienceTransformer (RepVGGPluX neck, encoder, two-stage "
                            "proposals + NMS, 6 decoder layers, 900 queries), batch=2 (800x1333 + 800x1066)",
                "requested_dtype": "fp16", "served_as": {"activations": str(act).replace("torch.", ""),
                                                         "value_maps": str(vdt).replace("torch.", ""),
                                                         "module_parameters": ran,
                                                         "library": "libsalience_hip_f16.so" if (ran == "float16" and _hip._lib_f16 is not None)
                                                                    else "libsalience_hip.so"},
                "ms_per_step": round(ms, 4), "images_per_s": round(2e3 / ms, 1), "steps": steps, "hipgraph": graphed,
                "queries": 900}

    guarded("fp32", fp32)
    guarded("config4", config4)
    guarded("config5", config5)
    # The same configuration in fp32 arithmetic.  Rounds 2-4 served the fp16 request with bf16 activations (a precision BELOW
    # the one named) and this record was the configuration's only valid figure; since round 5 `config5` runs IEEE-half
    # activations (stated in `served_as`) and this one stays for the trend.
    guarded("config5_fp32", lambda: config5(fp32_arithmetic=True))
    return out


def cpu_baseline(args, model, cpu_inputs_of, out, sel_log, gpu_inds=None):
    """The oracle's CPU port of the same path, timed on the host cores: per stage (F0-F3 filtering,
    each encoder layer, the MSDA core alone).  Default: bounded to ~15-30 s (batch 2; 8 threads 1 warm-up + 3 passes,
    all cores 1 + 2 passes; the faster leg is `value`);
    `--cpu-protocol full` runs the survey's whole protocol (3 warm-ups + 10 passes, all cores AND 8 threads, batch 1
    AND 2 -- minutes; its result is committed under profiles/)."""
    from oracle import salience_ref as R  # checker / baseline only; never on the product path
    from oracle import msda_c
    sd = {k: v.detach().float().cpu() for k, v in model.state_dict().items()}
    # torch's default intra-op thread count = the physical cores (hyper-thread siblings only slow the GEMMs down:
    # 62 s per pass at 256 threads against 4 s at 128 on a 2 x 64-core EPYC 9575F)
    all_cores = DEFAULT_THREADS
    full = args.cpu_protocol == "full"
    # (batch, threads, warm-ups, timed passes).  The torch CPU ops of this path run FASTER on 8 threads than on all
    # 128 physical cores on the benchmark boxes (1.1 s against 4-10 s per batch-2 pass: the tensors are small, the
    # thread fan-out dominates), so the bounded default times both and reports the faster one as `value`.
    if full:
        plans = [(args.batch, all_cores, 3, 10), (1, all_cores, 3, 10), (args.batch, 8, 3, 10), (1, 8, 3, 10)]
    else:
        plans = [(args.batch, 8, 1, 3), (args.batch, all_cores, 1, 2)]
    legs, ref_out = [], None
    cpu_model = ""
    try:
        with open("/proc/cpuinfo") as fh:
            cpu_model = next((l.split(":", 1)[1].strip() for l in fh if l.startswith("model name")), "")
    except OSError:
        pass
    for batch, threads, warm, reps in plans:
        torch.set_num_threads(threads)
        cf, cm, cp = cpu_inputs_of(batch)
        per_pass, stages = [], []
        with torch.no_grad():
            for i in range(warm + reps):
                tm = {}
                t1 = time.perf_counter()
                r = R.hot_path(sd, cf, cm, cp, timings=tm)
                dt = time.perf_counter() - t1
                if i >= warm:
                    per_pass.append(dt)
                    stages.append(tm)
                if batch == args.batch:
                    ref_out = r
        order = sorted(range(len(per_pass)), key=lambda i: per_pass[i])
        med = order[len(order) // 2]
        legs.append({"batch": batch, "threads": threads, "warmups": warm, "passes": reps,
                     "ms_per_pass_median": round(per_pass[med] * 1e3, 1),
                     "images_per_s": round(batch / per_pass[med], 3),
                     "ms_per_stage": {k: round(v * 1e3, 1) for k, v in sorted(stages[med].items())}})
    torch.set_num_threads(all_cores)
    main_leg = max((l for l in legs if l["batch"] == args.batch), key=lambda l: l["images_per_s"])
    result = {
        "value": main_leg["images_per_s"], "unit": "images/s", "cores": main_leg["threads"], "kind": "port",
        "cpu_model": cpu_model, "msda_core_threads": msda_c.num_threads(),
        "sample": "%d timed passes (after %d warm-up) of the same batch-%d 800x1333 hot path (oracle/salience_ref.py, "
                  "fp32, torch CPU ops + OpenMP C gather), median; per-stage ms of the median pass"
                  % (main_leg["passes"], main_leg["warmups"], main_leg["batch"]),
        "ms_per_pass": main_leg["ms_per_pass_median"], "ms_per_stage": main_leg["ms_per_stage"], "protocol": args.cpu_protocol,
        "legs": legs,
    }
    # ---- parity of the timed GPU output against the oracle, selection flips separated from rounding ----
    parity = None
    if ref_out is not None:
        err = (out.float().cpu() - ref_out["memory"]).abs()
        per_token = err.max(-1)[0]
        B, S = per_token.shape
        flipped = torch.zeros(B, S, dtype=torch.bool)
        flips_per_layer = []
        for k, gsel in sorted(sel_log.items()):
            inds = ref_out["foreground_inds"][k]
            ginds = gpu_inds[k] if gpu_inds is not None else inds
            n_layer = 0
            for b in range(B):
                a = set(inds[b][ref_out["layer_sel"][k][b]].tolist())
                g = set(ginds[b][gsel[b]].tolist())
                n_layer += len(a ^ g)
                for tok in a ^ g:
                    flipped[b, tok] = True
            flips_per_layer.append(n_layer)
        clean = per_token[~flipped]
        parity = {"max_abs": round(float(err.max()), 5), "mean_abs": round(float(err.mean()), 6),
                  "top300_selection_flips": {"tokens": int(flipped.sum()), "of": int(B * 300 * len(sel_log)),
                                             "per_layer_symmetric_difference": flips_per_layer,
                                             "note": "tokens in exactly one of (GPU, oracle) top-300 sets of some layer "
                                                     "(each side's positions mapped through its own sorted index list): "
                                                     "near-ties of the class score resolved differently under bf16"},
                  "non_flipped_tokens": {"max_abs": round(float(clean.max()), 5), "mean_abs": round(float(clean.mean()), 6),
                                         "p999_abs": round(float(clean.flatten().kthvalue(max(1, int(clean.numel() * 0.999)))[0]), 5)},
                  "note": "GPU %s output vs fp32 CPU oracle on the same batch" % args.dtype}
        # the reference's OWN bf16 mode against its fp32 run, from the committed fixture (tests/golden/
        # hotpath_autocast_digest.npz: torch.autocast("cpu", bfloat16) around the imported reference's encoder, 800x1333 +
        # 800x1066); tests/test_encoder_timed_mode_gpu.py holds the build's timed mode to it on the same inputs
        try:
            import numpy as np
            ac = np.load(os.path.join(ROOT, "tests", "golden", "hotpath_autocast_digest.npz"))
            e = ac["mixed.encoder.memory_err_non_flipped"]
            parity["reference_bf16_autocast_vs_its_fp32"] = {
                "inputs": "800x1333 + 800x1066 (fixture batch)", "top300_symmetric_difference_per_layer":
                    [int(v) for v in ac["mixed.encoder.flips_per_layer"]],
                "non_flipped_elements": {"mean_abs": round(float(e[0]), 6), "p999_abs": round(float(e[1]), 5),
                                         "max_abs": round(float(e[2]), 5)},
                "note": "elementwise statistics (the build's `non_flipped_tokens` above are per-token maxima over 256 "
                        "channels: compare through the test, which computes both sides the same way)"}
        except (OSError, KeyError, ValueError):
            pass
    return result, parity


def main():
    args = parse()
    spawn_ranks_if_needed(args)
    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started {world} rank(s); refusing to print a "
                         "line whose n_gpus is not the number of ranks that ran")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the hot path)")
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    dist = None
    backend = None
    if world > 1 or (args.force_dist_path and "RANK" in os.environ):
        # (--force-dist-path under a launcher: a one-rank RCCL group, so that a 1-GPU box runs the collectives too)
        import torch.distributed as dist
        # RCCL prints a version banner on STDOUT when its first communicator comes up; the contract is ONE JSON line
        # there -- send whatever the library writes during start-up to stderr
        sys.stdout.flush()
        saved = os.dup(1)
        os.dup2(2, 1)
        try:
            dist.init_process_group("nccl", device_id=device)
            dist.barrier()
            torch.cuda.synchronize()
        finally:
            sys.stdout.flush()
            os.dup2(saved, 1)
            os.close(saved)
        backend = dist.get_backend()
        if dist.get_world_size() != args.gpus:
            raise SystemExit("bench.py: process group size differs from --gpus")

    model = build_hot_path()
    model.load_state_dict(syn.det_state_dict(model.state_dict()))
    model = model.to(device).eval()
    if args.mode == "train":
        return train_main(args, model, device, rank, world, dist)
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    model.set_encoder_dtype(dtype, torch.float16 if (args.dtype == "bf16" and args.value_dtype == "fp16") else None)

    sizes, canvas, level_shapes, cpu_inputs, (feats, masks, pos) = make_inputs(
        args.batch, args.height, args.width, device, seed=rank)

    def step():
        with torch.no_grad():
            memory, score_maps = model(feats, masks, pos, image_sizes=sizes, canvas=canvas)
        # the salience maps are held past the step only when they are dumped: otherwise the captured graph's pool
        # reuses their buffers, as it does for every other intermediate
        return (memory, score_maps) if args.dump_outputs else (memory,)

    for _ in range(max(args.warmup, 3)):
        out = step()
    torch.cuda.synchronize()

    graphed = False
    run = step
    g = None
    main_capture = {}
    # N > 1: the process group's helper threads exist by now; thread-local capture mode keeps anything they
    # might call from invalidating this thread's capture (no collective is captured: the data path has none)
    capture_kw = {"capture_error_mode": "thread_local"} if world > 1 else {}
    if not args.no_graph:
        try:
            g, out = capture(step, capture_kw)
            main_capture = dict(CAPTURE_INFO)
            run = g.replay
            graphed = True
        except Exception as e:  # keep the eager path measurable if capture is unavailable
            sys.stderr.write(f"[bench] hipGraph capture failed, timing eager launches: {e}\n")
            torch.cuda.synchronize()
    for _ in range(3):
        run()

    def fence():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    lanes = []
    if not args.full and graphed and args.in_flight > 1 and args.dtype == "bf16":
        lanes = make_lanes(model, args, device, rank, (g, out[0], step), args.in_flight, capture_kw, sizes, canvas)
        run = lane_runner(lanes)
        for _ in range(2 * len(lanes)):
            run()

    fence()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        last = run()
    fence()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], device=device, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    ms_per_step = elapsed * 1e3 / args.steps
    images_per_s = world * args.batch * args.steps / elapsed

    if rank == 0 and args.dump_outputs:
        memory, score_maps = out if graphed else last   # (a replay refills the captured outputs)
        dump_outputs(args.dump_outputs, {"memory": memory,
                                         **{"salience_score_%d" % i: s_ for i, s_ in enumerate(score_maps)}})

    result = {
        "metric": "images/s (whole node) + ms/encoder-layer, ResNet50 800x1333",
        "value": round(images_per_s, 2), "unit": "images/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": args.dtype, "data": "synthetic", "full": args.full,
        "config": {"workload": "salience_detr_resnet50_800_1333 %s inference, batch=%d per MI355X: pyramid flatten + "
                               "hierarchical salience filtering + 6-layer salience encoder (MSDA)" % (args.dtype, args.batch),
                   "batch_per_gpu": args.batch, "global_batch": args.batch * world,
                   "image": [args.height, args.width], "levels": [list(s) for s in level_shapes],
                   "value_map_storage": ("fp16" if (args.dtype == "bf16" and args.value_dtype == "fp16") else args.dtype),
                   "parallelism": "replicas, images sharded across GPUs, no data-path collective",
                   "hipgraph": graphed, "hipgraph_nodes": main_capture.get("graph_nodes"),
                   "hipgraph_memset_nodes": main_capture.get("memset_nodes"),
                   "world_size": world, "backend": backend or "none (single process)"},
    }
    out = out[0]   # what the --full measurements below compare: `memory`

    nl = model.encoder.num_layers
    if not args.full:
        if lanes:
            result["batches_in_flight"] = len(lanes)
            result["lanes_bit_identical_to_solo"] = lanes_match_solo(lanes)
        if rank == 0:
            print(json.dumps(result))
        if dist is not None:
            dist.barrier()
            dist.destroy_process_group()
        return
    # ---- ms per encoder layer UNDER GRAPH REPLAY: graphs of the step truncated after k layers, differences ----
    layer_ms, layer_note = [None] * nl, "unavailable (eager run)"
    if graphed:
        try:
            trunc = []
            for k in range(nl + 1):
                model.encoder.max_layers = k
                gk, _ = capture(step, capture_kw)
                time_replays(gk, 3)
                trunc.append(min(time_replays(gk, 10) for _ in range(3)))
                del gk
            model.encoder.max_layers = None
            layer_ms = [trunc[k + 1] - trunc[k] for k in range(nl)]
            layer_note = ("hipGraph replay: time of the step's graph truncated after k+1 encoder layers minus after k "
                          "(min of 3 x 10 replays each); filtering + value projection + encoder entry: %.4f ms" % trunc[0])
        except Exception as e:
            model.encoder.max_layers = None
            layer_note = f"truncated-graph timing failed: {e}"

    # ---- instrumented eager pass: device time of every fused-MSDA launch (a captured graph of repeats), top-300 sets ----
    launches, launch_nq, kernels_used, msda_us, msda_us_exact = [], [], [], [], []
    real_fused = msda_mod.msda_fused_forward
    real_resident = msda_mod.msda_resident_forward
    real_bordered = msda_mod.msda_bordered_forward

    def record(call, value_hm, reference_points, proj, head_major, o, kernel):
        B, M, Nv, D = value_hm.shape
        nq = int(proj.shape[2] if head_major else proj.shape[1])
        launch_nq.append(nq)
        kernels_used.append(kernel)
        launches.append(algorithmic_bytes(B, Nv, nq, M, D, 4, 4, value_hm.element_size(), proj.element_size(),
                                          o.element_size(), reference_points.shape[-1]))
        msda_us.append(graph_time_us(call, MSDA_REPEATS))

    def timed_fused(value_hm, spatial_shapes, level_start_index, reference_points, proj, num_levels, num_points,
                    order=None, out_dtype=None, proj_head_major=False):
        call = lambda: real_fused(value_hm, spatial_shapes, level_start_index, reference_points, proj, num_levels,
                                  num_points, order=order, out_dtype=out_dtype, proj_head_major=proj_head_major)
        o = call()
        record(call, value_hm, reference_points, proj, proj_head_major, o, "msda_gather_l4p4_kernel<half_t>")
        return o

    def timed_resident(value_hm, level_shapes_, reference_points, proj_hm, out_dtype=None, chunks=0, **kw):
        call = lambda: real_resident(value_hm, level_shapes_, reference_points, proj_hm, out_dtype=out_dtype, chunks=chunks, **kw)
        o = call()
        record(call, value_hm, reference_points, proj_hm, True, o, "msda_resident_kernel<half_t>")
        return o

    def timed_bordered(value_hm, level_shapes_, reference_points, proj_hm, row_order=None, out_dtype=None, chunks=0, **kw):
        call = lambda: real_bordered(value_hm, level_shapes_, reference_points, proj_hm, row_order=row_order,
                                     out_dtype=out_dtype, chunks=chunks, **kw)
        o = call()
        # the same launch with the reference op's exact fp32 corner sums (ACC_EXACT), warm, for the A/B the line reports
        kw_exact = dict(kw, accumulate=msda_mod.ACC_EXACT)
        msda_us_exact.append(graph_time_us(lambda: real_bordered(value_hm, level_shapes_, reference_points, proj_hm,
                                                                 row_order=row_order, out_dtype=out_dtype, chunks=chunks,
                                                                 **kw_exact), MSDA_REPEATS))
        # (algorithmic bytes count the PIXELS of the maps, not the bordered layout's extra zero records)
        plain_shape = value_hm[:, :, :sum(h * w for h, w in level_shapes_)]
        record(call, plain_shape, reference_points, proj_hm, True, o,
               "msda_bordered_kernel" + ("<row order>" if row_order is not None else ""))
        return o

    sel_log = {}
    msda_mod.msda_fused_forward = timed_fused
    msda_mod.msda_resident_forward = timed_resident
    msda_mod.msda_bordered_forward = timed_bordered
    model.encoder.selection_hook = lambda k, s: sel_log.__setitem__(k, s.cpu()) or s
    gpu_inds = None
    try:
        with torch.no_grad():
            out_eager, _, aux_eager = model(feats, masks, pos, image_sizes=sizes, canvas=canvas, return_aux=True)
        # the GPU's own sorted index lists: a layer's selection is a set of POSITIONS in them.  (Until round 3 the
        # positions were mapped through the ORACLE's lists; the two orders differ wherever scores tie -- the ~700 border
        # tokens per image whose zeroed rows give identical salience scores -- which showed up as ~1400 phantom flips.)
        gpu_inds = [t.cpu() for t in aux_eager["foreground_inds"]]
        del aux_eager
        torch.cuda.synchronize()
    finally:
        msda_mod.msda_fused_forward = real_fused
        msda_mod.msda_resident_forward = real_resident
        msda_mod.msda_bordered_forward = real_bordered
        model.encoder.selection_hook = None

    bytes_per_layer = launches[:nl]
    total_bytes, warm_total_us = sum(bytes_per_layer), sum(msda_us[:nl])

    # ---- the same launches AS THEY RUN IN THE STEP: graphs of the step cut right before and right after the k-th
    # fused-MSDA launch, difference of their replay times (the launch with its cold operands -- this layer's value maps
    # were written ~0.5 ms earlier, its projection slab by the launch in front -- and one launch boundary).  This is
    # what `roofline.frac` is computed from; the warm back-to-back replay above is kept as `frac_warm`. ----
    in_step_us, in_step_note = [None] * nl, "unavailable (eager run)"
    if graphed:
        class _Cut(Exception):
            pass
        state = {"k": 0, "after": False, "n": 0}

        def cutting(real):
            def call(*a, **kw):
                if state["n"] == state["k"] and not state["after"]:
                    raise _Cut()
                o = real(*a, **kw)
                state["n"] += 1
                if state["n"] == state["k"] + 1 and state["after"]:
                    raise _Cut()
                return o
            return call

        def cut_step():
            state["n"] = 0
            try:
                with torch.no_grad():
                    model(feats, masks, pos, image_sizes=sizes, canvas=canvas)
            except _Cut:
                pass

        msda_mod.msda_fused_forward = cutting(real_fused)
        msda_mod.msda_resident_forward = cutting(real_resident)
        msda_mod.msda_bordered_forward = cutting(real_bordered)
        try:
            for k in range(nl):
                pair = []
                for after in (False, True):
                    state["k"], state["after"] = k, after
                    gk, _ = capture(cut_step, capture_kw)
                    time_replays(gk, 3)
                    pair.append(gk)
                # the two graphs take turns (clock / power state drifts between measurements that are taken minutes
                # apart: a difference of two ~1 ms numbers needs them taken under the same conditions); median of the
                # paired differences
                diffs = []
                for _ in range(CUT_PAIRS):
                    t0_ = time_replays(pair[0], CUT_REPLAYS)
                    t1_ = time_replays(pair[1], CUT_REPLAYS)
                    diffs.append(t1_ - t0_)
                diffs.sort()
                in_step_us[k] = diffs[len(diffs) // 2] * 1e3
                del pair
            in_step_note = ("hipGraph replay of the step cut right after the layer's fused-MSDA launch minus cut right "
                            "before it (the two graphs replayed in turns, %d x %d replays each, median of the paired "
                            "differences): the launch with the operands as cold as the step leaves them, one launch "
                            "boundary included" % (CUT_PAIRS, CUT_REPLAYS))
        except Exception as e:
            in_step_us, in_step_note = [None] * nl, f"cut-graph timing failed: {e}"
        finally:
            msda_mod.msda_fused_forward = real_fused
            msda_mod.msda_resident_forward = real_resident
            msda_mod.msda_bordered_forward = real_bordered
    have_in_step = all(u is not None and u > 0 for u in in_step_us)
    total_us = sum(in_step_us) if have_in_step else warm_total_us
    achieved = total_bytes / total_us / 1e3  # GB/s
    achieved_warm = total_bytes / warm_total_us / 1e3
    # HBM traffic per launch: rocprofv3 PMC passes of this same workload (benchmarks/profile_round.sh; bench.py cannot
    # run the profiler on itself), valid only for the kernel sources they were measured with -> null otherwise
    traffic, traffic_src = None, None
    tag = kernel_source_tag()
    try:
        tj = json.load(open(os.path.join(ROOT, "profiles", PROFILE_ROUND + "_msda_traffic.json")))
        nqs = launch_nq[:nl]
        if (tj.get("kernel_source_tag") == tag and args.dtype == "bf16" and args.value_dtype == tj.get("value_dtype", "same")
                and args.batch == tj["batch"] and all(str(n) in tj["per_num_query"] for n in nqs)):
            traffic = int(sum(tj["per_num_query"][str(n)]["hbm_bytes"] for n in nqs) / nl)
            traffic_src = "profiles/%s_msda_traffic.json (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes, kernel sources %s)" % (PROFILE_ROUND, tag)
        else:
            traffic_src = "null: committed PMC passes were measured on other kernel sources (%s) than these (%s)" % (
                tj.get("kernel_source_tag"), tag)
    except (OSError, ValueError, KeyError):
        traffic_src = "null: no PMC passes committed for this round"
    # the same launches by rocprofv3 (kernel-trace average over the timed loop of `bench.py --plain`, committed by
    # benchmarks/profile_round.sh with the kernel sources' tag): the steadier of the two in-step figures (the cut-graph
    # medians scatter around it by a few percent), reported next to them; null when the sources have changed since
    rocprof_us, rocprof_src = None, "null: no rocprofv3 summary committed for these kernel sources"
    try:
        rj = json.load(open(os.path.join(ROOT, "profiles", PROFILE_ROUND + "_msda_rocprof.json")))
        if rj.get("kernel_source_tag") == tag and rj.get("batch") == args.batch:
            rocprof_us = rj["avg_launch_us"]
            rocprof_src = "profiles/%s_msda_rocprof.json (%s)" % (PROFILE_ROUND, rj.get("source", "rocprofv3 --kernel-trace --stats"))
    except (OSError, ValueError, KeyError):
        pass
    # The vector-ALU side of the same launches (the counters name vector-ALU issue, not HBM, as the busiest
    # unit).  One bilinear corner of one channel is one multiply-add: B * Nq * heads * 16 samples * 4 corners * 32 channels
    # per launch.  `floor_us` = those MACs at one per SIMD lane and clock (v_fma_mix_f32 / v_fma_f32: 256 CUs x 4 SIMDs x 16
    # lanes); the packed-fp16 corner products of the 16-bit-output form (msda_resident.hip, PK) retire two per lane, so
    # the kernel's own instruction floor is lower: `instruction_floor_us` counts its FMA-class instructions (18 per
    # sample and lane for PK = 2, 24 for PK = 1, 32 for the exact form) at 4 cycles per wave instruction.
    props = torch.cuda.get_device_properties(device)
    cus = int(props.multi_processor_count)
    clk_peak = float(getattr(props, "clock_rate", 2400000)) / 1e6       # GHz
    clk_meas, clk_src = None, "null: no counter pass committed for these kernel sources"
    try:
        cj = json.load(open(os.path.join(ROOT, "profiles", PROFILE_ROUND + "_msda_clock.json")))
        if cj.get("kernel_source_tag") == tag:
            clk_meas, clk_src = cj["shader_clock_ghz"], "profiles/%s_msda_clock.json (%s)" % (PROFILE_ROUND, cj.get("source", "SQ_BUSY_CYCLES / duration"))
    except (OSError, ValueError, KeyError):
        pass
    # (the library's default accumulation form for the activation type: include/salience_hip.h SDETR_MSDA_ACC_DEFAULT)
    pk = 2 if args.dtype == "bf16" else 0
    fma_per_sample_lane = {0: 32, 1: 24, 2: 18}.get(pk, 32)
    macs = [args.batch * n * 8 * 16 * 4 * 32 for n in launch_nq[:nl]]
    lanes = cus * 4 * 16
    clk = clk_meas or clk_peak
    us_now = in_step_us if have_in_step else msda_us[:nl]
    valu = {
        "macs_per_launch": int(sum(macs) / nl), "simd_lanes": lanes, "clock_ghz": round(clk, 3),
        "clock_source": clk_src if clk_meas else "device property (peak engine clock); " + clk_src,
        "floor_us": round(sum(macs) / nl / (lanes * clk * 1e3), 2),
        "frac": round(sum(m / (lanes * clk * 1e3) for m in macs) / sum(us_now), 4),
        "per_layer_floor_us": [round(m / (lanes * clk * 1e3), 2) for m in macs],
        "corner_accumulation": {0: "exact fp32 products (v_fma_mix_f32)", 1: "packed fp16 per sample (PK = 1)",
                                2: "packed fp16 per sample and level (PK = 2)"}.get(pk),
        "instruction_floor_us": round(sum(m / 32.0 * fma_per_sample_lane for m in macs) / nl / (lanes * clk * 1e3), 2),
        "note": "MACs / (CUs x 4 SIMDs x 16 lanes x clock): the vector-ALU roofline of the gather beside the HBM one",
    }
    # the timed 16-bit form sums corners in packed fp16; the reference's op is fp32.  Both forms of the same
    # launches, warm (back to back in a graph); `frac_in_step_estimate` scales the in-step figure by the warm ratio.
    accumulate_ab = None
    if len(msda_us_exact) >= nl and warm_total_us > 0:
        ex_total = sum(msda_us_exact[:nl])
        accumulate_ab = {
            "timed_form": {0: "exact fp32 (ACC_EXACT)", 1: "packed fp16 per sample (ACC_PACKED_SAMPLE)",
                           2: "packed fp16 per sample and level (ACC_PACKED_LEVEL)"}[pk],
            "frac_warm_timed_form": round(total_bytes / warm_total_us / 1e3 / HBM_PEAK_GBPS, 4),
            "frac_warm_exact_fp32": round(total_bytes / ex_total / 1e3 / HBM_PEAK_GBPS, 4),
            "avg_launch_us_warm_exact_fp32": round(ex_total / nl, 2),
            "frac_in_step_exact_fp32_estimate": round(achieved / HBM_PEAK_GBPS * warm_total_us / ex_total, 4),
            "note": "the same six launches with the reference op's fp32 corner sums (accumulate = SDETR_MSDA_ACC_EXACT), "
                    "warm; the in-step estimate is roofline.frac x (warm time of the timed form / warm time of the exact form)",
        }
    roofline = {
        "kernel": "sdetr::" + " / ".join(sorted(set(kernels_used[:nl])))
                  + " (fused softmax + sampling locations + bilinear gather)",
        "kernel_per_layer": kernels_used[:nl],
        "bound": "hbm", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
        "frac": round(achieved / HBM_PEAK_GBPS, 4), "traffic": traffic,
        # `bound` names the roofline `frac` is taken against (the graded figure).  What the COUNTERS show as
        # the limit of this kernel is not HBM (traffic ~1.2x algorithmic at a quarter of the bandwidth): vector-ALU issue,
        # the L1's 64 B/clk/CU and the LDS each run at 50-85 % (profiles/r06_msda_pmc.md); `valu` is that roofline.
        "measured_limiter": "vector-ALU issue + L1 (64 B/clk/CU) + LDS, none saturated alone; not HBM",
        "valu": valu,
        "traffic_source": traffic_src, "kernel_source_tag": tag, "algorithmic_bytes_per_launch": int(total_bytes / nl),
        "launches_per_step": nl, "num_queries_per_layer": launch_nq[:nl], "avg_launch_us": round(total_us / nl, 2),
        "per_layer_us": [round(u, 2) for u in (in_step_us if have_in_step else msda_us[:nl])],
        "per_layer_frac": [round(b / u / 1e3 / HBM_PEAK_GBPS, 4)
                           for b, u in zip(bytes_per_layer, in_step_us if have_in_step else msda_us[:nl])],
        "per_layer_algorithmic_MB": [round(b / 1e6, 2) for b in bytes_per_layer],
        "timing": in_step_note if have_in_step else "warm replay only (see frac_warm)",
        "timing_rocprof_us": rocprof_us,
        "frac_rocprof": (round(total_bytes / nl / rocprof_us / 1e3 / HBM_PEAK_GBPS, 4) if rocprof_us else None),
        "timing_rocprof_source": rocprof_src,
        "accumulate_ab": accumulate_ab,
        "frac_warm": round(achieved_warm / HBM_PEAK_GBPS, 4), "achieved_warm": round(achieved_warm, 1),
        "avg_launch_us_warm": round(warm_total_us / nl, 2), "per_layer_us_warm": [round(u, 2) for u in msda_us[:nl]],
        "timing_warm": "per launch: %d back-to-back repetitions of the step's own launch captured in a hipGraph, replayed "
                       "between two events on the launch stream (operands hot in the XCDs' L2: NOT the step's condition)"
                       % MSDA_REPEATS,
    }

    result["ms_per_encoder_layer"] = {"mean": (round(sum(layer_ms) / nl, 4) if layer_ms[0] is not None else None),
                                      "per_layer": [None if x is None else round(x, 4) for x in layer_ms], "note": layer_note}
    result["roofline"] = roofline

    # ---- informational: the same K steps with three independent batches in flight (own inputs, graph, stream) ----
    # One batch is a dependent chain of ~76 launches, most of which fill a fraction of the 256 CUs; a server with
    # queued requests overlaps chains.  NOT the headline: `value` above is one batch at a time.
    # (bf16 only: library GEMMs of the fp32 mode must not replay side by side -- salience_detr_amd/graph_lanes.py)
    if graphed and world == 1 and args.in_flight_report > 1 and args.dtype == "bf16":
        try:
            lanes = make_lanes(model, args, device, rank, (g, out, step), args.in_flight_report, capture_kw, sizes, canvas)
            lrun = lane_runner(lanes)
            for _ in range(2 * len(lanes)):
                lrun()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                lrun()
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            result["batches_in_flight"] = {
                "lanes": len(lanes), "value": round(args.batch * args.steps / el, 2), "unit": "images/s",
                "ms_per_step": round(el * 1e3 / args.steps, 4), "outputs_bit_identical_to_solo": lanes_match_solo(lanes),
                "note": "informational, not `value`: the same %d steps with %d independent batches of %d images in "
                        "flight, each with its own inputs, hipGraph and stream" % (args.steps, len(lanes), args.batch)}
            del lanes, lrun
        except Exception as e:
            result["batches_in_flight"] = {"error": str(e)[:200]}

    # ---- configs[2] next to it: a few training steps of the same modules (fp32 forward + backward + AdamW, gradient
    # all-reduce when there are ranks), so that the run which produces this line also corroborates the training numbers
    # (`python bench.py --mode train` is the standalone form) ----
    if args.train_steps > 0:
        try:
            tmodel = build_hot_path()
            tmodel.load_state_dict(syn.det_state_dict(tmodel.state_dict()))
            tmodel = tmodel.to(device)
            tr = train_record(args, tmodel, device, rank, world, dist, args.train_steps, 2)
            result["train_step"] = {"ms_per_step": tr["ms_per_step"], "images_per_s": tr["value"], "steps": tr["steps"],
                                    "dtype": tr["dtype"], "execution": tr["config"]["execution"],
                                    "hipgraph_nodes": tr["config"].get("hipgraph_nodes"),
                                    "zero_arena": tr["config"].get("zero_arena"),
                                    "grad_bytes": tr["config"]["grad_bytes"], "msda_backward_roofline": tr["roofline"],
                                    "loss": tr["loss"], "workload": tr["config"]["workload"]}
            del tmodel
            torch.cuda.empty_cache()
        except Exception as e:
            result["train_step"] = {"error": str(e).split("\n")[0][:200]}

    # ---- the other configurations / arithmetic modes at N = 1 (sub-records; `--config-steps 0` skips them) ----
    if args.config_steps > 0 and args.dtype == "bf16":
        result["configs"] = config_records(args, device, steps=args.config_steps)

    # ---- CPU baseline: the oracle's port of the same path on the host cores (rank 0, N=1 only) ----
    if rank == 0 and world == 1 and not args.no_cpu_baseline:
        def cpu_inputs_of(batch):
            if batch == args.batch:
                return cpu_inputs
            return make_inputs(batch, args.height, args.width, "cpu", seed=rank)[3]
        result["cpu_baseline"], parity = cpu_baseline(args, model, cpu_inputs_of, out_eager, sel_log, gpu_inds)
        if parity is not None:
            result["parity_vs_cpu"] = parity

    if rank == 0:
        print(json.dumps(result))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
