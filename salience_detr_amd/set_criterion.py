"""The detector's set criterion on MI355X: ``HybridSetCriterion`` with
``HungarianMatcher`` (reference ``models/bricks/set_criterion.py``, ``models/matcher/hungarian_matcher.py``,
``models/bricks/losses.py:15-22``) and the denoising loss of ``models/detectors/base_detector.py:188-245``.

Same classes, constructor arguments, ``forward`` signatures and loss-dict keys as the reference, computed on the device
end to end (csrc/set_criterion.hip): the matching of every output of a step in one call (cost + assignment: two
launches), the losses of every output in one call (two launches), and their gradients in one ``autograd.Function``
(one launch).  No ``.cpu()``, no ``.item()``, no scipy: with targets staged once per batch (``stage_targets``) at a
fixed capacity, a step's ``forward`` + ``backward`` can be captured in a graph.

The assignment is an exact minimum-cost assignment (shortest augmenting paths, fp64 duals), so it agrees with scipy's
``linear_sum_assignment`` wherever the optimum is unique; between equally cheap assignments it may pick another one.
No CPU fallback: host tensors are rejected.
"""
import ctypes
from typing import Dict, List, NamedTuple, Optional, Sequence

import torch
import torch.distributed
from torch import Tensor, nn

from . import _hip

MAX_OUTPUTS = 16          # outputs per native call (the kernel-argument table)
STATUS_TEXT = {1: "more targets than queries", 2: "more targets than the staged capacity",
               3: "no finite assignment (NaN / inf cost)"}


class StagedTargets(NamedTuple):
    """A batch's targets on the device in the layout the kernels read: ``boxes`` f32 ``[B * capacity, 4]`` (cx, cy, w, h)
    and ``labels`` int32 ``[B * capacity]``, image b's ``counts[b]`` rows packed from ``offsets[b]``, zero padding after
    ``offsets[B]``; ``offsets`` int32 ``[B + 1]``.  ``capacity`` bounds every image's count; ``counts`` are the host-side
    counts of the batch this was staged from (``None`` where the contents were replaced on the device)."""
    boxes: Tensor
    labels: Tensor
    offsets: Tensor
    capacity: int
    counts: Optional[List[int]]

    @property
    def batch(self) -> int:
        return self.offsets.numel() - 1

    def copy_(self, other: "StagedTargets") -> "StagedTargets":
        """Overwrite these buffers with ``other``'s contents (same batch and capacity): new targets for a captured
        graph that reads these tensors.  Returns ``self`` with ``counts = other.counts``."""
        if other.batch != self.batch or other.capacity != self.capacity:
            raise RuntimeError("StagedTargets.copy_: batch and capacity must match")
        self.boxes.copy_(other.boxes)
        self.labels.copy_(other.labels)
        self.offsets.copy_(other.offsets)
        return self._replace(counts=other.counts)


def stage_targets(targets: Sequence[Dict[str, Tensor]], capacity: Optional[int] = None,
                  device=None) -> StagedTargets:
    """Host-to-device staging of ``targets[i]["boxes"]`` (cx, cy, w, h in [0, 1]) and ``targets[i]["labels"]``, done once
    per batch by the caller (the data loader's side of a training loop).  ``capacity`` defaults to the largest count of
    the batch (at least 1); a fixed capacity gives fixed shapes, so a captured step can be replayed with other targets."""
    counts = [int(t["labels"].shape[0]) for t in targets]
    for t, n in zip(targets, counts):
        if tuple(t["boxes"].shape) != (n, 4):
            raise RuntimeError(f"stage_targets: boxes {tuple(t['boxes'].shape)} do not match {n} labels")
    if not counts:
        raise RuntimeError("stage_targets: empty batch")
    cap = max(max(counts), 1) if capacity is None else int(capacity)
    if cap < 1 or max(counts) > cap:
        raise RuntimeError(f"stage_targets: capacity {cap} below the largest target count {max(counts)}")
    if device is None:
        device = targets[0]["boxes"].device
    B = len(counts)
    boxes = torch.zeros((B * cap, 4), dtype=torch.float32)
    labels = torch.zeros((B * cap,), dtype=torch.int32)
    offsets = [0]
    for t, n in zip(targets, counts):
        o = offsets[-1]
        boxes[o:o + n] = t["boxes"].detach().to("cpu", torch.float32)
        labels[o:o + n] = t["labels"].detach().to("cpu", torch.int32)
        offsets.append(o + n)
    offs = torch.tensor(offsets, dtype=torch.int32)
    return StagedTargets(boxes.to(device), labels.to(device), offs.to(device), cap, counts)


def dn_match_pattern(counts: Sequence[int], num_queries: int, denoising_groups: int, max_gt_num_per_image: int) -> Tensor:
    """Host restatement of the denoising assignment as a match table ``[B, num_queries]`` (target index or -1): query
    ``g * max_gt + t`` <-> target ``t`` (base_detector.py:205-218).  For tests and documentation."""
    match = torch.full((len(counts), num_queries), -1, dtype=torch.int32)
    for b, n in enumerate(counts):
        for g in range(denoising_groups):
            for t in range(min(n, max_gt_num_per_image)):
                match[b, g * max_gt_num_per_image + t] = t
    return match


def _check_outputs(what, logits: Sequence[Tensor], boxes: Sequence[Tensor]):
    if not logits or len(logits) != len(boxes) or len(logits) > MAX_OUTPUTS:
        raise RuntimeError(f"{what}: 1..{MAX_OUTPUTS} (logits, boxes) pairs expected")
    B, Nq, C = logits[0].shape
    for x, bx in zip(logits, boxes):
        if not isinstance(x, Tensor) or not isinstance(bx, Tensor):
            raise RuntimeError(f"{what}: logits and boxes must be tensors")
        if not x.is_cuda or not bx.is_cuda:
            raise RuntimeError(f"{what}: logits and boxes must be HIP (cuda) tensors; there is no CPU fallback")
        if x.dim() != 3 or tuple(x.shape) != (B, Nq, C):
            raise RuntimeError(f"{what}: every output's logits must be [B, Nq, C] = {(B, Nq, C)}, got {tuple(x.shape)}")
        if tuple(bx.shape) != (B, Nq, 4):
            raise RuntimeError(f"{what}: boxes must be [B, Nq, 4] = {(B, Nq, 4)}, got {tuple(bx.shape)}")
        if x.dtype != logits[0].dtype or x.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise RuntimeError(f"{what}: logits dtype {x.dtype}: float32 / bfloat16 / float16, one for all outputs")
        if bx.dtype != torch.float32:
            raise RuntimeError(f"{what}: boxes must be float32 (got {bx.dtype}); the decoder produces fp32 boxes")
    return B, Nq, C


def _rows_view(t: Tensor, inner: int) -> Tensor:
    """``t`` [B, N, inner] with contiguous rows; any batch stride is kept (a [:, :pad] query slice stays a view).  Boxes
    (inner = 4) are also read as float4: 16-byte aligned, images a multiple of 4 floats apart."""
    ok = t.stride(2) == 1 and t.stride(1) == inner
    if inner == 4:
        ok = ok and t.data_ptr() % 16 == 0 and (t.shape[0] == 1 or t.stride(0) % 4 == 0)
    return t if ok else t.contiguous()


def _output_table(logits: Sequence[Tensor], boxes: Sequence[Tensor], binary: Sequence[bool]):
    n = len(logits)
    table = (_hip.SetOutputStruct * n)()
    keep = []
    for i, (x, bx) in enumerate(zip(logits, boxes)):
        x = _rows_view(x.detach(), x.shape[2])
        bx = _rows_view(bx.detach(), 4)
        keep += [x, bx]
        B, Nq, C = x.shape
        table[i].logits = x.data_ptr()
        table[i].logits_batch_stride = x.stride(0) if B > 1 else Nq * C
        table[i].boxes = bx.data_ptr()
        table[i].boxes_batch_stride = bx.stride(0) if B > 1 else Nq * 4
        table[i].binary_cls = 1 if binary[i] else 0
    return table, keep


def _check_staged(what, staged: StagedTargets, B: int, device):
    if staged.batch != B:
        raise RuntimeError(f"{what}: staged targets hold {staged.batch} images, the outputs {B}")
    for name in ("boxes", "labels", "offsets"):
        t = getattr(staged, name)
        if not t.is_cuda or t.device != device:
            raise RuntimeError(f"{what}: staged {name} must be on {device}")


def match_outputs(logits: Sequence[Tensor], boxes: Sequence[Tensor], staged: StagedTargets, cost_class: float,
                  cost_bbox: float, cost_giou: float, focal_alpha: float, focal_gamma: float,
                  binary: Optional[Sequence[bool]] = None, with_duals: bool = False, with_cost: bool = False):
    """Hungarian matching of every (output, image) problem in one native call (cost + assignment launches).  Returns
    ``match`` int32 ``[n_outputs * B, Nq]`` (target index within the image, or -1), ``status`` int32 ``[n_outputs * B]``
    (0 = ok; see ``STATUS_TEXT``) and, when asked, the fp64 duals ``[n_outputs * B, Nq + capacity]`` (column duals, then
    row duals) and the cost ``[n_outputs * B, capacity, Nq]`` (rows past an image's count are not written).  No sync."""
    what = "set_match"
    B, Nq, C = _check_outputs(what, logits, boxes)
    dev = logits[0].device
    _check_staged(what, staged, B, dev)
    if staged.capacity > Nq:
        raise RuntimeError(f"{what}: target capacity {staged.capacity} exceeds {Nq} queries (T > Nq is not supported)")
    binary = [False] * len(logits) if binary is None else list(binary)
    L = _hip.lib(logits[0].dtype)
    table, keep = _output_table(logits, boxes, binary)
    P = len(logits) * B
    ws_bytes = int(L.sdetr_set_match_workspace_bytes(P, staged.capacity, Nq))
    ws = torch.empty(max(ws_bytes, 4), dtype=torch.uint8, device=dev)
    match = torch.empty((P, Nq), dtype=torch.int32, device=dev)
    status = torch.empty((P,), dtype=torch.int32, device=dev)
    duals = torch.empty((P, Nq + staged.capacity), dtype=torch.float64, device=dev) if with_duals else None
    _hip.launch("sdetr_set_match", L, dev, table, len(logits), _hip.dtype_code(logits[0].dtype), B, Nq, C,
                staged.boxes.data_ptr(), staged.labels.data_ptr(), staged.offsets.data_ptr(), staged.capacity,
                float(cost_class), float(cost_bbox), float(cost_giou), float(focal_alpha), float(focal_gamma), 0, 0,
                ws.data_ptr(), ws_bytes, match.data_ptr(), _hip.ptr(duals), status.data_ptr(), what=what)
    del keep
    res = [match, status]
    if with_duals:
        res.append(duals)
    if with_cost:
        res.append(ws[:ws_bytes].view(torch.float32).view(P, staged.capacity, Nq))
    return tuple(res)


def dn_match(staged: StagedTargets, num_queries: int, denoising_groups: int, max_gt_num_per_image: int,
             n_outputs: int = 1):
    """The denoising loss's assignment on the device (no cost): ``match`` int32 ``[n_outputs * B, num_queries]`` with
    query ``g * max_gt + t`` <-> target ``t`` for every output, and ``status`` (2 where an image has more targets than
    ``max_gt_num_per_image``).  One launch, no sync."""
    if not staged.offsets.is_cuda:
        raise RuntimeError("dn_match: staged targets must be on a HIP device")
    if n_outputs < 1 or n_outputs > MAX_OUTPUTS:
        raise RuntimeError(f"dn_match: 1..{MAX_OUTPUTS} outputs")
    dev = staged.offsets.device
    B = staged.batch
    L = _hip.lib()
    match = torch.empty((n_outputs * B, num_queries), dtype=torch.int32, device=dev)
    status = torch.empty((n_outputs * B,), dtype=torch.int32, device=dev)
    _hip.launch("sdetr_set_match", L, dev, None, n_outputs, _hip.F32, B, num_queries, 1, None, None,
                staged.offsets.data_ptr(), 0, 0.0, 0.0, 0.0, 0.0, 0.0, int(denoising_groups), int(max_gt_num_per_image),
                None, 0, match.data_ptr(), None, status.data_ptr(), what="dn_match")
    return match, status


class _LossSpec(NamedTuple):
    staged: StagedTargets
    match: Tensor
    num_boxes: Optional[Tensor]
    num_boxes_scale: float
    alpha: float
    gamma: float
    binary: List[bool]


class _SetLoss(torch.autograd.Function):
    """``[n_outputs, 3]`` = (loss_class, loss_bbox, loss_giou) of every output; inputs = logits_0, boxes_0, logits_1, ..."""

    @staticmethod
    def forward(ctx, spec: _LossSpec, *tensors):
        logits, boxes = list(tensors[0::2]), list(tensors[1::2])
        B, Nq, C = logits[0].shape
        dev = logits[0].device
        L = _hip.lib(logits[0].dtype)
        table, keep = _output_table(logits, boxes, spec.binary)
        n = len(logits)
        ws_bytes = int(L.sdetr_set_loss_workspace_bytes(n, B, Nq, C))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        losses = torch.empty((n, 3), dtype=torch.float32, device=dev)
        st = spec.staged
        _hip.launch("sdetr_set_loss", L, dev, table, n, _hip.dtype_code(logits[0].dtype), B, Nq, C, st.boxes.data_ptr(),
                    st.labels.data_ptr(), st.offsets.data_ptr(), spec.match.data_ptr(), _hip.ptr(spec.num_boxes),
                    float(spec.num_boxes_scale), float(spec.alpha), float(spec.gamma), ws.data_ptr(), ws_bytes,
                    losses.data_ptr())
        del keep
        ctx.spec = spec
        ctx.save_for_backward(*tensors)
        return losses

    @staticmethod
    def backward(ctx, grad_losses: Tensor):
        spec = ctx.spec
        tensors = ctx.saved_tensors
        logits, boxes = list(tensors[0::2]), list(tensors[1::2])
        B, Nq, C = logits[0].shape
        dev = logits[0].device
        n = len(logits)
        L = _hip.lib(logits[0].dtype)
        table, keep = _output_table(logits, boxes, spec.binary)
        g = grad_losses.detach().to(torch.float32).contiguous()
        gl = [torch.empty((B, Nq, C), dtype=logits[0].dtype, device=dev) for _ in range(n)]
        gb = [torch.empty((B, Nq, 4), dtype=torch.float32, device=dev) for _ in range(n)]
        gl_ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in gl])
        gb_ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in gb])
        st = spec.staged
        _hip.launch("sdetr_set_loss_backward", L, dev, table, n, _hip.dtype_code(logits[0].dtype), B, Nq, C,
                    st.boxes.data_ptr(), st.labels.data_ptr(), st.offsets.data_ptr(), spec.match.data_ptr(),
                    _hip.ptr(spec.num_boxes), float(spec.num_boxes_scale), float(spec.alpha), float(spec.gamma),
                    g.data_ptr(), gl_ptrs, gb_ptrs)
        del keep
        grads = [None]
        for a, b in zip(gl, gb):
            grads += [a, b]
        return tuple(grads)


def set_losses(logits: Sequence[Tensor], boxes: Sequence[Tensor], staged: StagedTargets, match: Tensor,
               alpha: float = 0.25, gamma: float = 2.0, num_boxes: Optional[Tensor] = None, num_boxes_scale: float = 1.0,
               binary: Optional[Sequence[bool]] = None) -> Tensor:
    """``[n_outputs, 3]`` unweighted (loss_class, loss_bbox, loss_giou) of every output for ``match`` int32
    ``[n_outputs * B, Nq]``, differentiable with respect to every logits / boxes tensor.  ``num_boxes``: a device scalar
    (float32, 1 element), or ``None`` for max(total target count, 1); the divisor is ``num_boxes * num_boxes_scale``."""
    what = "set_loss"
    B, Nq, C = _check_outputs(what, logits, boxes)
    dev = logits[0].device
    _check_staged(what, staged, B, dev)
    n = len(logits)
    if not isinstance(match, Tensor) or match.dtype != torch.int32 or tuple(match.shape) != (n * B, Nq) \
            or not match.is_cuda:
        raise RuntimeError(f"{what}: match must be a device int32 tensor [n_outputs * B, Nq] = {(n * B, Nq)}")
    if num_boxes is not None:
        if not isinstance(num_boxes, Tensor) or num_boxes.numel() != 1 or not num_boxes.is_cuda:
            raise RuntimeError(f"{what}: num_boxes must be a one-element device tensor")
        num_boxes = num_boxes.detach().to(torch.float32).reshape(1).contiguous()
    spec = _LossSpec(staged, match.contiguous(), num_boxes, float(num_boxes_scale), float(alpha), float(gamma),
                     [False] * n if binary is None else [bool(b) for b in binary])
    tensors = []
    for x, bx in zip(logits, boxes):
        tensors += [x, bx]
    return _SetLoss.apply(spec, *tensors)


def _num_boxes_tensor(staged: StagedTargets) -> Optional[Tensor]:
    """``set_criterion.py:141-147`` without ``.item()``: the all-reduced count over the world size, clamped to 1, as a
    device scalar; ``None`` (the kernels read the count themselves) outside torch.distributed."""
    if not (torch.distributed.is_available() and torch.distributed.is_initialized()):
        return None
    nb = staged.offsets[-1:].to(torch.float32)
    torch.distributed.all_reduce(nb)
    return torch.clamp(nb / torch.distributed.get_world_size(), min=1)


def _num_boxes_arg(num_boxes, device) -> Optional[Tensor]:
    if num_boxes is None:
        return None
    if isinstance(num_boxes, Tensor):
        return num_boxes.to(device=device, dtype=torch.float32).reshape(1)
    return torch.tensor([float(num_boxes)], dtype=torch.float32).to(device)


def indices_to_match(indices, batch: int, num_queries: int, device) -> Tensor:
    """The reference's per-image ``(src, tgt)`` index pairs as a match table int32 ``[batch, num_queries]``."""
    match = torch.full((batch, num_queries), -1, dtype=torch.int32, device=device)
    for b, (src, tgt) in enumerate(indices):
        if len(src):
            match[b, torch.as_tensor(src, device=device).long()] = torch.as_tensor(tgt, device=device).int()
    return match


class HungarianMatcher(nn.Module):
    """Drop-in for the reference's ``HungarianMatcher`` (same constructor).  ``forward`` matches ONE image, as the
    reference does, and returns ``(src int64 ascending, tgt int64)`` on the logits' device; sizing that result reads the
    match back to the host (one sync per call).  ``HybridSetCriterion`` calls ``match`` instead: every output and image
    of a step in one call, no sync."""

    def __init__(self, cost_class: float = 1, cost_bbox: float = 1, cost_giou: float = 1, focal_alpha: float = 0.25,
                 focal_gamma: float = 2.0, mixed_match: bool = False):
        super().__init__()
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "all costs cant be 0"
        if mixed_match:
            raise NotImplementedError("HungarianMatcher: mixed_match (Align-DETR) is not implemented")
        self.cost_class = cost_class
        self.cost_bbox = cost_bbox
        self.cost_giou = cost_giou
        self.focal_alpha = focal_alpha
        self.focal_gamma = focal_gamma
        self.mixed_match = mixed_match

    def match(self, logits: Sequence[Tensor], boxes: Sequence[Tensor], staged: StagedTargets,
              binary: Optional[Sequence[bool]] = None, **kw):
        """``match_outputs`` with this matcher's weights."""
        return match_outputs(logits, boxes, staged, self.cost_class, self.cost_bbox, self.cost_giou, self.focal_alpha,
                             self.focal_gamma, binary, **kw)

    @torch.no_grad()
    def forward(self, pred_boxes: Tensor, pred_logits: Tensor, gt_boxes: Tensor, gt_labels: Tensor, gt_copy: int = 1):
        if not pred_logits.is_cuda or not pred_boxes.is_cuda:
            raise RuntimeError("HungarianMatcher: HIP (cuda) tensors required; there is no CPU fallback")
        Nq = pred_logits.shape[0]
        T = int(gt_labels.shape[0])
        if T > Nq:
            raise RuntimeError(f"HungarianMatcher: {T} targets for {Nq} queries (T > Nq is not supported)")
        dev = pred_logits.device
        staged = stage_targets([{"boxes": gt_boxes, "labels": gt_labels}], device=dev)
        match, status = self.match([pred_logits[None]], [pred_boxes[None]], staged)[:2]
        match, status = match[0].cpu(), int(status[0])
        if status:
            raise RuntimeError(f"HungarianMatcher: {STATUS_TEXT.get(status, status)}")
        src = torch.nonzero(match >= 0).flatten()
        return src.to(dev), match[src].long().to(dev)


class HybridSetCriterion(nn.Module):
    """Drop-in for the reference's ``HybridSetCriterion`` (same constructor, ``forward`` and ``calculate_loss``
    signatures, same loss-dict keys; values unweighted as in the reference).

    ``forward(outputs, targets, staged=None)``: ``staged`` = ``stage_targets(targets, capacity)`` when the caller has
    already put the batch's targets on the device -- with a fixed capacity the call issues no host-to-device copy and
    no sync and can be captured into a graph (``targets`` is then not read).  Under torch.distributed ``num_boxes`` is
    all-reduced as a device tensor (set_criterion.py:141-147, no ``.item()``); that path has not been run on hardware.
    """

    def __init__(self, num_classes: int, matcher: nn.Module, weight_dict: Dict, alpha: float = 0.25, gamma: float = 2.0,
                 two_stage_binary_cls=False):
        super().__init__()
        self.num_classes = num_classes
        self.matcher = matcher
        self.weight_dict = weight_dict
        self.alpha = alpha
        self.gamma = gamma
        self.two_stage_binary_cls = two_stage_binary_cls

    def _stage(self, targets, staged, device) -> StagedTargets:
        if staged is not None:
            return staged
        return stage_targets(targets, device=device)

    def _losses(self, named, staged, num_boxes, num_boxes_scale=1.0, match=None):
        """named: [(suffix, outputs dict, binary)] -> {loss key + suffix: value}."""
        logits = [o["pred_logits"] for _, o, _ in named]
        boxes = [o["pred_boxes"] for _, o, _ in named]
        binary = [b for _, _, b in named]
        if match is None:
            match = self.matcher.match(logits, boxes, staged, binary)[0]
        out = set_losses(logits, boxes, staged, match, self.alpha, self.gamma, num_boxes, num_boxes_scale, binary)
        values = out.view(-1).unbind(0)
        losses = {}
        for i, (suffix, _, _) in enumerate(named):
            losses["loss_class" + suffix] = values[3 * i]
            losses["loss_bbox" + suffix] = values[3 * i + 1]
            losses["loss_giou" + suffix] = values[3 * i + 2]
        return losses

    def calculate_loss(self, outputs, targets, num_boxes, indices=None, staged=None, **kwargs):
        """One output's ``loss_class`` / ``loss_bbox`` / ``loss_giou``.  ``num_boxes``: a float (as the reference passes)
        or a device tensor.  ``indices``: the reference's per-image ``(src, tgt)`` list, or a device match table int32
        ``[B, Nq]`` (``dn_match``); ``None`` matches here."""
        dev = outputs["pred_logits"].device
        staged = self._stage(targets, staged, dev)
        match = None
        if indices is not None and len(indices):
            B, Nq = outputs["pred_logits"].shape[:2]
            match = indices if isinstance(indices, Tensor) else indices_to_match(indices, B, Nq, dev)
            match = match.to(torch.int32)
        return self._losses([("", outputs, False)], staged, _num_boxes_arg(num_boxes, dev), 1.0, match)

    def forward(self, outputs, targets, staged=None):
        dev = outputs["pred_logits"].device
        staged = self._stage(targets, staged, dev)
        if staged.counts is not None and max(staged.counts) > outputs["pred_logits"].shape[1]:
            raise RuntimeError("HybridSetCriterion: more targets than queries (T > Nq is not supported)")
        num_boxes = _num_boxes_tensor(staged)
        named = [("", {k: outputs[k] for k in ("pred_logits", "pred_boxes")}, False)]
        for i, aux in enumerate(outputs.get("aux_outputs", [])):
            named.append((f"_{i}", aux, False))
        if "enc_outputs" in outputs:
            named.append(("_enc", outputs["enc_outputs"], bool(self.two_stage_binary_cls)))
        losses = {}
        for start in range(0, len(named), MAX_OUTPUTS):
            losses.update(self._losses(named[start:start + MAX_OUTPUTS], staged, num_boxes))
        return losses

    def dn_losses(self, denoising_output, targets, denoising_groups: int, max_gt_num_per_image: int, staged=None):
        """``DNDETRDetector.compute_dn_loss`` (base_detector.py:188-245) without its host loop: ``*_dn`` for
        ``denoising_output`` and ``*_dn_{i}`` for its ``aux_outputs``, divided by ``num_boxes * denoising_groups``; the
        assignment comes from ``dn_match`` on the device."""
        dev = denoising_output["pred_logits"].device
        staged = self._stage(targets, staged, dev)
        named = [("_dn", denoising_output, False)]
        for i, aux in enumerate(denoising_output.get("aux_outputs", [])):
            named.append((f"_dn_{i}", aux, False))
        num_boxes = _num_boxes_tensor(staged)
        Nq = denoising_output["pred_logits"].shape[1]
        losses = {}
        for start in range(0, len(named), MAX_OUTPUTS):
            part = named[start:start + MAX_OUTPUTS]
            match = dn_match(staged, Nq, denoising_groups, max_gt_num_per_image, len(part))[0]
            losses.update(self._losses(part, staged, num_boxes, float(denoising_groups), match))
        return losses
