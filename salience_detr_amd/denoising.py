"""``GenerateCDNQueries`` on MI355X: the contrastive denoising queries of the training
forward (reference ``models/bricks/denoising.py:178-329``) as one launch forward and one launch backward
(csrc/denoising.hip).

Same constructor arguments, parameter name (``label_encoder.weight``) and five return values as the reference.  The
targets are read from the ``StagedTargets`` buffers the set criterion reads (``set_criterion.stage_targets``), so a step
stages its targets once; the padding slots and the attention mask are written by the same launch (no ``torch.zeros``, no
memset node), and with ``staged`` at a fixed capacity and ``max_gt_num_per_image`` pinned the call issues no
host-to-device copy and no sync and can be captured into a graph.

Noise: the reference makes four draws per repeated target (flip uniform, new label, four signs, four magnitudes).  Here
the kernel reads ONE fp32 tensor ``[2 * groups, B * capacity, 10]`` of uniforms in [0, 1) per (repeat, staged row):
column 0 flip, column 1 the new label as ``floor(u * num_classes)``, columns 2-5 the signs (``u >= 0.5`` -> +1), columns
6-9 the magnitudes.  In normal use it is one ``torch.rand`` on the device (torch owns the generator state: graph-safe,
``torch.manual_seed`` repeats it); tests inject it, ``pack_noise`` builds it from the reference's recorded draws.
No CPU fallback: host tensors are rejected.
"""
from typing import List, Optional, Sequence

import torch
from torch import Tensor, nn

from . import _hip
from .set_criterion import StagedTargets, stage_targets

NOISE_COLUMNS = 10


def denoising_groups(denoising_nums: int, max_gt: int) -> int:
    """``denoising.py:251-252``: the number of (positive, negative) groups for a batch whose largest image has
    ``max_gt`` targets."""
    return max(denoising_nums * max_gt // max(max_gt ** 2, 1), 1)


def query_mask(max_gt: int, groups: int, num_queries: int) -> Tensor:
    """Host restatement of the attention mask ``[n_dn + num_queries]^2`` (True = may not attend), for tests and
    documentation: allowed(i, j) iff ``j >= n_dn``, or ``i < n_dn`` and i, j lie in the same block of ``2 * max_gt``."""
    n_dn = 2 * groups * max_gt
    idx = torch.arange(n_dn + num_queries)
    block = idx // max(2 * max_gt, 1)
    allowed = (idx[None, :] >= n_dn) | ((idx[:, None] < n_dn) & (block[:, None] == block[None, :]))
    return ~allowed


def pack_noise(counts: Sequence[int], groups: int, num_classes: int, capacity: int, flip: Optional[Tensor] = None,
               new_label: Optional[Tensor] = None, sign: Optional[Tensor] = None, magnitude: Optional[Tensor] = None
               ) -> Tensor:
    """The reference's four recorded draws in its packed, repeat-major order -- ``flip`` ``[2G * N]`` (``rand_like``),
    ``new_label`` ``[2G * N]`` (``randint_like(0, C)``), ``sign`` ``[2G * N, 4]`` (``randint_like(0, 2)``), ``magnitude``
    ``[2G * N, 4]`` (``rand_like``), N = the batch's target count -- as the noise tensor ``[2G, B * capacity, 10]`` of the
    kernel (host tensor): labels as ``(r + 0.5) / C``, signs as 0.25 / 0.75, the two uniforms verbatim.  A draw the
    reference did not make (``label_noise_prob == 0`` / ``box_noise_scale == 0``) may be ``None`` (zeros)."""
    n, reps = sum(counts), 2 * groups
    noise = torch.zeros((reps, len(counts) * capacity, NOISE_COLUMNS), dtype=torch.float32)
    if n == 0:
        return noise
    if flip is not None:
        noise[:, :n, 0] = torch.as_tensor(flip, dtype=torch.float32).reshape(reps, n)
    if new_label is not None:
        noise[:, :n, 1] = (torch.as_tensor(new_label).reshape(reps, n).to(torch.float64) + 0.5).div(num_classes).float()
    if sign is not None:
        noise[:, :n, 2:6] = torch.as_tensor(sign, dtype=torch.float32).reshape(reps, n, 4) * 0.5 + 0.25
    if magnitude is not None:
        noise[:, :n, 6:10] = torch.as_tensor(magnitude, dtype=torch.float32).reshape(reps, n, 4)
    return noise


def unpack_noise(noise: Tensor, counts: Sequence[int], num_classes: int):
    """Inverse of ``pack_noise`` as the kernel reads the tensor: ``(flip, new_label, sign, magnitude)`` in packed order."""
    n = sum(counts)
    part = noise[:, :n]
    new_label = torch.clamp((part[..., 1] * num_classes).floor().long(), max=num_classes - 1)
    sign = (part[..., 2:6] >= 0.5).float()
    return part[..., 0].reshape(-1), new_label.reshape(-1), sign.reshape(-1, 4), part[..., 6:10].reshape(-1, 4)


class _CdnQueries(torch.autograd.Function):
    """(label queries, box queries, noised labels, attention mask) of one launch; d ``weight`` of one launch."""

    @staticmethod
    def forward(ctx, weight: Tensor, staged: StagedTargets, noise: Optional[Tensor], max_gt: int, groups: int,
                num_queries: int, label_noise_prob: float, box_noise_scale: float):
        B, (C, E) = staged.batch, weight.shape
        dev = weight.device
        n_dn = 2 * groups * max_gt
        total = n_dn + num_queries
        label_q = torch.empty((B, n_dn, E), dtype=torch.float32, device=dev)
        box_q = torch.empty((B, n_dn, 4), dtype=torch.float32, device=dev)
        labels = torch.empty((B, n_dn), dtype=torch.int32, device=dev)
        mask = torch.empty((total, total), dtype=torch.bool, device=dev)
        w = weight.detach()
        lib = _hip.lib()
        _hip.launch("sdetr_cdn_queries", lib, dev, staged.boxes.data_ptr(), staged.labels.data_ptr(),
                    staged.offsets.data_ptr(), staged.capacity, w.data_ptr(), _hip.ptr(noise), B, max_gt, groups, C, E,
                    num_queries, float(label_noise_prob), float(box_noise_scale), label_q.data_ptr(), box_q.data_ptr(),
                    labels.data_ptr(), mask.data_ptr(), what="GenerateCDNQueries")
        ctx.save_for_backward(labels)
        ctx.num_classes = C
        ctx.mark_non_differentiable(box_q, labels, mask)
        ctx.set_materialize_grads(False)      # no zero-fill launches for the three outputs that carry no gradient
        return label_q, box_q, labels, mask

    @staticmethod
    def backward(ctx, grad_label_q, _grad_box, _grad_labels, _grad_mask):
        if grad_label_q is None:
            return (None,) * 8
        (labels,) = ctx.saved_tensors
        B, n_dn = labels.shape
        g = grad_label_q.detach().to(torch.float32).contiguous()
        E = g.shape[-1]
        grad_w = torch.empty((ctx.num_classes, E), dtype=torch.float32, device=g.device)
        lib = _hip.lib()
        _hip.launch("sdetr_cdn_label_grad", lib, g.device, g.data_ptr(), labels.data_ptr(), B, n_dn, ctx.num_classes, E,
                    grad_w.data_ptr(), what="GenerateCDNQueries (backward)")
        return grad_w, None, None, None, None, None, None, None


class GenerateCDNQueries(nn.Module):
    """Drop-in for the reference's ``GenerateCDNQueries`` (module docstring)."""

    def __init__(self, num_queries: int = 300, num_classes: int = 80, label_embed_dim: int = 256,
                 denoising_nums: int = 100, label_noise_prob: float = 0.5, box_noise_scale: float = 1.0):
        super().__init__()
        self.num_queries = num_queries
        self.num_classes = num_classes
        self.label_embed_dim = label_embed_dim
        self.denoising_nums = denoising_nums
        self.label_noise_prob = label_noise_prob
        self.box_noise_scale = box_noise_scale
        self.denoising_groups = 1
        self.label_encoder = nn.Embedding(num_classes, label_embed_dim)
        self.last_noised_labels = None      # int32 [B, n_dn], -1 on padding slots: for inspection / tests

    def noise_shape(self, batch: int, capacity: int, groups: int):
        return (2 * groups, batch * capacity, NOISE_COLUMNS)

    def forward(self, gt_labels_list: Sequence[Tensor], gt_boxes_list: Sequence[Tensor],
                staged: Optional[StagedTargets] = None, noise: Optional[Tensor] = None,
                max_gt_num_per_image: Optional[int] = None):
        """``gt_labels_list[i]`` ``[n_i]``, ``gt_boxes_list[i]`` ``[n_i, 4]`` (cx, cy, w, h in [0, 1]); ``staged`` = the
        batch's ``stage_targets(...)`` when the caller has it (the lists then only give the counts, and not even those
        when ``max_gt_num_per_image`` is pinned).  Returns ``(noised_label_queries [B, n_dn, E], noised_box_queries
        [B, n_dn, 4], attn_mask, denoising_groups, 2 * max_gt)`` with ``n_dn = 2 * denoising_groups * max_gt``."""
        weight = self.label_encoder.weight
        if not weight.is_cuda:
            raise RuntimeError("GenerateCDNQueries: HIP (cuda) tensors required; there is no CPU fallback")
        if weight.dtype != torch.float32 or not weight.is_contiguous():
            raise RuntimeError("GenerateCDNQueries: label_encoder.weight must be contiguous float32")
        dev = weight.device
        for i, labels in enumerate(gt_labels_list or ()):
            # labels still on the host are checked there (no sync): the reference's nn.Embedding raises on such a label,
            # the kernel can only skip it (it writes the slot as padding to stay inside the table)
            if torch.is_tensor(labels) and not labels.is_cuda and labels.numel() and \
                    (int(labels.min()) < 0 or int(labels.max()) >= self.num_classes):
                raise RuntimeError(f"GenerateCDNQueries: a label of image {i} lies outside [0, {self.num_classes})")
        if staged is None:
            if len(gt_labels_list) != len(gt_boxes_list):
                raise RuntimeError("GenerateCDNQueries: one box list per label list expected")
            staged = stage_targets([{"labels": l, "boxes": b} for l, b in zip(gt_labels_list, gt_boxes_list)], device=dev)
        for name in ("boxes", "labels", "offsets"):
            t = getattr(staged, name)
            if not t.is_cuda or t.device != dev:
                raise RuntimeError(f"GenerateCDNQueries: staged {name} must be on {dev}; there is no CPU fallback")
        counts = staged.counts if staged.counts is not None else \
            ([int(l.shape[0]) for l in gt_labels_list] if gt_labels_list is not None else None)
        if max_gt_num_per_image is not None:
            max_gt = int(max_gt_num_per_image)
            if counts is not None and max(counts) > max_gt:
                raise RuntimeError(f"GenerateCDNQueries: max_gt_num_per_image = {max_gt} is below the largest target "
                                   f"count {max(counts)}")
        elif counts is not None:
            max_gt = max(counts)
        else:
            raise RuntimeError("GenerateCDNQueries: target counts unknown (staged on the device): pass max_gt_num_per_image")
        if max_gt > staged.capacity:
            raise RuntimeError(f"GenerateCDNQueries: max_gt = {max_gt} exceeds the staged capacity {staged.capacity}")
        groups = denoising_groups(self.denoising_nums, max_gt)
        self.denoising_groups = groups
        B, E = staged.batch, self.label_embed_dim
        if max_gt == 0:     # no targets in the batch: nothing to launch (the reference returns the same empties)
            self.last_noised_labels = torch.empty((B, 0), dtype=torch.int32, device=dev)
            mask = torch.empty((self.num_queries, self.num_queries), dtype=torch.bool, device=dev).fill_(False)
            return weight.new_empty((B, 0, E)), weight.new_empty((B, 0, 4)), mask, groups, 0
        needs_noise = self.label_noise_prob > 0 or self.box_noise_scale > 0
        shape = self.noise_shape(B, staged.capacity, groups)
        if noise is None:
            if needs_noise:
                noise = torch.rand(shape, dtype=torch.float32, device=dev)
        else:
            if not noise.is_cuda or noise.device != dev:
                raise RuntimeError("GenerateCDNQueries: noise must be a HIP (cuda) tensor; there is no CPU fallback")
            if tuple(noise.shape) != shape or noise.dtype != torch.float32:
                raise RuntimeError(f"GenerateCDNQueries: noise must be float32 {shape}, got {noise.dtype} "
                                   f"{tuple(noise.shape)}")
            noise = noise.contiguous()
        label_q, box_q, labels, mask = _CdnQueries.apply(weight, staged, noise, max_gt, groups, self.num_queries,
                                                         self.label_noise_prob, self.box_noise_scale)
        self.last_noised_labels = labels
        return label_q, box_q, mask, groups, max_gt * 2
