"""The reference detector (``models/detectors/salience_detr.py:120-243``): the eval path from backbone features or from
images, and -- for a detector built with a ``criterion`` -- the training forward that returns the weighted loss dict.

``SalienceDETRHead`` holds ``neck`` (``ChannelMapper``), ``position_embedding`` (``PositionEmbeddingSine``), ``transformer``
(``SalienceTransformer``) and ``postprocessor`` (``PostProcess``) under the reference's attribute names, so a reference
``SalienceDETR`` state dict loads once its ``backbone.*``, ``denoising_generator.*`` and ``_classes_`` entries are removed
(``head_state_dict``).  ``forward(backbone_feats, mask, original_image_sizes)`` runs neck -> per-level masks and positions
(one launch) -> transformer -> post-processing and returns ``PostProcess``'s list of dicts.

``SalienceDETR`` is the whole eval detector from images: the same four parts plus ``backbone`` (``ResNetBackbone``), so a
reference ``SalienceDETR`` state dict loads once its ``denoising_generator.*`` and ``_classes_`` entries are removed
(``detector_state_dict``).  ``forward(images)`` runs image batching (one launch: ``ConvertImageDtype`` + ``Normalize`` +
padding to a multiple of 32 + the padding mask) -> backbone -> the head above, handing the transformer the image sizes
and the canvas so that its token budgets come from the host.  (The transformer's proposal stage still reads its kept
count on the host, so the whole detector does not capture into one graph; batching + backbone do.)

``SalienceDETR(..., min_size=, max_size=)`` (the reference constructor's keywords and rule, base_detector.py:57-75: the
transform exists when at least one is a number, with ``min(size)``, ``max(size)``) puts the reference's ``EvalResize`` in
front of the eval path, fused into the batching launch (``batch_images(images, resize=...)``): the canvas and the
transformer's token budgets come from the RESIZED sizes, ``PostProcess`` gets the sizes BEFORE the resize, so the boxes
are in the original image's pixels (salience_detr.py:165).  Training mode ignores it, as the reference does (its
training images are resized by the dataset transforms).  ``EvalResize`` has no parameters or buffers: state dicts are
the same with and without it, and a detector built without the keywords has today's module tree and path.

Training (``criterion=`` given, ``train()`` mode, ``forward(images, targets)``; salience_detr.py:163-240,
base_detector.py:156-261): images are batched WITHOUT the eval transform (they arrive normalised from the dataset
transforms), the targets' boxes go from xyxy pixels to cxcywh normalised by each image's own size (``prepare_targets``)
and are staged on the device ONCE (``set_criterion.stage_targets``); the same ``StagedTargets`` feed the denoising
generator (``denoising.GenerateCDNQueries``, held as ``denoising_generator`` so a reference state dict loads with only
``_classes_`` removed: ``train_state_dict``), the set criterion, the denoising loss and -- as absolute boxes -- the
salience criterion.  The first ``n_dn`` queries of every decoder layer are split off as the denoising output
(``dn_post_process``); the result is ``{k: loss[k] * weight_dict[k]}`` as in the reference.  A detector built without
``criterion`` has exactly the module tree and state-dict keys of the eval detector.  ``forward_batch(batch)`` is the same
training forward from the canvas ``train_transform.TrainTransform`` builds out of decoded images (the dataset transform
in one launch), without batching the images again.
"""
from typing import Dict, List, Optional, Sequence, Tuple, Union

import torch
from torch import Tensor, nn

from .backbone import batch_images
from .position_encoding import level_masks_and_positions
from .set_criterion import StagedTargets, stage_targets


def head_state_dict(detector_state: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """A reference ``SalienceDETR`` state dict without the entries this head has no holder for: ``backbone.*``,
    ``denoising_generator.*`` and the ``_classes_`` buffer (the encoded class names the reference's training script
    registers on the model before saving it, ``main.py:138-141``)."""
    return {k: v for k, v in detector_state.items()
            if not k.startswith(("backbone.", "denoising_generator.")) and k != "_classes_"}


def train_state_dict(detector_state: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """A reference ``SalienceDETR`` state dict for a ``SalienceDETR`` built with ``criterion`` (it holds
    ``denoising_generator``): only the ``_classes_`` buffer is removed."""
    return {k: v for k, v in detector_state.items() if k != "_classes_"}


def prepare_targets(targets: Sequence[Dict[str, Tensor]], image_sizes: Sequence[Sequence[int]]) -> List[Dict[str, Tensor]]:
    """``DETRDetector.prepare_targets`` + ``check_boxes`` (base_detector.py:100-112, 156-166): ``boxes`` from
    ``(x0, y0, x1, y1)`` pixels to ``(cx, cy, w, h)`` divided by the image's own ``(w, h, w, h)``; the inputs are not
    modified.  Degenerate boxes are rejected -- on the host, without a device sync, when the targets are host tensors
    (device tensors pay one sync for the check, as the reference does)."""
    out = []
    for i, (t, (h, w)) in enumerate(zip(targets, image_sizes)):
        boxes = t["boxes"]
        if boxes.dim() != 2 or boxes.shape[-1] != 4:
            raise RuntimeError(f"prepare_targets: boxes of target {i} must be [n, 4], got {tuple(boxes.shape)}")
        bad = (boxes[:, 2:] <= boxes[:, :2]).any(dim=1)
        if bool(bad.any()):
            first = int(torch.nonzero(bad)[0, 0])
            raise RuntimeError("All bounding boxes should have positive height and width."
                               f" Found invalid box {boxes[first].tolist()} for target at index {i}.")
        x0, y0, x1, y1 = boxes.unbind(-1)
        cxcywh = torch.stack(((x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0), -1)
        new = dict(t)
        new["boxes"] = cxcywh / cxcywh.new_tensor([w, h, w, h])
        out.append(new)
    return out


def split_denoising(outputs_class: Tensor, outputs_coord: Tensor, n_dn: int, aux_loss: bool = True):
    """``DNDETRDetector.dn_post_process`` (base_detector.py:246-261): the first ``n_dn`` queries of every decoder layer as
    the denoising output dict, the rest as the matching part ``(outputs_class, outputs_coord)``."""
    known_class, known_coord = outputs_class[:, :, :n_dn, :], outputs_coord[:, :, :n_dn, :]
    out = {"pred_logits": known_class[-1], "pred_boxes": known_coord[-1]}
    if aux_loss:
        out["aux_outputs"] = [{"pred_logits": a, "pred_boxes": b} for a, b in zip(known_class[:-1], known_coord[:-1])]
    return out, outputs_class[:, :, n_dn:, :], outputs_coord[:, :, n_dn:, :]


class SalienceDETRHead(nn.Module):
    def __init__(self, neck: nn.Module, position_embedding: nn.Module, transformer: nn.Module, postprocessor: nn.Module,
                 criterion: Optional[nn.Module] = None, focus_criterion: Optional[nn.Module] = None, num_classes: int = 91,
                 num_queries: int = 900, denoising_nums: int = 100, aux_loss: bool = True):
        super().__init__()
        self.neck = neck
        self.position_embedding = position_embedding
        self.transformer = transformer
        self.postprocessor = postprocessor
        self.num_classes = num_classes
        self.aux_loss = aux_loss
        # the training parts exist only in a detector built for training: without `criterion` the module tree and the
        # state-dict keys are the eval detector's
        self.criterion = criterion
        self.focus_criterion = focus_criterion
        if criterion is not None:
            from .denoising import GenerateCDNQueries
            self.denoising_generator = GenerateCDNQueries(num_queries=num_queries, num_classes=num_classes,
                                                          label_embed_dim=transformer.embed_dim,
                                                          denoising_nums=denoising_nums, label_noise_prob=0.5,
                                                          box_noise_scale=1.0)

    def set_dtype(self, dtype: torch.dtype):
        for part in (self.neck, self.position_embedding, self.transformer):
            if hasattr(part, "set_dtype"):
                part.set_dtype(dtype)
        return self

    def inputs(self, backbone_feats: Union[Dict[str, Tensor], Sequence[Tensor]],
               mask: Tensor) -> Tuple[List[Tensor], List[Tensor], List[Tensor]]:
        """The transformer's three inputs: neck features, per-level masks, per-level positions."""
        feats = self.neck(backbone_feats)
        masks, pos = level_masks_and_positions(mask, [tuple(f.shape[-2:]) for f in feats], self.position_embedding)
        return feats, masks, pos

    def _wants_training(self, targets) -> bool:
        if not (self.training and self.criterion is not None):
            return False
        if targets is None:
            raise RuntimeError(f"{type(self).__name__}: training mode needs targets (a list of dicts with 'boxes' and "
                               "'labels', one per image); call eval() for detections")
        return True

    def forward_train(self, backbone_feats: Union[Dict[str, Tensor], Sequence[Tensor]], mask: Tensor,
                      targets: Sequence[Dict[str, Tensor]], image_sizes: Sequence[Sequence[int]],
                      canvas: Optional[Tuple[int, int]] = None, noise: Optional[Tensor] = None,
                      staged: Optional[StagedTargets] = None,
                      focus_boxes: Optional[Tuple[Tensor, Tensor]] = None) -> Dict[str, Tensor]:
        """The training half of the reference's forward (salience_detr.py:170-240) from backbone features.  ``targets``:
        prepared (``prepare_targets``: cxcywh in [0, 1]); ``image_sizes``: (h, w) of every image before padding;
        ``canvas``: the padded (H, W), default ``mask.shape[-2:]``; ``noise``: the generator's noise tensor (tests);
        ``staged``: the batch's ``stage_targets(...)`` when the caller already has it; ``focus_boxes``: the salience
        criterion's ``stage_boxes(targets, image_sizes, device)`` likewise (with both, the call makes no host-to-device
        copy: a captured step)."""
        if self.criterion is None:
            raise RuntimeError(f"{type(self).__name__}: built without a criterion; there is no training forward")
        if len(targets) != mask.shape[0] or len(image_sizes) != mask.shape[0]:
            raise RuntimeError(f"{type(self).__name__}: one target dict and one image size per image expected")
        canvas = tuple(int(v) for v in (canvas if canvas is not None else mask.shape[-2:]))
        image_sizes = [[int(h), int(w)] for h, w in image_sizes]
        feats, masks, pos = self.inputs(backbone_feats, mask)
        dev = feats[0].device
        if staged is None:
            staged = stage_targets(targets, device=dev)       # the step's one host-to-device copy of the targets
        gen = self.denoising_generator
        label_q, box_q, attn_mask, groups, twice_max_gt = gen([t["labels"] for t in targets],
                                                              [t["boxes"] for t in targets], staged=staged, noise=noise)
        outputs_class, outputs_coord, enc_class, enc_coord, foreground_mask = self.transformer(
            feats, masks, pos, label_q, box_q, attn_mask=attn_mask, image_sizes=image_sizes, canvas=canvas)
        # salience_detr.py:205: the embedding always takes part in the graph (DDP, batches without targets)
        outputs_class[0] += gen.label_encoder.weight[0, 0] * 0.0
        n_dn = groups * twice_max_gt
        denoising_output, outputs_class, outputs_coord = split_denoising(outputs_class, outputs_coord, n_dn, self.aux_loss)
        output = {"pred_logits": outputs_class[-1], "pred_boxes": outputs_coord[-1]}
        if self.aux_loss:
            output["aux_outputs"] = [{"pred_logits": a, "pred_boxes": b}
                                     for a, b in zip(outputs_class[:-1], outputs_coord[:-1])]
        output["enc_outputs"] = {"pred_logits": enc_class, "pred_boxes": enc_coord}
        loss_dict = self.criterion(output, targets, staged=staged)
        if n_dn > 0:
            loss_dict.update(self.criterion.dn_losses(denoising_output, targets, groups, twice_max_gt, staged=staged))
        else:   # no targets in the batch: the reference's denoising losses are sums over nothing
            zero = enc_coord.new_zeros(())
            for suffix in ["_dn"] + [f"_dn_{i}" for i in range(len(denoising_output.get("aux_outputs", [])))]:
                loss_dict.update({k + suffix: zero for k in ("loss_class", "loss_bbox", "loss_giou")})
        if self.focus_criterion is not None:
            feature_stride = [(canvas[0] / f.shape[-2], canvas[1] / f.shape[-1]) for f in feats]
            boxes = focus_boxes if focus_boxes is not None else self.focus_criterion.stage_boxes(
                [{"boxes": staged.boxes[o:o + n]} for o, n in self._staged_slices(staged, targets)],
                image_sizes, dev)
            loss_dict.update(self.focus_criterion(foreground_mask, targets, feature_stride, image_sizes, staged=boxes))
        weight_dict = self.criterion.weight_dict
        return {k: loss_dict[k] * weight_dict[k] for k in loss_dict.keys() if k in weight_dict}

    @staticmethod
    def _staged_slices(staged: StagedTargets, targets) -> List[Tuple[int, int]]:
        """(first row, count) of every image in the staged buffers, from the host-side counts."""
        counts = staged.counts if staged.counts is not None else [int(t["labels"].shape[0]) for t in targets]
        out, o = [], 0
        for n in counts:
            out.append((o, n))
            o += n
        return out

    def forward(self, backbone_feats: Union[Dict[str, Tensor], Sequence[Tensor]], mask: Tensor,
                original_image_sizes: Union[Tensor, Sequence[Sequence[int]]], image_sizes=None, canvas=None,
                targets=None, noise=None):
        """``mask`` ``[B, H, W]`` True on padding (the padded canvas of the backbone's input); ``original_image_sizes``
        ``[B, 2]`` (h, w) per image.  ``image_sizes`` / ``canvas`` go to the transformer when given.  In training mode
        (a head built with ``criterion``) ``targets`` (prepared, see ``forward_train``) are required and the weighted
        loss dict is returned; otherwise the detections, under ``no_grad``.  A head built WITHOUT ``criterion`` has no
        training branch: it returns detections under ``no_grad`` in ``train()`` mode too, and ignores ``targets``."""
        if self._wants_training(targets):
            if image_sizes is None:
                image_sizes = original_image_sizes.tolist() if torch.is_tensor(original_image_sizes) else original_image_sizes
            return self.forward_train(backbone_feats, mask, targets, image_sizes, canvas, noise=noise)
        with torch.no_grad():
            return self._detect(backbone_feats, mask, original_image_sizes, image_sizes, canvas)

    def _detect(self, backbone_feats, mask, original_image_sizes, image_sizes=None, canvas=None) -> List[Dict[str, Tensor]]:
        feats, masks, pos = self.inputs(backbone_feats, mask)
        kwargs = {}
        if image_sizes is not None:
            kwargs["image_sizes"] = image_sizes
        if canvas is not None:
            kwargs["canvas"] = canvas
        outputs_class, outputs_coord = self.transformer(feats, masks, pos, **kwargs)[:2]
        output = {"pred_logits": outputs_class[-1], "pred_boxes": outputs_coord[-1]}
        if not torch.is_tensor(original_image_sizes):
            original_image_sizes = torch.tensor([[int(h), int(w)] for h, w in original_image_sizes],
                                                device=outputs_class.device)
        return self.postprocessor(output, original_image_sizes)


def detector_state_dict(detector_state: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """A reference ``SalienceDETR`` state dict without the entries ``SalienceDETR`` has no holder for:
    ``denoising_generator.*`` (training only) and the ``_classes_`` buffer."""
    return {k: v for k, v in detector_state.items() if not k.startswith("denoising_generator.") and k != "_classes_"}


class SalienceDETR(SalienceDETRHead):
    """The eval detector from images (module docstring): ``backbone`` + the ``SalienceDETRHead`` parts."""

    def __init__(self, backbone: nn.Module, neck: nn.Module, position_embedding: nn.Module, transformer: nn.Module,
                 postprocessor: nn.Module, criterion: Optional[nn.Module] = None,
                 focus_criterion: Optional[nn.Module] = None, num_classes: int = 91, num_queries: int = 900,
                 denoising_nums: int = 100, aux_loss: bool = True, min_size: Optional[int] = None,
                 max_size: Optional[int] = None):
        super().__init__(neck, position_embedding, transformer, postprocessor, criterion=criterion,
                         focus_criterion=focus_criterion, num_classes=num_classes, num_queries=num_queries,
                         denoising_nums=denoising_nums, aux_loss=aux_loss)
        self.backbone = backbone
        self._sizes_cache = {}
        # base_detector.py:68-72: the resize exists when at least one of the two is a number
        size = [s for s in (min_size, max_size) if isinstance(s, (int, float)) and not isinstance(s, bool)]
        if len(size) != 0:
            from .eval_resize import EvalResize
            self.eval_resize = EvalResize(min(size), max(size), antialias=True)

    def set_dtype(self, dtype: torch.dtype):
        if hasattr(self.backbone, "set_dtype"):
            self.backbone.set_dtype(dtype)
        return super().set_dtype(dtype)

    def forward(self, images: Sequence[Tensor], targets: Optional[Sequence[Dict[str, Tensor]]] = None, noise=None):
        """``images``: ``[3, h_i, w_i]`` each; in eval mode of any size when the detector was built with ``min_size`` /
        ``max_size`` (they are resized in the batching launch and the boxes come back in the original pixels), otherwise
        already at model size.  Eval mode (or a detector built
        without ``criterion``): float in [0, 1] or uint8, returns the detections under ``no_grad``.  Training mode:
        float32, already normalised by the dataset transforms; ``targets[i]`` = ``{"boxes": [n, 4] xyxy pixels of image
        i, "labels": [n]}``, required (``None`` raises); returns the weighted loss dict.  A detector built without
        ``criterion`` takes the eval path under ``no_grad`` in ``train()`` mode too and ignores ``targets``.  ``noise``: the denoising generator's noise (tests).
        The backbone's backward goes through ``F.conv2d`` unless ``self.backbone.set_train_form("hip")`` was called
        (``ResNetBackbone``: its own backward-data / backward-weight kernels)."""
        if torch.is_tensor(images):
            images = list(images.unbind(0))
        sizes = tuple((int(i.shape[-2]), int(i.shape[-1])) for i in images)
        if self._wants_training(targets):
            if len(targets) != len(images):
                raise RuntimeError("SalienceDETR: one target dict per image expected")
            with torch.no_grad():
                canvas, mask = batch_images(images, normalize=False)
            prepared = prepare_targets(targets, sizes)
            return self.forward_train(self.backbone(canvas), mask, prepared, sizes, tuple(canvas.shape[-2:]), noise=noise)
        with torch.no_grad():
            return self._detect_images(images, sizes)

    def forward_batch(self, batch, noise=None) -> Dict[str, Tensor]:
        """The training forward from a ready canvas: ``batch`` is ``train_transform.TrainBatch`` (``TrainTransform``'s
        result: the normalised padded canvas, the padding mask, the transformed image sizes and targets), so the images
        are not batched again: ``prepare_targets`` -> backbone -> ``forward_train``.  Returns the weighted loss dict, the
        one ``forward(images, targets)`` gives for the images inside the canvas.  Training only: a detector built
        without ``criterion``, eval mode and a batch without targets raise."""
        if self.criterion is None:
            raise RuntimeError(f"{type(self).__name__}: built without a criterion; there is no training forward")
        if not self.training:
            raise RuntimeError(f"{type(self).__name__}: forward_batch is the training forward; call train() first "
                               "(eval() detections come from forward(images))")
        self._wants_training(batch.targets)
        sizes = tuple((int(h), int(w)) for h, w in batch.image_sizes)
        if len(batch.targets) != len(sizes) or batch.canvas.shape[0] != len(sizes):
            raise RuntimeError("SalienceDETR: one target dict per image expected")
        prepared = prepare_targets(batch.targets, sizes)
        return self.forward_train(self.backbone(batch.canvas), batch.mask, prepared, sizes,
                                  tuple(batch.canvas.shape[-2:]), noise=noise)

    def _detect_images(self, images, sizes) -> List[Dict[str, Tensor]]:
        key = (sizes, images[0].device)
        if self._sizes_cache.get("key") != key:   # one host-to-device copy per distinct batch of sizes
            self._sizes_cache = {"key": key, "value": torch.tensor(sizes, device=images[0].device)}
        original_image_sizes = self._sizes_cache["value"]
        resize = getattr(self, "eval_resize", None)
        if resize is None:
            canvas, mask = batch_images(images)
        else:   # boxes in the ORIGINAL pixels (sizes before the resize), token budgets from the RESIZED sizes
            canvas, mask = batch_images(images, resize=(resize.min_size, resize.max_size))
            sizes = tuple(resize.output_size(h, w) for h, w in sizes)
        # the image sizes and the canvas give the transformer its token budgets on the host (one device sync fewer)
        return self._detect(self.backbone(canvas), mask, original_image_sizes, image_sizes=[list(s) for s in sizes],
                            canvas=tuple(canvas.shape[-2:]))
