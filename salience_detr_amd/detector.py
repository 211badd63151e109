"""The reference detector after its backbone, in eval mode (``models/detectors/salience_detr.py:158-243`` without
``self.backbone``, the pre-processing and the training branch).

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
count on the host, so the whole detector does not capture into one graph; batching + backbone do.)  Out of scope: ``EvalResize`` (images
arrive already at model size, the training path's contract), the denoising generator and the training branch.
"""
from typing import Dict, List, Sequence, Tuple, Union

import torch
from torch import Tensor, nn

from .backbone import batch_images
from .position_encoding import level_masks_and_positions


def head_state_dict(detector_state: Dict[str, Tensor]) -> Dict[str, Tensor]:
    """A reference ``SalienceDETR`` state dict without the entries this head has no holder for: ``backbone.*``,
    ``denoising_generator.*`` and the ``_classes_`` buffer (the encoded class names the reference's training script
    registers on the model before saving it, ``main.py:138-141``)."""
    return {k: v for k, v in detector_state.items()
            if not k.startswith(("backbone.", "denoising_generator.")) and k != "_classes_"}


class SalienceDETRHead(nn.Module):
    def __init__(self, neck: nn.Module, position_embedding: nn.Module, transformer: nn.Module, postprocessor: nn.Module):
        super().__init__()
        self.neck = neck
        self.position_embedding = position_embedding
        self.transformer = transformer
        self.postprocessor = postprocessor

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

    @torch.no_grad()
    def forward(self, backbone_feats: Union[Dict[str, Tensor], Sequence[Tensor]], mask: Tensor,
                original_image_sizes: Union[Tensor, Sequence[Sequence[int]]], image_sizes=None, canvas=None
                ) -> List[Dict[str, Tensor]]:
        """``mask`` ``[B, H, W]`` True on padding (the padded canvas of the backbone's input); ``original_image_sizes``
        ``[B, 2]`` (h, w) per image.  ``image_sizes`` / ``canvas`` go to the transformer when given."""
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
                 postprocessor: nn.Module):
        super().__init__(neck, position_embedding, transformer, postprocessor)
        self.backbone = backbone
        self._sizes_cache = {}

    def set_dtype(self, dtype: torch.dtype):
        if hasattr(self.backbone, "set_dtype"):
            self.backbone.set_dtype(dtype)
        return super().set_dtype(dtype)

    @torch.no_grad()
    def forward(self, images: Sequence[Tensor]) -> List[Dict[str, Tensor]]:
        """``images``: ``[3, h_i, w_i]`` each, float in [0, 1] or uint8, already at model size (no ``EvalResize``)."""
        if torch.is_tensor(images):
            images = list(images.unbind(0))
        sizes = tuple((int(i.shape[-2]), int(i.shape[-1])) for i in images)
        key = (sizes, images[0].device)
        if self._sizes_cache.get("key") != key:   # one host-to-device copy per distinct batch of sizes
            self._sizes_cache = {"key": key, "value": torch.tensor(sizes, device=images[0].device)}
        original_image_sizes = self._sizes_cache["value"]
        canvas, mask = batch_images(images)
        # the image sizes and the canvas give the transformer its token budgets on the host (one device sync fewer)
        return super().forward(self.backbone(canvas), mask, original_image_sizes, image_sizes=[list(s) for s in sizes],
                               canvas=tuple(canvas.shape[-2:]))
