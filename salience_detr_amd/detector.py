"""The reference detector after its backbone, in eval mode (``models/detectors/salience_detr.py:158-243`` without
``self.backbone``, the pre-processing and the training branch).

``SalienceDETRHead`` holds ``neck`` (``ChannelMapper``), ``position_embedding`` (``PositionEmbeddingSine``), ``transformer``
(``SalienceTransformer``) and ``postprocessor`` (``PostProcess``) under the reference's attribute names, so a reference
``SalienceDETR`` state dict loads once its ``backbone.*``, ``denoising_generator.*`` and ``_classes_`` entries are removed
(``head_state_dict``).  ``forward(backbone_feats, mask, original_image_sizes)`` runs neck -> per-level masks and positions
(one launch) -> transformer -> post-processing and returns ``PostProcess``'s list of dicts.
"""
from typing import Dict, List, Sequence, Tuple, Union

import torch
from torch import Tensor, nn

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
