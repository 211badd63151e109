"""Salience-DETR on MI355X.  Modules are imported by name (``salience_detr_amd.detector`` ...); the training-side entry
points are also reachable from the package, resolved on first use so that importing the package stays free of torch."""

_LAZY = {"GenerateCDNQueries": "denoising", "SalienceDETR": "detector", "SalienceDETRHead": "detector",
         "EvalResize": "eval_resize", "eval_resize_size": "eval_resize", "batch_images": "backbone",
         "ConvNeXtBackbone": "convnext", "CNBlockConfig": "convnext", "FocalNetBackbone": "focalnet",
         "SwinBackbone": "swin", "TrainTransform": "train_transform", "TrainBatch": "train_transform",
         "AugmentParams": "train_transform", "sample_params": "train_transform", "shortest_size": "train_transform",
         "transform_targets": "train_transform", "CocoBoxEvaluator": "coco_eval", "evaluate": "coco_eval",
         "deform_conv2d": "deform_conv", "DeformConv2d": "deform_conv", "DeformConv2dPack": "deform_conv"}


def __getattr__(name):
    if name in _LAZY:
        from importlib import import_module
        return getattr(import_module("." + _LAZY[name], __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
