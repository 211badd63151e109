"""tests/golden/eval_resize_cases.npz: the reference's ``EvalResize`` (models/detectors/base_detector.py:20-53) run on the CPU
on the sizes and images of tests/eval_resize_cases.py.

``base_detector.py`` is imported through ``_ref_import`` with the REAL ``transforms/functional.py`` and
``_functional_tensor.py`` (the ``transforms`` package is pointed at the reference checkout without running its
``__init__``; ``transforms.v2``, which needs torchvision, is a stub: only ``EvalResize`` is used), so
``EvalResize.forward`` itself produces everything stored here.  Inputs are not stored: the cases module regenerates them.

Stored:
  * ``size.rows`` [N, 4] (h, w, min_size, max_size), ``size.out`` [N, 2] the (new_height, new_width) of the reference's own
    shape arithmetic (read off the resize's output), ``size.differs`` [N] where exact rational arithmetic gives another size.
  * per float image ``<name>.f32.*``: ``ref64`` = the reference's resize of the float64 image (which its cast helper keeps in
    float64), STORED AS float32 (adds at most 3e-8 on values in [0, 1]; the file would otherwise pass the size limit);
    ``d_ref`` = max |reference's float32 output - the float64 one|.  (The float32 output itself is not stored, for size.)
  * per uint8 image ``<name>.u8.*``: ``ref32`` = the reference's uint8 output; ``diff_idx`` / ``diff_val``: the flat positions
    where ``round_half_even(float64 value)`` differs from it, and that value there (so ``round64`` is rebuilt exactly);
    ``d_ref`` = max |float32 pre-rounding value - float64 pre-rounding value| on the 0..255 scale; ``excluded`` = packed bits of
    the pixels whose float64 value is closer than ``tau = max(4 d_ref, 1e-3)`` to a .5 boundary; ``share`` = their share.
  * ``mixed.*``: the batch of three sizes: ``sizes`` (resized), ``canvas_hw``, ``mask`` (packed bits) of the reference's
    ``image_list_from_tensors``, and per dtype ``d_ref`` = max |float32 eval preprocessing - float64 one| on the canvas (uint8:
    off the excluded pixels, where both start from the same uint8 value).  The float64 canvas itself is
    ``eval_resize_cases.canvas64`` of the stored per-image values; this script asserts that it equals the reference's
    ``image_list_from_tensors`` of the float64 Normalize.

Asserted here (and re-checked by tests/test_eval_resize_cpu.py from the arrays): every excluded share is at most 2 %; the
reference's own uint8 output equals ``round64`` off the excluded pixels and is within 1 of it on them.

Run from the repository root: ``python tests/golden/make_eval_resize_golden.py`` (needs the reference checkout).
"""
import importlib.machinery
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as TF

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))   # tests/ (eval_resize_cases)
sys.path.insert(0, HERE)

import _ref_import  # noqa: E402
import eval_resize_cases as EC  # noqa: E402

OUT = os.path.join(HERE, "eval_resize_cases.npz")


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    return m


def load_reference():
    """``(base_detector module, image_list_from_tensors)`` with the real ``transforms.functional``."""
    _ref_import.install()
    root = _ref_import.REFERENCE_ROOT
    _stub("transforms").__path__ = [os.path.join(root, "transforms")]      # the package without its __init__
    _stub("transforms.v2", ConvertImageDtype=None, Normalize=None)
    sys.modules["torchvision.ops"].boxes = sys.modules["torchvision.ops.boxes"]

    class ImageList:   # torchvision's holder: the batched tensor and the sizes before padding
        def __init__(self, tensors, image_sizes):
            self.tensors, self.image_sizes = tensors, image_sizes
    sys.modules["torchvision.models.detection.image_list"].ImageList = ImageList
    for name in ("omegaconf", "accelerate"):
        try:
            importlib.import_module(name)
        except ImportError:
            _stub(name, DictConfig=dict, ListConfig=list, OmegaConf=object)
    if "accelerate.logging" not in sys.modules:
        try:
            importlib.import_module("accelerate.logging")
        except ImportError:
            _stub("accelerate.logging", get_logger=lambda *a, **k: None)
    _stub("models").__path__ = [os.path.join(root, "models")]
    _stub("models.detectors").__path__ = [os.path.join(root, "models", "detectors")]
    spec = importlib.util.spec_from_file_location("models.detectors.base_detector",
                                                  os.path.join(root, "models", "detectors", "base_detector.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    from util.misc import image_list_from_tensors
    return mod, image_list_from_tensors


def main():
    mod, image_list_from_tensors = load_reference()
    torch.set_num_threads(1)
    data = {}

    # ---- sizes: the reference's shape arithmetic, read off the output of its own forward on a 1-channel image
    rows = EC.size_grid()
    out = np.zeros((len(rows), 2), dtype=np.int64)
    differs = np.zeros(len(rows), dtype=bool)
    probes = {}
    for i, (h, w, mn, mx) in enumerate(rows.tolist()):
        captured = {}
        real_resize = mod.F.resize

        def spy(image, size, **kw):
            captured["size"] = (int(size[0]), int(size[1]))
            return image
        mod.F.resize = spy
        try:
            probe = probes.setdefault((h, w), torch.empty(1, h, w, dtype=torch.uint8))
            mod.EvalResize(mn, mx, antialias=True)(probe)
        finally:
            mod.F.resize = real_resize
        probes.clear()
        out[i] = captured["size"]
        differs[i] = tuple(out[i]) != EC.exact_size(h, w, mn, mx)
    assert differs.any()
    data["size.rows"], data["size.out"], data["size.differs"] = rows, out, differs
    print("sizes", len(rows), "float32 != exact on", int(differs.sum()), flush=True)

    # ---- images
    resize = mod.EvalResize(EC.MIN_SIZE, EC.MAX_SIZE, antialias=True)
    kept = {}
    for name, ((h, w), (nh, nw), _) in EC.IMAGES.items():
        img = EC.image(name, "f32")
        ref32 = resize(img)
        ref64 = resize(img.double())
        assert ref32.dtype == torch.float32 and ref64.dtype == torch.float64 and tuple(ref32.shape[1:]) == (nh, nw)
        d = (ref32.double() - ref64).abs().max().item()
        data[f"{name}.f32.ref64"] = ref64.float().numpy()
        data[f"{name}.f32.d_ref"] = np.float64(d)
        u8 = EC.image(name, "u8")
        r8 = resize(u8)
        assert r8.dtype == torch.uint8 and tuple(r8.shape[1:]) == (nh, nw)
        if (h, w) == (nh, nw):
            pre64, pre32 = u8.double(), u8.float()
        else:
            pre64 = TF.interpolate(u8.double()[None], size=(nh, nw), mode="bilinear", align_corners=False, antialias=True)[0]
            pre32 = TF.interpolate(u8.float()[None], size=(nh, nw), mode="bilinear", align_corners=False, antialias=True)[0]
        assert torch.equal(pre32.round().to(torch.uint8), r8)          # the reference's path is exactly this
        d8 = (pre32.double() - pre64).abs().max().item()
        pre64 = pre64.numpy()
        round64 = EC.round_half_even(pre64).astype(np.uint8)
        exc = EC.excluded(pre64, EC.tau_u8(d8))
        share = exc.mean()
        r8n = r8.numpy()
        diff = np.flatnonzero(round64 != r8n)
        assert share <= EC.EXCLUDED_CAP, (name, share)
        assert exc.reshape(-1)[diff].all() and (np.abs(round64.astype(int) - r8n.astype(int)) <= 1).all(), name
        data[f"{name}.u8.ref32"] = r8n
        data[f"{name}.u8.diff_idx"] = diff.astype(np.int64)
        data[f"{name}.u8.diff_val"] = round64.reshape(-1)[diff]
        data[f"{name}.u8.excluded"] = np.packbits(exc.reshape(-1))
        data[f"{name}.u8.d_ref"] = np.float64(d8)
        data[f"{name}.u8.share"] = np.float64(share)
        kept[name] = dict(ref32=ref32, ref64=ref64, r8=r8, round64=round64, exc=exc)
        print(f"{name}: {h}x{w} -> {nh}x{nw}  d_ref f32 {d:.3g}  u8 {d8:.3g}  excluded {share:.4%}  ref32 != round64 on "
              f"{len(diff)}", flush=True)

    # ---- the canvas of the mixed batch
    def norm(t):   # Normalize in the image's own dtype (the statistics become tensors of that dtype, as in the reference)
        return (t - torch.tensor(EC.MEAN, dtype=t.dtype).view(3, 1, 1)) / torch.tensor(EC.STD, dtype=t.dtype).view(3, 1, 1)
    for dt in EC.DTYPES:
        if dt == "f32":
            imgs64 = [kept[n]["ref64"] for n in EC.MIXED]
            imgs32 = [kept[n]["ref32"] for n in EC.MIXED]
            stored = [data[f"{n}.f32.ref64"].astype(np.float64) for n in EC.MIXED]
        else:
            imgs64 = [torch.from_numpy(kept[n]["round64"]).double() / 255 for n in EC.MIXED]
            imgs32 = [kept[n]["r8"].float() / 255 for n in EC.MIXED]
            stored = [kept[n]["round64"].astype(np.float64) / 255 for n in EC.MIXED]
        il64 = image_list_from_tensors([norm(i) for i in imgs64])
        il32 = image_list_from_tensors([norm(i) for i in imgs32])
        c64, c32 = il64.tensors, il32.tensors
        assert [tuple(s) for s in il64.image_sizes] == [EC.IMAGES[n][1] for n in EC.MIXED]
        assert tuple(c64.shape[-2:]) == EC.MIXED_CANVAS
        mine, mask = EC.canvas64(stored)
        tol = 0 if dt == "u8" else 3e-8 / min(EC.STD) * 1.01
        assert np.abs(mine - c64.numpy()).max() <= tol          # the cases module's canvas IS the reference's
        err = (c32.double() - c64).abs().numpy()
        if dt == "u8":
            for b, n in enumerate(EC.MIXED):
                e = kept[n]["exc"]
                err[b, :, :e.shape[1], :e.shape[2]][e] = 0
        data[f"mixed.{dt}.d_ref"] = np.float64(err.max())
        print("mixed", dt, "canvas", tuple(c64.shape), "d_ref %.3g" % err.max(), flush=True)
    data["mixed.mask"] = np.packbits(mask.reshape(-1))
    data["mixed.canvas_hw"] = np.array(EC.MIXED_CANVAS)
    data["mixed.sizes"] = np.array([EC.IMAGES[n][1] for n in EC.MIXED])
    np.savez_compressed(OUT, **data)
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
