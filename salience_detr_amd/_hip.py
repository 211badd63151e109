"""ctypes binding of libsalience_hip.so (the C ABI declared in include/salience_hip.h).

The product path has NO CPU fallback: if the library is missing, or an operator is handed a
tensor that is not on a HIP device, the call raises.  PyTorch is used here only as the owner
of device memory and streams (``tensor.data_ptr()``, ``torch.cuda.current_stream()``).
"""
import ctypes
import os
import re
from typing import Optional

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libsalience_hip.so")
# The fp16-activation flavour (round 5): the same sources built with -DSDETR_ACT_F16, same C ABI, every 16-bit ACTIVATION
# (token rows, projection slabs, 16-bit outputs, packed weights) IEEE half instead of bfloat16 (csrc/common.h).  An
# operator picks the library by the dtype of the activations it is handed: ``lib(x.dtype)``.
F16_LIB_PATH = os.path.join(_HERE, "libsalience_hip_f16.so")

F32, BF16, F16, I64 = 0, 1, 2, 3
EINVAL = -1
ACT16 = (torch.bfloat16, torch.float16)      # the two 16-bit activation types (one library each)

_lib = None
_lib_f16 = None


def is_act16(dt) -> bool:
    return dt in ACT16


class HipExtensionError(RuntimeError):
    pass


# ---- the ABI, read from the header -----------------------------------------------------------------------------------
# include/salience_hip.h is the only place an entry point or a job struct is declared: SIGNATURES, the ctypes Structure
# classes and LAUNCHES below are derived from it.  parse_header is no C parser -- it takes the declarations this header
# is written in (`typedef struct {...} name;` and `ret sdetr_name(args);`) and refuses anything else.
HEADER_PATH = os.path.normpath(os.path.join(_HERE, "..", "include", "salience_hip.h"))
_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
            "double": ctypes.c_double, "sdetr_stream_t": ctypes.c_void_p}
_STRUCT = re.compile(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;")
_FUNCTION = re.compile(r"([\w\s*]+?)\b(sdetr_\w+)\s*\(([^()]*)\)\s*;")
_OTHER = re.compile(r'extern\s+"C"\s*\{|typedef\s+struct\s+\w+\s*\*\s*sdetr_stream_t\s*;|\}')


def _declared(decl: str, where: str):
    """``[(name, ctype), ...]`` of ``T a`` / ``const T *a, *b`` / ``T a[]``: a pointer or an array is ``c_void_p``."""
    m = re.fullmatch(r"\s*(?:const\s+)?(\w+)\b(.+)", decl, re.S)
    out = []
    for d in m.group(2).split(",") if m else ():
        name = re.search(r"(\w+)\s*(?:\[\w*\])?\s*$", d)
        ctype = ctypes.c_void_p if "*" in d or "[" in d else _SCALARS.get(m.group(1))
        if name is None or ctype is None:
            raise HipExtensionError(f"unknown type in '{decl.strip()}' of '{where}'")
        out.append((name.group(1), ctype))
    if not out:
        raise HipExtensionError(f"cannot read '{decl.strip()}' of '{where}'")
    return out


def parse_header(text: str):
    """``(signatures, structs, launches)`` of a header in the format of include/salience_hip.h: ``signatures`` maps every
    ``sdetr_*`` function to ``(restype, argtypes)``, ``structs`` every ``typedef struct`` to its ``_fields_`` list,
    ``launches`` is the set of functions whose first parameter is ``sdetr_stream_t``."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    structs = {name: [f for field in body.split(";") if field.strip() for f in _declared(field, name)]
               for body, name in _STRUCT.findall(text)}
    text = _STRUCT.sub(" ", text)
    signatures, launches = {}, set()
    for ret, name, params in _FUNCTION.findall(text):
        params = [] if params.strip() in ("void", "") else params.split(",")
        if ret.split() == ["const", "char", "*"]:
            restype = ctypes.c_char_p
        else:
            restype = _declared(ret + " " + name, name)[0][1]          # (the function's name stands in for a declarator's)
        args = [_declared(p, name) for p in params]
        if any(len(a) != 1 for a in args):
            raise HipExtensionError(f"cannot read the parameters of '{name}'")
        signatures[name] = (restype, [a[0][1] for a in args])
        if params and params[0].split()[0] == "sdetr_stream_t":
            launches.add(name)
    rest = _OTHER.sub(" ", _FUNCTION.sub(" ", text)).strip()
    if rest:
        raise HipExtensionError(f"cannot read this declaration: '{rest[:120]}'")
    return signatures, structs, launches


def _read_header():
    if not os.path.exists(HEADER_PATH):
        raise HipExtensionError(f"{HEADER_PATH} is missing: the binding reads the C ABI from it")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


# name -> (restype, argtypes); the job structs' fields; the entry points that take a stream first (what launch() calls)
SIGNATURES, _STRUCTS, LAUNCHES = _read_header()
# One ctypes.Structure per typedef, sdetr_finalize_job -> FinalizeJobStruct: FinalizeJobStruct, BorderedLayoutStruct,
# RowOrdersJobStruct, RankJobStruct, SetOutputStruct, FrontendLevelStruct, BackboneOpStruct, BackboneBwdOpStruct, ...
for _name, _fields in _STRUCTS.items():
    _cls = "".join(w.capitalize() for w in _name[len("sdetr_"):].split("_")) + "Struct"
    globals()[_cls] = type(_cls, (ctypes.Structure,), {"_fields_": _fields, "__doc__": f"``{_name}`` of include/salience_hip.h."})


def _load(path: str) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise HipExtensionError(
            f"{path} is missing: build it with `python -m salience_detr_amd.csrc.build` "
            "(or __graft_entry__.build()); there is no CPU fallback for the hot path")
    cdll = ctypes.CDLL(path)          # RTLD_LOCAL: the two flavours export the same names and do not see each other
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(cdll, name)  # AttributeError -> the header and the library disagree
        fn.restype = res
        fn.argtypes = args
    if cdll.sdetr_abi_version() != 1:
        raise HipExtensionError(f"{os.path.basename(path)} ABI version mismatch")
    return cdll


def lib(act=None) -> ctypes.CDLL:
    """Load the shared library once; fail loudly if it is not built.  ``act``: the dtype (or a tensor) of the 16-bit
    activations of the call -- ``torch.float16`` selects the fp16-activation flavour, anything else the bf16 library (which
    also holds every fp32 / integer operator)."""
    global _lib, _lib_f16
    if act is not None and not isinstance(act, torch.dtype):
        act = act.dtype
    if act == torch.float16:
        if _lib_f16 is None:
            _lib_f16 = _load(F16_LIB_PATH)
        return _lib_f16
    if _lib is None:
        _lib = _load(LIB_PATH)
    return _lib


def check(code: int, what: str, library: Optional[ctypes.CDLL] = None) -> None:
    """Raises on a non-zero status.  The error text is thread-local inside each library; ``library`` names the one the
    failing call went to (default: the bf16 library, ``lib()``)."""
    if code != 0:
        msg = (library or lib()).sdetr_last_error().decode(errors="replace")
        if code == EINVAL:
            raise RuntimeError(f"{what}: {msg}")
        raise RuntimeError(f"{what}: HIP launch error {code}: {msg}")


def launch(name: str, act, device, *args, what: Optional[str] = None) -> None:
    """Enqueue entry point ``name`` on ``device``'s current stream: ``lib(act).<name>(stream, *args)`` under
    ``torch.cuda.device(device)`` -- ``device`` is the device of the tensors whose pointers are in ``args`` --, raising
    with the called library's own error text on a non-zero status.  ``act``: what ``lib()`` takes, or a library it
    returned.  ``what`` names the call in the error (default: ``name`` without ``sdetr_``).  Only entry points whose first
    parameter is ``sdetr_stream_t`` are launches; size queries and the like go through ``lib().fn(...)``."""
    if name not in LAUNCHES:
        raise HipExtensionError(f"{name} is not a launch: its first parameter in the header is not sdetr_stream_t")
    library = act if isinstance(act, ctypes.CDLL) else lib(act)
    with torch.cuda.device(device):
        code = getattr(library, name)(torch.cuda.current_stream().cuda_stream, *args)
    check(code, what or name[len("sdetr_"):], library)


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def require_device(what: str, **tensors) -> None:
    """The reference asserts `.is_cuda` + contiguity (ms_deform_attn_cuda.cu:20-30); so do we."""
    for name, t in tensors.items():
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(f"{what}: {name} must be a HIP (cuda) tensor; the hot path has no CPU fallback")
        if not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} tensor has to be contiguous")


def dtype_code(dt: torch.dtype) -> int:
    if dt == torch.float32:
        return F32
    if dt == torch.bfloat16:
        return BF16
    if dt == torch.float16:
        return F16  # head-major value maps (either library); activations of the fp16 flavour (lib(torch.float16))
    raise RuntimeError(f"unsupported dtype {dt} (float32 / bfloat16 / float16)")
