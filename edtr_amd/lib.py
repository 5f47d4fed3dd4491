"""ctypes binding of libedtr_hip.so, derived at import from include/edtr_hip.h (edtr_amd/header.py reads it): the parameter
structs, every EDTR_* constant (here without the prefix: lib.BF16, lib.ACT_GEGLU, lib.E_ALIGN, lib.NOISE_STEP, ...) and the
prototypes.  Nothing of the header is restated here.  The product path has NO fallback: if the library is missing or a launch
fails, a RuntimeError is raised."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

from .header import HeaderError, parse

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EDTR_AMD_LIB") or os.path.join(HERE, "libedtr_hip.so")     # (EDTR_AMD_LIB: another build of the same ABI, for A/B runs on one device)
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "edtr_hip.h")
with open(HEADER_PATH) as _f:
    HEADER = parse(_f.read())

# the Python class of every struct of the header; its fields are the header's, in order, pointers as c_void_p
STRUCT_NAMES = {
    "IgemmParams": "edtr_igemm_params", "AttnParams": "edtr_attn_params", "GnParams": "edtr_gn_params",
    "WindowAttnParams": "edtr_window_attn_params", "SwinMlpParams": "edtr_swin_mlp_params", "SwinAttnParams": "edtr_swin_attn_params",
    "FfnParams": "edtr_ffn_params", "Lin320Params": "edtr_lin320_params", "Conv64Params": "edtr_conv64_params",
    "Conv128OutParams": "edtr_conv128_out_params", "ImageDesc": "edtr_image_desc", "DetImage": "edtr_det_image",
}
if sorted(STRUCT_NAMES.values()) != sorted(HEADER.structs):
    raise HeaderError(f"lib.STRUCT_NAMES does not name the header's structs: {sorted(set(STRUCT_NAMES.values()) ^ set(HEADER.structs))}")
STRUCTS = {c: type(py, (C.Structure,), {"_fields_": [(f, t.ctype or C.c_void_p) for f, t in HEADER.structs[c]], "__doc__": c})
           for py, c in STRUCT_NAMES.items()}
globals().update({py: STRUCTS[c] for py, c in STRUCT_NAMES.items()})
globals().update({name[len("EDTR_"):]: value for name, value in HEADER.constants.items()})
DECLARED_SYMBOLS = list(HEADER.functions)


def prototype(name: str):
    """(restype, argtypes) of a declared function.  Scalars by width; a pointer to a header struct is POINTER(Struct); every
    other pointer is c_void_p (takes data_ptr() integers, None, ctypes arrays and byref alike); `const char*` is returned as
    c_char_p."""
    ret, params = HEADER.functions[name]
    argtypes, before = [], ""
    for pname, t in params:
        # The one rule the header cannot spell: a struct array comes twice, `X_host` (read by the entry point) followed by `X`,
        # its DEVICE copy.  The device copy is an address the host never dereferences and is passed as an integer.
        device_copy = before == pname + "_host"
        argtypes.append(C.POINTER(STRUCTS[t.base]) if t.ptr == 1 and t.base in STRUCTS and not device_copy else t.ctype or C.c_void_p)
        before = pname
    return ret.ctype or (C.c_char_p if ret.base == "char" else C.c_void_p), argtypes


def bind(cdll: C.CDLL, names=DECLARED_SYMBOLS) -> C.CDLL:
    """Set restype and argtypes of the header's functions (all of them unless `names` says otherwise) on an opened libedtr_hip.so."""
    for name in names:
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = prototype(name)
    return cdll


_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load the shared library (building nothing: see edtr_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    # torch ships its own libamdhip64.so.7; import it FIRST so that libedtr_hip.so binds to the same (already
    # loaded) HIP runtime instead of pulling a second one from /opt/rocm ("no ROCm-capable device" otherwise).
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the EDTR MI355X path has no CPU/PyTorch fallback. "
            "Build it with `python -m edtr_amd.build` (hipcc --offload-arch=gfx950).")
    lib = bind(C.CDLL(LIB_PATH))
    if lib.edtr_abi_version() != HEADER.constants["EDTR_ABI_VERSION"]:
        raise RuntimeError("libedtr_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(code: int, what: str = "") -> None:
    if code != 0:
        msg = load().edtr_error_string(code).decode()
        raise RuntimeError(f"libedtr_hip {what} failed with code {code}: {msg}")
