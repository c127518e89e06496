"""ctypes binding of libvst_hip.so (the C ABI declared in include/vst.h).

This is the only place the shared library is touched.  There is deliberately no CPU or
PyTorch fallback: if the library is missing, or a tensor is not on a HIP device, the call
raises.  (The reference path is PyTorch eager; our kernels replace it, they do not wrap it.)
"""
from __future__ import annotations

import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libvst_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "vst.h")


class VstError(RuntimeError):
    pass


_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "size_t": ctypes.c_size_t, "unsigned": ctypes.c_uint}


def _ctype(decl: str, what: str, ret: bool = False):
    """The ctypes type of one parameter (or return) declaration: any pointer is c_void_p (a `const char*` return
    c_char_p), the scalars are _SCALARS; anything else raises."""
    words = decl.replace("*", " * ").split()
    if "*" in words:
        return ctypes.c_char_p if ret and words[:3] == ["const", "char", "*"] else ctypes.c_void_p
    if not ret and len(words) > 1:
        words = words[:-1]  # the parameter's name
    if len(words) != 1 or words[0] not in _SCALARS:
        raise VstError(f"include/vst.h: cannot map `{decl.strip()}` of {what} to a ctypes type")
    return _SCALARS[words[0]]


def parse_header(text: str) -> dict:
    """name -> (restype, argtypes) of every prototype in the text of include/vst.h."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^\s*#.*$|extern\s+\"C\"\s*\{|\}", " ", text, flags=re.M)
    sigs = {}
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        m = re.fullmatch(r"(.*?)\b(\w+)\s*\((.*)\)", stmt, flags=re.S)
        if not m:
            raise VstError(f"include/vst.h: `{' '.join(stmt.split())}` is not a prototype")
        ret, name, params = m.groups()
        params = [] if params.strip() in ("", "void") else params.split(",")
        sigs[name] = (_ctype(ret, name, ret=True), [_ctype(p, name) for p in params])
    return sigs


def _read_header() -> dict:
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise VstError(f"the ABI header {HEADER_PATH} is missing ({e}); the signatures are read from it") from e


SIGNATURES = _read_header()  # name -> (restype, argtypes)

_lib = None


def load(path: str | None = None):
    """Load the HIP library (idempotent).  Raises VstError when it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    alt = os.environ.get("VST_LIB_AB")  # diagnostics only (tools/gemm_ablate.py A/B of two builds)
    path = path or alt or LIB_PATH
    if not os.path.exists(path):
        raise VstError(f"libvst_hip.so not found at {path}; build it with `make` (hipcc --offload-arch=gfx950)")
    lib = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        if alt and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def exported_symbols() -> list[str]:
    return list(SIGNATURES)


def call(name: str, *args):
    rc = getattr(load(), name)(*args)
    if rc != 0:
        why = {1: "bad argument", 2: "launch failure", 3: "unsupported shape"}.get(rc, "error")
        raise VstError(f"{name} failed with status {rc} ({why})")
    return rc
