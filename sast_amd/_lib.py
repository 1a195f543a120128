"""ctypes binding of libsast_hip.so, built at import from include/sast_hip.h (the single source: _header.py reads it; nothing of the
header is restated here).  Fails loudly when the library is missing: there is NO CPU / PyTorch fallback for the hot path."""
from __future__ import annotations

import ctypes as C
import os

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULT_LIB_PATH = os.path.join(_HERE, "libsast_hip.so")
# SAST_LIB_PATH: an A/B or variant build instead of the in-tree product library (tools / measurement scripts only).  The override is
# announced on stderr when the library is loaded and `loaded_path()` reports it (bench.py records it in its JSON line), so a stale
# variable in a shell cannot silently put a parity or benchmark claim on another binary.
LIB_PATH = os.environ.get("SAST_LIB_PATH") or DEFAULT_LIB_PATH
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "sast_hip.h")

with open(HEADER_PATH) as _f:
    _HEADER = _header.parse(_f.read())

RND_MAX_CLASSES = 256     # csrc/sampler_rows.cuh, not in the header
# every struct of the header as a ctypes.Structure under its own name, every SAST_X constant as X
for _name, _value in [*_HEADER.structs.items(), *((k[len("SAST_"):], v) for k, v in _HEADER.constants.items())]:
    if _name in globals():
        raise RuntimeError(f"include/sast_hip.h: {_name} would overwrite sast_amd._lib.{_name}")
    globals()[_name] = _value

_SIGNATURES = {p.name: (p.restype, [a.ctype for a in p.args]) for p in _HEADER.prototypes.values()}

_lib = None


def declared_symbols():
    """every function name declared in include/sast_hip.h"""
    return sorted(_HEADER.prototypes)


def lib():
    global _lib
    if _lib is None:
        # PyTorch-ROCm ships its own libamdhip64.so: it must be in the process BEFORE this library is loaded, otherwise the dynamic
        # linker binds libsast_hip.so to the system copy under /opt/rocm and the process ends up with two HIP runtimes -- torch's
        # owns the device, ours reports "no ROCm-capable device" at the first launch (seen when build() loaded the library first)
        import torch  # noqa: F401
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -m sast_amd.build` (needs hipcc, gfx950). "
                "sast_amd has no CPU/PyTorch fallback for the SAST hot path.")
        if os.path.abspath(LIB_PATH) != os.path.abspath(DEFAULT_LIB_PATH):
            import sys
            print(f"[sast_amd] WARNING: SAST_LIB_PATH is set: loading {LIB_PATH} instead of the product library {DEFAULT_LIB_PATH}", file=sys.stderr)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGNATURES.items():
            fn = getattr(l, name, None)
            if fn is None:
                if is_product_library():
                    raise AttributeError(f"{LIB_PATH} lacks {name}: rebuild it with `python -m sast_amd.build`")
                continue           # an A/B library built from another commit (tools only): that entry point raises when it is called
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def reload_knobs() -> int:
    """the library re-reads every SAST_* tuning knob from the environment at its next use (call after changing os.environ in-process)"""
    return int(lib().sast_config_reload())


def knobs() -> dict:
    """{name: value in use} of the SAST_* knobs the library has read so far"""
    n = lib().sast_config_report(None, 0)
    buf = C.create_string_buffer(n)
    lib().sast_config_report(buf, n)
    out = {}
    for line in buf.value.decode().splitlines():
        k, v = line.split("=", 1)
        out[k] = int(v.split(" ")[0])
    return out


def loaded_path() -> str:
    """the library file behind lib() (the in-tree product unless SAST_LIB_PATH overrides it)"""
    return os.path.abspath(LIB_PATH)


def is_product_library() -> bool:
    return os.path.abspath(LIB_PATH) == os.path.abspath(DEFAULT_LIB_PATH)


_tools = None


def tools_lib():
    """libsast_hip_tools.so: GEMM micro-benchmark / timeline entry points (csrc/k_test.hip) for tools/*.py -- not the product"""
    global _tools
    if _tools is None:
        lib()      # the tools library links against the product library (same directory, rpath $ORIGIN)
        _tools = C.CDLL(os.environ.get("SAST_TOOLS_LIB_PATH") or os.path.join(_HERE, "libsast_hip_tools.so"))   # (variant builds: A/B of k_test.hip)
    return _tools


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"libsast_hip: {what} failed with code {rc}")
