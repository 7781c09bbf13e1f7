"""ctypes loader for libnbp_hip.so (the C ABI declared in include/nbp_hip.h).

The product path has no fallback: ``lib()`` raises if the shared object is missing or does
not export a declared symbol.  Building is explicit (``python -m nextbestpath_amd.build`` or
``__graft_entry__.build()``); importing this module never compiles anything.

The ctypes signatures are not written down here: ``SIGNATURES`` is read from the header's declarations at import
(``parse_header``), so an entry point is declared in include/nbp_hip.h, defined in csrc/ (the compiler checks the two against
each other) and is bound.  Every pointer parameter is ``c_void_p``: the header's C types cannot tell a host ``const float*``
from a device one, so passing a bare integer address where a host array is expected is not a ``TypeError``; ctypes arrays,
``byref(...)``, ``pointer(...)``, ``bytes``, string buffers, ``None`` and integer addresses are all accepted.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libnbp_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(HERE), "include", "nbp_hip.h")


class NbpHipError(RuntimeError):
    pass


class LayerTiming(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("flops", C.c_double), ("ms", C.c_float), ("tile", C.c_int), ("split_k", C.c_int),
                ("M", C.c_longlong), ("N", C.c_int), ("K", C.c_int)]


# the scalar types include/nbp_hip.h uses; anything else in a declaration is an error, not a guess
_SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong,
            "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t}
_DECL = re.compile(r"([\w\s*]+?)\b(nbp_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;")


def _scalar(words: str, name: str, what: str):
    key = " ".join(w for w in words.split() if w != "const")
    if key not in _SCALARS:
        raise NbpHipError(f"include/nbp_hip.h: {name}: {what} `{key}` is not a scalar type of this ABI ({', '.join(_SCALARS)})")
    return _SCALARS[key]


def _param(p: str, name: str):
    p = " ".join(p.split())
    if "(" in p:
        raise NbpHipError(f"include/nbp_hip.h: {name}: function pointer `{p}` cannot be bound")
    if "[" in p:
        raise NbpHipError(f"include/nbp_hip.h: {name}: array parameter `{p}` cannot be bound")
    if "*" in p:
        return C.c_void_p
    return _scalar(p.rpartition(" ")[0], name, "parameter type")   # `<type> <name>`: the last word is the name


def parse_header(text: str) -> dict:
    """{name: (restype, [argtypes])} of every `<ret> nbp_<name>(<params>);` in the text of a C header."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r"\btypedef\s+struct\s+\w+\s*(\{.*?\})?\s*\w+\s*;", "", text, flags=re.S)
    sigs = {}
    for ret, name, params in _DECL.findall(text):
        res = None if ret.strip() == "void" else _scalar(ret, name, "return type")
        sigs[name] = (res, [] if params.strip() == "void" else [_param(p, name) for p in params.split(",")])
    # cross-check with a cruder pattern: every `nbp_<name>(` left in the text has been read as a declaration
    unread = set(re.findall(r"\b(nbp_[a-z0-9_]+)\s*\(", text)) - set(sigs)
    if unread:
        raise NbpHipError(f"include/nbp_hip.h: {', '.join(sorted(unread))}: not readable as `<ret> nbp_<name>(<params>);`")
    return sigs


def _read_header() -> dict:
    try:
        with open(HEADER_PATH) as fh:
            return parse_header(fh.read())
    except OSError as e:
        raise NbpHipError(f"{HEADER_PATH} is missing or unreadable: the ctypes signatures are read from it") from e


# name -> (restype, argtypes), in the order of include/nbp_hip.h; read once per process, here
SIGNATURES = _read_header()

_lock = threading.Lock()
_lib = None


def lib() -> C.CDLL:
    """Returns the loaded library; raises (never falls back) if it cannot be loaded."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NbpHipError(
                f"{LIB_PATH} is missing: build it with `python -m nextbestpath_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        # PyTorch ships its own libamdhip64; it has to be in the process first so that this library binds to the
        # SAME HIP runtime (device pointers and streams cross the boundary).  Loaded the other way round the
        # process ends up with two runtimes and the second one reports hipErrorNoDevice.
        import torch  # noqa: F401
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            try:
                fn = getattr(handle, name)
            except AttributeError as e:  # pragma: no cover
                raise NbpHipError(f"libnbp_hip.so does not export {name}") from e
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


_ERR = {-1: "NBP_E_ARG (bad argument)", -2: "NBP_E_WS (workspace too small)", -3: "NBP_E_SHAPE (unsupported shape)"}


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = _ERR.get(rc, f"hipError_t {rc}" if rc > 0 else f"error {rc}")
        raise NbpHipError(f"{what} failed: {msg}")


def ptr(t) -> int:
    """Device pointer of a contiguous torch tensor (0 for None)."""
    if t is None:
        return 0
    if not t.is_contiguous():
        raise ValueError("tensor passed to the HIP path must be contiguous")
    return t.data_ptr()


# ---- A/B switches of the host side: the same gate as the library's (csrc/nbp_tuning.cpp).  A switch keeps its default unless
# the process opted in with NBP_TUNING=1 AND sets the variable, so an inherited environment never changes results.
_knobs = {}
# switches that change the ARITHMETIC (results differ beyond reordering): a benchmark line measured with one of them set is
# not the headline configuration (bench.py refuses to call it `value`)
NUMERICS_KNOBS = {"NBP_CONV_PRECISION", "NBP_SPLIT_MAX_K", "NBP_SPLIT_MAX_K_SMALL", "NBP_GATE_PSI", "NBP_CONV_HEAD", "NBP_BF16_PSI",
                  "NBP_BF16_FUSE"}
# bit-identical switches (NBP_STEP_OVERLAP, ...) are not listed here; effective_knobs() reports every switch
# that is off its default, numerics-affecting or not


def tuning_active() -> bool:
    return os.environ.get("NBP_TUNING") == "1"


def tune(name: str, default: str) -> str:
    """String-valued A/B switch `name`: `default` unless NBP_TUNING=1 and the variable is set.  Recorded for effective_knobs()."""
    v = default
    if tuning_active():
        e = os.environ.get(name)
        if e is not None and e != "":
            v = e
    _knobs[name] = (default, v)
    return v


def effective_knobs() -> dict:
    """{name: value} of every switch (host side and library) read so far whose value differs from its default."""
    out = {k: v for k, (d, v) in _knobs.items() if v != d}
    if _lib is not None:
        buf = C.create_string_buffer(4096)
        if _lib.nbp_tuning_report(buf, 4096) > 0:
            for item in buf.value.decode().split(","):
                if "=" in item:
                    k, v = item.split("=", 1)
                    out[k] = v
    return out


_raw_stream = None


def current_stream() -> int:
    """Raw hipStream_t of torch's current stream on the current device (the fast private accessor: the public
    torch.cuda.current_stream() builds a Stream object, ~9 us per call and ~25 calls per exploration step)."""
    global _raw_stream
    import torch
    if _raw_stream is None:
        _raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", False)
    if _raw_stream:
        return _raw_stream(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream
