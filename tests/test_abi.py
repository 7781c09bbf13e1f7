"""The C-ABI library builds for gfx950, loads, and exports every symbol include/nbp_hip.h declares; the reader that derives the
ctypes signatures from that header; the header as C."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from nextbestpath_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "nbp_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(nbp_[a-z0-9_]+)\s*\(", txt)))


def test_library_exists_and_loads():
    assert os.path.exists(_lib.LIB_PATH), "run `python -m nextbestpath_amd.build` (or __graft_entry__.build())"
    ctypes.CDLL(_lib.LIB_PATH)


def test_every_declared_symbol_is_exported_and_bound():
    names = _declared()
    assert len(names) >= 20
    handle = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(handle, n), f"{n} declared in include/nbp_hip.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature in nextbestpath_amd/_lib.py"
    for n in _lib.SIGNATURES:
        assert n in names, f"{n} bound in _lib.py but not declared in the header"


# ---- the reader that fills _lib.SIGNATURES, on small synthetic headers

def test_reader_declaration_over_three_lines_and_the_integer_types():
    sigs = _lib.parse_header("int nbp_a(const float* x,\n"
                             "          long long n, unsigned long long m,\n"
                             "          unsigned k, int i, float f, double d);\n")
    assert sigs == {"nbp_a": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_longlong, ctypes.c_ulonglong, ctypes.c_uint, ctypes.c_int,
                                             ctypes.c_float, ctypes.c_double])}
    assert len({ctypes.c_uint, ctypes.c_longlong, ctypes.c_ulonglong}) == 3


def test_reader_skips_comments_preprocessor_lines_and_struct_bodies():
    sigs = _lib.parse_header("/* not bound: nbp_fake(int x); */\n"
                             "#define NBP_E_ARG (-1)\n"
                             "typedef struct nbp_weights nbp_weights;\n"
                             "typedef struct nbp_layer_timing {\n    char name[48];\n    double flops;   /* 2*M*N*K */\n"
                             "    int tile, split_k;\n} nbp_layer_timing;\n"
                             "int nbp_timed(const nbp_weights* handle, nbp_layer_timing* timings_host, int max_entries);\n")
    assert sigs == {"nbp_timed": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int])}


def test_reader_void_size_t_and_pointer_to_pointer():
    sigs = _lib.parse_header("int nbp_version(void);\n"
                             "size_t nbp_bytes(size_t n, const void* const* w_host_array);\n"
                             "void nbp_free(nbp_weights* handle);\n")
    assert sigs == {"nbp_version": (ctypes.c_int, []),
                    "nbp_bytes": (ctypes.c_size_t, [ctypes.c_size_t, ctypes.c_void_p]),
                    "nbp_free": (None, [ctypes.c_void_p])}
    assert list(sigs) == ["nbp_version", "nbp_bytes", "nbp_free"]          # the header's order


@pytest.mark.parametrize("decl", ["int nbp_bad(short n);", "int nbp_bad(float v[3]);", "int nbp_bad(int (*cb)(int));",
                                  "int32_t nbp_bad(int n);", "const char* nbp_bad(void);",
                                  # what the strict pattern cannot read, the crude one still sees
                                  "int nbp_bad(int n) { return n; }", "int nbp_bad(int n)\nint nbp_good(void);"])
def test_reader_refuses_what_it_cannot_bind(decl):
    with pytest.raises(_lib.NbpHipError, match="nbp_bad"):
        _lib.parse_header("int nbp_before(void);\n" + decl + "\nint nbp_after(int n);\n")


def test_reader_names_a_missing_header(monkeypatch, tmp_path):
    missing = str(tmp_path / "include" / "nbp_hip.h")
    monkeypatch.setattr(_lib, "HEADER_PATH", missing)
    with pytest.raises(_lib.NbpHipError, match=re.escape(missing)):
        _lib._read_header()


# ---- the header as C, and the one struct Python mirrors by hand

def test_header_compiles_as_c_and_layer_timing_matches(tmp_path):
    cc = shutil.which("cc") or shutil.which("clang", path="/opt/rocm/llvm/bin:/opt/rocm/bin")
    if cc is None:
        pytest.skip("no host C compiler")
    fields = [f for f, _ in _lib.LayerTiming._fields_]
    src, exe = str(tmp_path / "abi.c"), str(tmp_path / "abi")
    with open(src, "w") as fh:
        fh.write('#include <stdio.h>\n#include "nbp_hip.h"\nint main(void) {\n'
                 '    printf("%zu", sizeof(nbp_layer_timing));\n'
                 + "".join(f'    printf(" %zu", offsetof(nbp_layer_timing, {f}));\n' for f in fields)
                 + "    return 0;\n}\n")
    subprocess.run([cc, "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.LayerTiming)] + [getattr(_lib.LayerTiming, f).offset for f in fields]


def test_host_only_queries():
    L = _lib.lib()
    assert L.nbp_abi_version() == 1
    assert L.nbp_packed_weights_bytes() > 49_000_000 * 4
    assert L.nbp_forward_workspace_bytes(1, 256) > 0
    assert L.nbp_forward_workspace_bytes(1, 250) == 0          # S % 16 != 0
    # 2*91.206 GMAC at 256^2
    assert abs(L.nbp_forward_flops(1, 256) / 1e9 - 182.41) < 0.05
    assert abs(L.nbp_forward_flops(1, 128) / 1e9 - 45.60) < 0.02


def test_no_cpu_fallback():
    import pytest
    import torch
    from nextbestpath_amd.networks.nbp_model import NBP
    from nextbestpath_amd.utility import utils
    with torch.device("meta"):
        net = NBP()
    net.eval()
    with pytest.raises(RuntimeError):
        net(torch.zeros(1, 5, 32, 32))
    with pytest.raises(RuntimeError):
        utils.map_points_to_n_imgs(torch.zeros(1, 4, 2), (8, 8), (-1, 1))
