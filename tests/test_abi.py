"""The ABI between Python and libsast_hip.so.  include/sast_hip.h is the single source: sast_amd/_header.py reads it and sast_amd/_lib.py
builds every ctypes.Structure, signature and constant from the reader's tables.  Here a C compiler judges the reader: ONE
`gcc -std=c99 -Wall -Werror -c` of a generated file that includes the header and holds, as compile-time assertions (an array type of
negative size when false), the sizeof and every offsetof of EVERY struct the reader found, the value of EVERY constant, the width of
every scalar type of the mapping, and for EVERY prototype a function pointer of the reader's argument types initialised with the
function (an argument dropped, merged or mis-split is an incompatible pointer: an error).  Nothing is linked or run.  CPU only."""
import ctypes as C
import subprocess

import pytest

from sast_amd import _header, _lib

H = _lib._HEADER
P = C.c_void_p
# the signatures that mix widths, written out by hand: the one place where the mapping text -> ctypes is pinned and not derived
PINNED = {
    "sast_adamw_onecycle": (C.c_int, [P, P, P, P, C.c_size_t, P, C.c_double, C.c_double, C.c_float, C.c_float, C.c_float, C.c_float,
                                      C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, P]),
    "sast_select": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(_lib.SastSel), P]),
    "sast_evqueue_push": (C.c_int, [C.POINTER(_lib.SastEvQueueArgs), P, P, P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, C.c_int64, P, P]),
    "sast_prof_calibrate": (C.c_float, [P, C.c_int]),
    "sast_launch_count": (C.c_ulonglong, []),
    "sast_config_get": (C.c_int, [C.c_char_p, C.c_int]),
    "sast_mean_square_bwd": (C.c_int, [P, P, C.c_int, P, C.c_int, P, P]),
    "sast_mswsa_fused_ws_floats": (C.c_size_t, [C.c_int] * 5),
}


def _abi_c(header=H, sizeof=C.sizeof):
    """the C file: `sizeof` is ctypes.sizeof (the negative control of test_the_c_file_fails_when_a_number_is_wrong passes a wrong one)"""
    lines = ["#include <stddef.h>", f'#include "{_lib.HEADER_PATH}"', "#define CHECK(name, cond) typedef char name[(cond) ? 1 : -1]"]
    for n, st in header.structs.items():
        lines.append(f"CHECK(sizeof_{n}, sizeof({n}) == {sizeof(st)});")
        for f in st.c_fields:
            lines.append(f"CHECK(offsetof_{n}_{f.name}, offsetof({n}, {f.name}) == {getattr(st, f.name).offset});")
            lines.append(f"CHECK(sizeof_{n}_{f.name}, sizeof((({n}*)0)->{f.name}) == {C.sizeof(f.ctype)});")
    for n, v in header.constants.items():
        lines.append(f"CHECK(value_{n}, {n} == {v});")
    for n, ct in _header.SCALARS.items():         # width, and for the integer types signedness (a cast of a float is no integer constant)
        sign = "" if ct in (C.c_float, C.c_double) else f" && (({n})-1 < 0) == {int(ct(-1).value < 0)}"
        lines.append(f"CHECK(width_{n.replace(' ', '_')}, sizeof({n}) == {C.sizeof(ct)}{sign});")
    for p in header.prototypes.values():
        lines.append(f"{p.ret} (*p_{p.name})({', '.join(a.ctext for a in p.args) or 'void'}) = {p.name};")
    return "\n".join(lines) + "\n"


def _gcc(tmp_path, text):
    (tmp_path / "abi.c").write_text(text)
    return subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-o", str(tmp_path / "abi.o"), str(tmp_path / "abi.c")],
                          capture_output=True, text=True)


def test_a_c_compiler_agrees_with_every_struct_constant_scalar_and_prototype(tmp_path):
    assert len(H.structs) >= 20 and len(H.constants) >= 39 and len(H.prototypes) >= 94     # the header only grows (99 before the five sast_dw_* left)
    text = _abi_c()
    for st in H.structs.values():
        assert [f for f, _t in st._fields_] == [f.name for f in st.c_fields] and len(set(f.name for f in st.c_fields)) == len(st.c_fields)
        assert all(text.count(f"offsetof({st.__name__}, {f.name})") == 1 for f in st.c_fields)
    assert text.count(" = sast_") == len(H.prototypes) and text.count("CHECK(value_") == len(H.constants)
    r = _gcc(tmp_path, text)
    assert r.returncode == 0, r.stderr[-6000:]


def test_the_c_file_fails_when_a_number_is_wrong(tmp_path):
    """the negative control of the method: one struct size off by one, and one argument dropped, each stop the compile by name"""
    r = _gcc(tmp_path, _abi_c(sizeof=lambda st: C.sizeof(st) + (st is _lib.SastSel)))
    assert r.returncode != 0 and "sizeof_SastSel" in r.stderr and "sizeof_SastLstmArgs" not in r.stderr
    p = H.prototypes["sast_add_rows"]
    one = H._replace(structs={}, constants={}, prototypes={p.name: p._replace(args=p.args[:3] + p.args[4:])})
    r = _gcc(tmp_path, _abi_c(one))
    assert r.returncode != 0 and "p_sast_add_rows" in r.stderr


def test_lib_is_built_from_the_reader_tables():
    for n, st in H.structs.items():
        assert getattr(_lib, n) is st and issubclass(st, C.Structure)
    for n, v in H.constants.items():
        assert n.startswith("SAST_") and getattr(_lib, n[len("SAST_"):]) == v and type(v) is int
    assert set(_lib._SIGNATURES) == set(H.prototypes) and _lib.declared_symbols() == sorted(H.prototypes)
    for n, p in H.prototypes.items():
        assert _lib._SIGNATURES[n] == (p.restype, [a.ctype for a in p.args]), n
    assert _lib.RND_MAX_CLASSES == 256 and "SAST_RND_MAX_CLASSES" not in H.constants     # csrc/sampler_rows.cuh's, not the header's
    # arrays sized by a constant of the header
    assert _lib.ZERO_MAX_TENSORS == len(_lib.SastSampleZeroDev().x) == len(_lib.SastTensorCopy().dst)
    assert _lib.GATHER_MAX_SRC == len(_lib.SastSampleGather().src) and _lib.GATHER_MAX_OUT == len(_lib.SastSampleGather().t_of)
    assert _lib.SastMswsaArgs.sel.size == C.sizeof(_lib.SastSel)                          # a struct-typed field, by value


@pytest.mark.parametrize("name", sorted(PINNED))
def test_pinned_signatures(name):
    assert _lib._SIGNATURES[name] == PINNED[name]


def test_constants_and_fields_forms():
    h = _header.parse("#ifndef G_H\n#define G_H\n#define SAST_N 3   /* three */\n#define SAST_F(x) ((x) + SAST_N)\n"
                      "enum { SAST_A, SAST_B, SAST_C = 1 << 4, SAST_D, SAST_E = 0x20 };\n"
                      "typedef struct { int32_t B, H; float *a, *b, c; const float* x; uint8_t m[SAST_N], k[2]; double* w[SAST_D]; } SastT;\n"
                      "typedef struct SastU { SastT t; int64_t n; } SastU;\nvoid sast_g(void);\nlong sast_f(const SastU* u, char* s);\n#endif\n")
    assert [(p.ret, p.restype, p.args) for p in h.prototypes.values()] == [("void", None, ()), ("long", C.c_long, (
        ("const SastU*", C.POINTER(h.structs["SastU"])), ("char*", C.c_char_p)))]
    assert h.constants == {"SAST_N": 3, "SAST_A": 0, "SAST_B": 1, "SAST_C": 16, "SAST_D": 17, "SAST_E": 32}
    assert list(h.structs) == ["SastT", "SastU"]
    assert [(f.name, f.ctext) for f in h.structs["SastT"].c_fields] == [
        ("B", "int32_t"), ("H", "int32_t"), ("a", "float*"), ("b", "float*"), ("c", "float"), ("x", "const float*"), ("m", "uint8_t"),
        ("k", "uint8_t"), ("w", "double*")]
    assert [t for _n, t in h.structs["SastT"]._fields_] == [C.c_int32, C.c_int32, P, P, C.c_float, P, C.c_uint8 * 3, C.c_uint8 * 2, P * 17]
    assert h.structs["SastU"]._fields_ == [("t", h.structs["SastT"]), ("n", C.c_int64)]


@pytest.mark.parametrize("bad", [
    "static int x;",                                           # a line it cannot classify
    "typedef struct { int32_t n; wchar_t w; } SastBad;",       # a field of an unknown type
    "typedef struct { int32_t n; mystery_t* w; } SastBad;",    # ... also behind a pointer
    "int sast_bad(unsigned n, sast_stream_t stream);",         # an unknown scalar in an argument list
    "int sast_bad(int, sast_stream_t stream);",                # an argument without a name
    "short sast_bad(void);", "#define SAST_BAD 1.5f", "#define SAST_BAD (1 << 3)", "#define OTHER 3", "#if 0",
    "enum { SAST_BAD = SAST_DT_F32 + 1 };", "typedef struct { int32_t n : 3; } SastBad;", "typedef struct { int32_t n[SAST_UNKNOWN]; } SastBad;",
    "typedef struct { union { int32_t a; float b; } u; } SastBad;", "typedef int (*sast_callback)(int);", "}",
    "int sast_version(void);", "enum { SAST_DT_F32 = 0 };",    # declared twice
])
def test_the_reader_refuses_what_it_does_not_know(bad):
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    at = text.rindex("#ifdef __cplusplus")                      # inside the extern "C" bracket, after every declaration
    with pytest.raises(RuntimeError, match="sast_hip.h"):
        _header.parse(text[:at] + bad + "\n" + text[at:])
