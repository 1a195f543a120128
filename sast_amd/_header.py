"""Reader of include/sast_hip.h: the header is the single source of the ctypes binding (sast_amd/_lib.py builds everything from the
three tables of `parse`).  Pure `re`, no compiler.  It knows the plain, regular C the header is written in and REFUSES everything else
with a RuntimeError that quotes the text: nothing is skipped and no type falls back to int.  tests/test_abi.py lets gcc judge it."""
from __future__ import annotations

import ctypes as C
import re
from collections import namedtuple

Field = namedtuple("Field", "name ctext ctype")        # ctext: the element type of an array field; ctype: the whole field
Arg = namedtuple("Arg", "ctext ctype")
Proto = namedtuple("Proto", "name ret restype args")
Header = namedtuple("Header", "constants structs prototypes")   # dicts in header order; a struct is a ctypes.Structure with .c_fields

SCALARS = {
    "int": C.c_int, "long": C.c_long, "unsigned long long": C.c_ulonglong, "float": C.c_float, "double": C.c_double, "size_t": C.c_size_t,
    "int8_t": C.c_int8, "uint8_t": C.c_uint8, "int16_t": C.c_int16, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64,
    "uint64_t": C.c_uint64,
}
_INT = r"(?:0[xX][0-9a-fA-F]+|[1-9][0-9]*|0)[uUlL]*"
_ITEMS = [(kind, re.compile(rx)) for kind, rx in (
    ("directive", r"#[^\n]*"),
    ("bracket", r'extern\s+"C"\s*\{|\}'),
    ("handle", r"typedef\s+void\s*\*\s*(\w+)\s*;"),
    ("enum", r"enum\s*\{([^{}]*)\}\s*;"),
    ("struct", r"typedef\s+struct\s*(\w*)\s*\{([^{}]*)\}\s*(\w+)\s*;"),
    ("proto", r"([\w\s*]+?)\b(sast_\w+)\s*\(([^(){};]*)\)\s*;"),
)]
_SPACE = re.compile(r"\s*")
_DIRECTIVES = re.compile(r"#\s*(?:include\s*<[\w./]+>|ifndef\s+(\w+)|ifdef\s+__cplusplus|endif)\s*$")
_DEFINE = re.compile(r"#\s*define\s+(\w+)(\(?)\s*(.*?)\s*$")


def _int(text, what):
    if not re.fullmatch(_INT, text):
        raise RuntimeError(f"sast_hip.h: {what}: not an integer literal: {text!r}")
    return int(text.rstrip("uUlL"), 0)


def parse(text: str) -> Header:
    constants, structs, protos, handles = {}, {}, {}, {}
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)

    def new(table, name, value):
        if name in constants or name in structs or name in protos or name in handles:
            raise RuntimeError(f"sast_hip.h: {name} is declared twice")
        table[name] = value

    def ctype(ctext, what):
        base = " ".join(w for w in ctext.replace("*", " ").split() if w != "const")
        depth = ctext.count("*")
        if depth == 0 and base in handles:
            return C.c_void_p
        if depth == 0 and (base in SCALARS or base in structs):
            return SCALARS.get(base) or structs[base]
        if depth == 0 or not (base in SCALARS or base in structs or base in handles or base in ("void", "char")):
            raise RuntimeError(f"sast_hip.h: {what}: unknown type {ctext!r}")
        if depth == 1 and base in structs:
            return C.POINTER(structs[base])
        return C.c_char_p if (depth == 1 and base == "char") else C.c_void_p

    def split_name(decl, what):   # 'const float* x' -> ('const float*', 'x', None); 'uint8_t sel[256]' -> ('uint8_t', 'sel', '256')
        m = re.fullmatch(r"([\w\s*]*?[\s*])(\w+)\s*(?:\[\s*(\w+)\s*\])?", decl.strip())
        if not m:
            raise RuntimeError(f"sast_hip.h: {what}: cannot read {decl.strip()!r}")
        return re.sub(r"\s*\*", "*", " ".join(m.group(1).split())), m.group(2), m.group(3)

    def directive(line):
        m = None if line.rstrip().endswith("\\") else _DIRECTIVES.match(line)
        if m:
            guard.extend(g for g in m.groups() if g)
            return
        m = None if line.rstrip().endswith("\\") else _DEFINE.match(line)
        if m and (m.group(2) or (not m.group(3) and m.group(1) in guard)):
            return                                # a function-like macro, or the include guard
        if not m or not m.group(1).startswith("SAST_"):
            raise RuntimeError(f"sast_hip.h: cannot place the preprocessor line {line!r}")
        new(constants, m.group(1), _int(m.group(3), m.group(1)))

    def enum(body):
        value = -1
        for item in filter(None, (i.strip() for i in body.split(","))):
            m = re.fullmatch(r"(SAST_\w+)(?:\s*=\s*(\w+)(?:\s*<<\s*(\w+))?)?", item)
            if not m:
                raise RuntimeError(f"sast_hip.h: cannot read the enum member {item!r}")
            name, a, b = m.groups()
            value = value + 1 if a is None else _int(a, name) << (_int(b, name) if b else 0)
            new(constants, name, value)

    def struct(_tag, body, name):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            first, *more = decl.split(",")
            ctext, fname, dim = split_name(first, name)
            declarators = [(ctext, fname, dim)]
            base = ctext.rstrip("* ")                 # 'float *a, *b': every declarator carries its own stars
            for part in more:
                m = re.fullmatch(r"([\s*]*)(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*", part)
                if not m or "*" in base:
                    raise RuntimeError(f"sast_hip.h: {name}: cannot read {decl!r}")
                declarators.append((base + m.group(1).replace(" ", ""), m.group(2), m.group(3)))
            for ctext, fname, dim in declarators:
                ct = ctype(ctext, f"{name}.{fname}")
                if dim is not None:
                    ct = ct * (constants[dim] if dim in constants else _int(dim, f"{name}.{fname}[]"))
                fields.append(Field(fname, ctext, ct))
        new(structs, name, type(name, (C.Structure,), {"_fields_": [(f.name, f.ctype) for f in fields], "c_fields": tuple(fields)}))

    def proto(ret, name, args):
        ret, args = " ".join(ret.split()), args.strip()
        out = []
        for a in ([] if args == "void" else args.split(",")):
            ctext, _aname, dim = split_name(a, name)
            if dim is not None:
                raise RuntimeError(f"sast_hip.h: {name}: array argument {a.strip()!r}")
            out.append(Arg(ctext, ctype(ctext, name)))
        new(protos, name, Proto(name, ret, None if ret == "void" else ctype(ret, name), tuple(out)))

    guard, depth, pos = [], 0, 0
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos == len(text):
            break
        for kind, rx in _ITEMS:
            m = rx.match(text, pos)
            if m:
                break
        else:
            raise RuntimeError(f"sast_hip.h: cannot place {re.match(r'[^;{}]*[;{}]?', text[pos:]).group(0).strip()!r}")
        if kind == "directive":
            directive(m.group(0))
        elif kind == "bracket":
            depth += 1 if m.group(0) != "}" else -1
            if depth < 0:
                raise RuntimeError("sast_hip.h: cannot place '}'")
        elif kind == "handle":
            new(handles, m.group(1), C.c_void_p)
        else:
            {"enum": enum, "struct": struct, "proto": proto}[kind](*m.groups())
        pos = m.end()
    if depth:
        raise RuntimeError('sast_hip.h: extern "C" { is not closed')
    return Header(constants, structs, protos)
