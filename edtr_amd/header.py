"""Reader of include/edtr_hip.h: the structs, constants and prototypes that edtr_amd/lib.py binds with ctypes, so that the
header is the only place where the C ABI is written down.  Standard library only (tools/hipfree.py must start without torch).

The header keeps to a narrow dialect and this reader accepts nothing else (HeaderError quotes the offending line): block
comments; the include guard, `#include`, `#ifdef __cplusplus` / `extern "C"`; `#define NAME <integer expression>`; `enum` with
explicit values; `typedef struct edtr_x { ... } edtr_x;` of scalar and pointer fields; prototypes; `typedef void* edtr_stream_t;`."""
from __future__ import annotations

import ctypes as C
import re
from collections import namedtuple

SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float,
           "edtr_stream_t": C.c_void_p}
POINTEES = set(SCALARS) | {"void", "char", "double", "uint8_t", "uint32_t"}          # and every struct declared above the use

# c: the C spelling ("const float*"); base: the type name; ptr: the number of `*`; ctype: of a scalar, None for a pointer
CType = namedtuple("CType", "c base ptr ctype")
Header = namedtuple("Header", "structs constants functions")    # {struct: [(field, CType)]}, {NAME: int}, {fn: (CType, [(param, CType)])}

_DECL = r"\s*(const\s+)?(\w+)\b\s*((?:\*\s*(?:const\b\s*)?)*)"      # [const] base [* [const] *...]
_NAMES = re.compile(_DECL + r"(\w+(?:\s*,\s*\w+)*)\s*")             # ... a, b, c
_PROTO = re.compile(_DECL + r"(edtr_\w+)\s*\(([^()]*)\)\s*")
_SPACE, _DIRECTIVE, _LINKAGE = re.compile(r"\s*"), re.compile(r"#[^\n]*"), re.compile(r'extern\s+"C"\s*\{|\}')
_STATEMENT = re.compile(r"[^;{}#]*(?:\{[^{}#]*\}[^;{}#]*)?;")       # up to its `;`, with at most one flat `{ ... }` inside


class HeaderError(ValueError):
    pass


def int_expr(text: str) -> int:
    """Value of an expression of integers, parentheses and `<<` (all the header uses); ValueError for anything else."""
    toks = re.findall(r"-?\d+|<<|[()]|\S+", text)

    def atom() -> int:
        t = toks.pop(0) if toks else ""
        if t == "(":
            v = shift()
            if not toks or toks.pop(0) != ")":
                raise ValueError(text)
            return v
        if not re.fullmatch(r"-?\d+", t):
            raise ValueError(text)
        return int(t)

    def shift() -> int:
        v = atom()
        while toks and toks[0] == "<<":
            toks.pop(0)
            v <<= atom()
        return v

    v = shift()
    if toks:
        raise ValueError(text)
    return v


def parse(text: str) -> Header:
    text = re.sub(r"/\*.*?\*/", lambda m: " " + "\n" * m.group().count("\n"), text, flags=re.S)       # keeps every line number
    structs, constants, functions = {}, {}, {}

    def fail(pos: int, why: str):
        pos = _SPACE.match(text, pos).end()
        n = text.count("\n", 0, pos)
        raise HeaderError(f"edtr_hip.h:{n + 1}: {why}: {text.splitlines()[n].strip()!r}")

    def ctype(m: re.Match, pos: int) -> CType:
        const, base, stars = m.group(1), m.group(2), m.group(3)
        ptr = stars.count("*")
        if not (base in POINTEES or base in structs if ptr else base in SCALARS):
            fail(pos, f"unknown type {base!r}")
        return CType(("const " if const else "") + base + " ".join(stars.split()), base, ptr, None if ptr else SCALARS[base])

    def constant(name: str, value: str, pos: int):
        try:
            constants[name] = int_expr(value)
        except ValueError:
            fail(pos, f"{name} is not an integer expression")

    def pieces(body: str, at: int, sep: str):          # (offset in text, piece) of the non-blank sep-separated pieces
        return [(at + m.start(), m.group()) for m in re.finditer(f"[^{sep}]+", body) if m.group().strip()]

    def declarations(body: str, at: int, sep: str, what: str):      # [(name, CType)] of struct fields (`;`) or parameters (`,`)
        out = []
        for at, item in pieces(body, at, sep):
            d = _NAMES.fullmatch(item)
            if not d:
                fail(at, f"not a scalar or pointer {what}")
            out += [(name.strip(), ctype(d, at)) for name in d.group(4).split(",")]
        return out

    pos = 0
    while (pos := _SPACE.match(text, pos).end()) < len(text):
        if m := _DIRECTIVE.match(text, pos):
            d = re.fullmatch(r"#define\s+(EDTR_\w+)(.*)", m.group().strip())
            if d and (d.group(2).strip() or not d.group(1).endswith("_H")):     # the include guard has no value
                constant(d.group(1), d.group(2), pos)
            elif not d and not re.match(r"#(include|ifndef|ifdef|endif)\b", m.group()):
                fail(pos, "unknown directive")
            pos = m.end()
            continue
        if m := _LINKAGE.match(text, pos):
            pos = m.end()
            continue
        st = _STATEMENT.match(text, pos)
        if not st:
            fail(pos, "not a declaration of the dialect")
        s = st.group()[:-1]
        if m := re.fullmatch(r"enum\s+\w+\s*\{(.*)\}\s*", s, re.S):
            for at, item in pieces(m.group(1), pos + m.start(1), ","):
                e = re.fullmatch(r"\s*(EDTR_\w+)\s*=(.*)", item, re.S)
                if not e:
                    fail(at, "enumerator without an explicit value")
                constant(e.group(1), e.group(2), at)
        elif m := re.fullmatch(r"typedef\s+struct\s+(\w+)\s*\{(.*)\}\s*(\w+)\s*", s, re.S):
            if m.group(1) != m.group(3):
                fail(pos, "struct tag and typedef name differ")
            structs[m.group(1)] = declarations(m.group(2), pos + m.start(2), ";", "field")
        elif m := _PROTO.fullmatch(s):
            params = [] if m.group(5).strip() == "void" else declarations(m.group(5), pos + m.start(5), ",", "parameter")
            functions[m.group(4)] = (ctype(m, pos), params)
        elif not re.fullmatch(r"typedef\s+void\s*\*\s*edtr_stream_t\s*", s):
            fail(pos, "not a declaration of the dialect")
        pos = st.end()
    named = set(re.findall(r"\b(edtr_[a-z0-9_]+)\s*\(", text))
    if named != set(functions):
        raise HeaderError(f"edtr_hip.h: {sorted(named ^ set(functions))} named with `(` but not parsed as prototypes")
    return Header(structs, constants, functions)
