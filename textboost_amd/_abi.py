"""The ctypes tables of libtextboost_hip.so, read from include/textboost_hip.h (its opening comment states the subset of C this understands).
Anything outside that subset raises with the declaration's text: a guessed type would be a wrong pointer handed to a kernel."""
from __future__ import annotations

import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "textboost_hip.h")

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float, "double": C.c_double}
_POINTEES = set(_SCALARS) | {"void", "char", "uint8_t"}

_DECL = re.compile(r"""\s*(?:
      typedef\s+struct\s*\w*\s*\{(?P<fields>[^{}]*)\}\s*(?P<struct>\w+)
    | enum\s*\{(?P<enum>[^{}]*)\}
    | typedef\s+(?P<aliased>[^;{}()]+?)\b(?P<alias>\w+)
    | (?P<ret>[^;{}()]+?)\b(?P<fn>\w+)\s*\((?P<params>[^;{}()]*)\)
    )\s*;""", re.X)


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _ctype(ctype, types, decl, where):
    """the ctypes type of the C type `ctype`; where = "param" | "field" | "return" """
    words = ctype.replace("*", " * ").split()
    stars = words.count("*")
    base = [w for w in words if w not in ("const", "*")]
    name = base[0] if len(base) == 1 else None
    if not (name in types or (stars and name in _POINTEES) or (name == "void" and where == "return")):
        raise ValueError(f"include/textboost_hip.h: unknown type {ctype.strip()!r} in: {decl.strip()}")
    t = types.get(name)
    if not stars:
        if t is not None and issubclass(t, C.Structure):
            raise ValueError(f"include/textboost_hip.h: struct passed by value in: {decl.strip()}")
        return t   # None: a void return
    if stars == 1 and t is not None and issubclass(t, C.Structure):
        return C.POINTER(t)
    if where == "return" and name == "char":
        return C.c_char_p
    if where == "field" and stars == 1 and name == "int32_t":   # a HOST int the library writes: callers assign ctypes.pointer(c_int32)
        return C.POINTER(C.c_int32)
    return C.c_void_p   # device pointers (callers pass _lib.ptr(tensor)) and host arrays / byref() results alike


def _named(decl, whole):
    """'const void* x' -> ('const void* ', 'x')"""
    m = re.fullmatch(r"(.+?)\b(\w+)", decl.strip(), re.S)
    if not m:
        raise ValueError(f"include/textboost_hip.h: cannot read {decl.strip()!r} in: {whole.strip()}")
    return m[1], m[2]


def parse(text):
    """header text -> (structs {C name: ctypes.Structure class}, sigs {name: ([argtypes], restype)}, constants {name: int})"""
    text = strip_comments(text)
    consts = {m[1]: int(m[2]) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(-?\d+)[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    types, structs, sigs = dict(_SCALARS), {}, {}
    pos = 0
    while text[pos:].strip():
        m = _DECL.match(text, pos)
        if not m:
            raise ValueError(f"include/textboost_hip.h: cannot classify the declaration at: {text[pos:].strip()[:120]!r}")
        pos, decl = m.end(), m[0]
        if m["struct"]:
            fields = []
            for f in filter(str.strip, m["fields"].split(";")):
                first, *more = f.split(",")
                ctype, name = _named(first, f)
                if not all(re.fullmatch(r"\s*\w+\s*", n) for n in more):
                    raise ValueError(f"include/textboost_hip.h: cannot read the declarators of: {f.strip()}")
                fields += [(n.strip(), _ctype(ctype, types, f, "field")) for n in [name] + more]
            types[m["struct"]] = structs[m["struct"]] = type(m["struct"], (C.Structure,), {"_fields_": fields})
        elif m["enum"] is not None:
            for e in filter(str.strip, m["enum"].split(",")):
                em = re.fullmatch(r"\s*(\w+)\s*=\s*(-?\d+)\s*", e)
                if not em:
                    raise ValueError(f"include/textboost_hip.h: enumerator without an explicit value {e.strip()!r} in: {decl.strip()}")
                consts[em[1]] = int(em[2])
        elif m["alias"]:
            types[m["alias"]] = _ctype(m["aliased"], types, decl, "param")
        else:
            params = [] if m["params"].strip() == "void" else m["params"].split(",")
            sigs[m["fn"]] = ([_ctype(_named(p, decl)[0], types, decl, "param") for p in params], _ctype(m["ret"], types, decl, "return"))
    return structs, sigs, consts


def load(path=HEADER):
    if not os.path.exists(path):
        raise RuntimeError(f"{os.path.normpath(path)} is missing: the ctypes binding of libtextboost_hip.so is derived from it")
    with open(path) as f:
        return parse(f.read())
