"""The C ABI of libsplatt3r_hip.so as ctypes, read from include/*.h.

The headers are the only place an entry point, an argument struct or a
constant of the ABI is written down; this module is their only reader:

  functions   name -> (return type, [parameter types])
  structs     typedef name -> generated ctypes.Structure (C field names)
  constants   integer #defines and enumerators -> int

The headers are plain C in a closed vocabulary and the mapping is fixed:
scalars map to their ctypes namesake, an enum to c_int, a `const char*`
return to c_char_p, a pointer to an ABI struct to POINTER(that struct), every
other pointer (to a scalar, to void, to a pointer) to c_void_p, which takes
the integer addresses, None, ctypes arrays and byref() objects the call sites
pass.  Anything else is a ValueError naming the header and the line: the
fix is a plainer header, not a larger parser.

Imports neither torch nor the library.
"""
from __future__ import annotations

import ctypes
import glob
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__)))), "include")

_SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double,
            "size_t": ctypes.c_size_t, "unsigned long long": ctypes.c_ulonglong}
_SCALARS.update({f"{u}int{b}_t": getattr(ctypes, f"c_{u}int{b}")
                 for u in ("", "u") for b in (8, 16, 32, 64)})
_POINTEES = ("void", "char")        # complete only behind a '*'
_TYPE_WORDS = set(" ".join([*_SCALARS, *_POINTEES, "const"]).split())

# one top-level statement: a declaration, or `... { body } name;`
_STMT = re.compile(r"(?P<head>[^;{}]*)(?:\{(?P<body>[^{}]*)\}(?P<tail>[^;{}]*))?;")
_SPACE = re.compile(r"\s*")
_TOKEN = re.compile(r"\w+|\*|\S")
_FUNCTION = re.compile(r"(.+?)\b(\w+)\s*\((.*)\)\s*", re.S)
_DECLARATOR = re.compile(r"(.*?)\b(\w+)\s*(?:\[\s*(\w+)\s*\])?", re.S)
_DEFINE = re.compile(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(.+?)[ \t]*$", re.M)
_CPLUSPLUS = re.compile(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b[^\n]*$",
                        re.S | re.M)


def _blank(m):
    return " " + "\n" * m.group().count("\n")     # line numbers survive


class Headers:
    """What a set of headers declares (see the module docstring)."""

    def __init__(self):
        self.functions: dict = {}
        self.structs: dict = {}
        self.constants: dict = {}
        self._enums: set = set()
        self._loaded: set = set()

    def load(self, path: str) -> None:
        """Parse a header file once, the headers it #includes "..." first."""
        path = os.path.abspath(path)
        if path in self._loaded:
            return
        self._loaded.add(path)
        with open(path) as f:
            text = f.read()
        for inc in re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', text, re.M):
            self.load(os.path.join(os.path.dirname(path), inc))
        self.parse(text, os.path.basename(path))

    def parse(self, text: str, header: str = "<text>") -> None:
        text = re.sub(r"/\*.*?\*/", _blank, text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        text = _CPLUSPLUS.sub(_blank, text)
        for name, value in _DEFINE.findall(text):
            if (value := self._int(value)) is not None:
                self.constants[name] = value
        text = re.sub(r"^[ \t]*#[^\n]*$", _blank, text, flags=re.M)
        pos = 0
        while True:
            pos = _SPACE.match(text, pos).end()
            if pos == len(text):
                break
            where = f"{header}:{text.count(chr(10), 0, pos) + 1}"
            m = _STMT.match(text, pos)
            if not m:
                raise ValueError(f"{where}: cannot parse")
            pos = m.end()
            head, body, tail = m.group("head"), m.group("body"), (m.group("tail") or "").strip()
            kind = head.split()
            if body is None:
                self._function(head, where)
            elif kind[:1] == ["enum"] and not tail:
                self._enum(body, where)
            elif kind[:2] == ["typedef", "enum"] and re.fullmatch(r"\w+", tail):
                self._enum(body, where)
                self._enums.add(tail)
            elif kind[:2] == ["typedef", "struct"] and re.fullmatch(r"\w+", tail):
                self._struct(tail, body, header, text.count("\n", 0, m.start("body")) + 1)
            else:
                raise ValueError(f"{where}: cannot parse '{' '.join(kind)} {{...}} {tail}'")

    def _int(self, text: str):
        """An integer literal, a known constant, or `a << b` of two such,
        in parentheses or not; None for anything else."""
        m = re.fullmatch(r"\(?\s*(\w+)\s*(?:<<\s*(\w+)\s*)?\)?", text.strip())
        try:
            a, b = (self.constants[w] if w in self.constants else int(w, 0)
                    for w in (m.group(1), m.group(2) or "0"))
        except (AttributeError, ValueError):
            return None
        return a << b

    def _ctype(self, text: str, where: str, ret: bool = False):
        words = _TOKEN.findall(text)
        stars = words.count("*")
        base = " ".join(w for w in words if w not in ("*", "const"))
        if stars == 0:
            if base in _SCALARS:
                return _SCALARS[base]
            if base in self._enums:
                return ctypes.c_int
            if base == "void" and ret:
                return None
            if base in self.structs:
                raise ValueError(f"{where}: struct '{base}' by value")
        elif stars == 1 and base in self.structs:
            return ctypes.POINTER(self.structs[base])
        elif stars == 1 and base == "char" and ret:
            return ctypes.c_char_p
        elif base in _SCALARS or base in _POINTEES or base in self._enums or base in self.structs:
            return ctypes.c_void_p
        raise ValueError(f"{where}: unknown type '{' '.join(text.split())}'")

    def _declarator(self, text: str):
        """(type text, name, array size) of `type name[size]`; the name is
        None where the text is a type alone (an unnamed parameter)."""
        m = _DECLARATOR.fullmatch(text.strip())
        word = m and m.group(2)
        if not m or word in _TYPE_WORDS or word in self._enums or word in self.structs:
            return text, None, None
        return m.groups()

    def _function(self, decl: str, where: str) -> None:
        m = _FUNCTION.fullmatch(decl)
        if not m:
            raise ValueError(f"{where}: cannot parse '{' '.join(decl.split())}'")
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        if "(" in params or "..." in params:
            raise ValueError(f"{where}: {name}: variadic or function-pointer parameter")
        args = []
        for p in params.split(",") if params not in ("", "void") else []:
            ctext, pname, dim = self._declarator(p)
            ctext = ctext if pname and ctext.strip() else p
            # an array parameter (`const float T[8]`) is a pointer
            args.append(self._ctype(ctext + ("*" if dim else ""), f"{where}: {name}"))
        sig = (self._ctype(ret, f"{where}: {name}", ret=True), args)
        if self.functions.setdefault(name, sig) != sig:
            raise ValueError(f"{where}: {name} declared twice with different signatures")

    def _enum(self, body: str, where: str) -> None:
        value = 0
        for item in filter(str.strip, body.split(",")):
            name, eq, text = (s.strip() for s in item.partition("="))
            value = self._int(text) if eq else value
            if value is None or not re.fullmatch(r"[A-Za-z_]\w*", name):
                raise ValueError(f"{where}: cannot parse enumerator '{item.strip()}'")
            self.constants[name] = value
            value += 1

    def _struct(self, name: str, body: str, header: str, line: int) -> None:
        fields = []
        for decl in body.split(";"):
            lead = len(decl) - len(decl.lstrip())
            where = f"{header}:{line + decl.count(chr(10), 0, lead)}: {name}"
            line += decl.count("\n")
            if not decl.strip():
                continue
            first, *more = decl.split(",")
            ctext, fname, dim = self._declarator(first)
            if fname is None or not ctext.strip():
                raise ValueError(f"{where}: cannot parse field '{' '.join(decl.split())}'")
            if more and "*" in ctext:
                raise ValueError(f"{where}: pointer type in a multi-declarator")
            ctype = self._ctype(ctext, where)
            for none, fname, dim in [("", fname, dim)] + [self._declarator(d) for d in more]:
                count = None if dim is None else self._int(dim)
                if fname is None or none.strip() or (dim is not None and count is None):
                    raise ValueError(f"{where}: cannot parse field '{' '.join(decl.split())}'")
                fields.append((fname, ctype if dim is None else ctype * count))
        self.structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})


if not os.path.isdir(INCLUDE):
    raise ImportError(f"splatt3r-slam_amd ABI headers not found: {INCLUDE}")
_headers = Headers()
for _h in sorted(glob.glob(os.path.join(INCLUDE, "*.h"))):
    _headers.load(_h)
functions, structs, constants = _headers.functions, _headers.structs, _headers.constants
