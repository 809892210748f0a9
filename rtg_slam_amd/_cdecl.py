"""Reads the C declarations of include/*.h into ctypes: struct mirrors, function prototypes, integer constants.

It understands the small C subset that the comment at the top of include/rtgs_raster.h states, and raises `CDeclError`
on anything else rather than guess.  The one rule for a type: a scalar maps exactly; a struct by value (members only)
to its mirror; a pointer to a known struct to POINTER(mirror); a callback typedef to its CFUNCTYPE; a `const char*`
result to c_char_p; every other pointer - `void*`, `float*`, `int64_t*`, the opaque `rtgs_ctx*` - to c_void_p."""
from __future__ import annotations

import ctypes as C
import re

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint8_t": C.c_uint8, "uint16_t": C.c_uint16,
           "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double}
_DIRECTIVES = ("ifndef", "define", "include", "endif")          # the C++ guards are cut out as whole blocks first
_DEFINE = re.compile(r"define\s+(RTGS_\w+)\s+(.+)")
_INTEGER = re.compile(r"\(?\s*(-?\d+)\s*\)?(?:LL)?")
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)")
_OPAQUE = re.compile(r"typedef\s+struct\s+(\w+)\s+(\w+)")
_CALLBACK = re.compile(r"typedef\s+([\w\s*]+?)\(\s*\*\s*(\w+)\s*\)\s*\(([^()]*)\)")
_FUNCTION = re.compile(r"([\w\s*]+?)\b(rtgs_\w+)\s*\(([^()]*)\)")
_TYPED = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w*)")      # a parameter or a result: type, stars, name
_MEMBER = re.compile(r"(?:const\s+)?(\w+)\s*(.*)", re.S)
_DECLARATOR = re.compile(r"(\**)\s*(\w+)")


class CDeclError(ValueError):
    pass


class Declarations:
    """structs: C name -> ctypes.Structure class; callbacks: typedef name -> CFUNCTYPE; opaque: names of forward-declared
    structs; functions: name -> (restype, argtypes); constants: RTGS_NAME -> int.  `read` may be called once per header."""

    def __init__(self):
        self.structs, self.callbacks, self.opaque, self.functions, self.constants = {}, {}, set(), {}, {}

    def _ctype(self, base, stars, what, result=False, member=False):
        if stars:
            if base in self.structs and stars == 1:
                return C.POINTER(self.structs[base])
            if base == "char" and stars == 1 and result:
                return C.c_char_p
            if base in SCALARS or base in self.structs or base in self.opaque or base == "void":
                return C.c_void_p
        elif base in SCALARS:
            return SCALARS[base]
        elif base in self.callbacks:
            return self.callbacks[base]
        elif base == "void" and result:
            return None
        elif base in self.structs and member:
            return self.structs[base]
        raise CDeclError(f"unknown type in {what!r}")

    def _typed(self, text, result=False):
        m = _TYPED.fullmatch(text.strip())
        if not m or (result and m.group(3)):
            raise CDeclError(f"cannot read {text.strip()!r}")
        return self._ctype(m.group(1), m.group(2).count("*"), text.strip(), result=result)

    def _signature(self, result, params):
        params = params.strip()
        return self._typed(result, result=True), [] if params == "void" else [self._typed(p) for p in params.split(",")]

    def _struct(self, name, body):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            head = _MEMBER.fullmatch(decl)
            for d in head.group(2).split(",") if head else [""]:
                m = _DECLARATOR.fullmatch(d.strip())
                if not m:                                        # a bit-field, an array, a type of several words ...
                    raise CDeclError(f"cannot read member {decl!r} of {name}")
                fields.append((m.group(2), self._ctype(head.group(1), len(m.group(1)), decl, member=True)))
        self.structs[name] = type(name, (C.Structure,), {"_fields_": fields, "__doc__": f"`{name}` of include/*.h"})

    def read(self, text):
        text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
        text = re.sub(r"#\s*ifdef\s+__cplusplus\b.*?#\s*endif", " ", text, flags=re.S)
        for word, rest in re.findall(r"^[ \t]*#[ \t]*(\w*)(.*)$", text, flags=re.M):
            if word not in _DIRECTIVES:
                raise CDeclError(f"directive outside the subset: #{word}{rest}")
            m = _DEFINE.fullmatch((word + rest).strip())
            if m:
                value = _INTEGER.fullmatch(m.group(2).strip())
                if not value:
                    raise CDeclError(f"#define {m.group(1)} is not an integer")
                self.constants[m.group(1)] = int(value.group(1))
        text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
        statements, depth, start = [], 0, 0
        for i, ch in enumerate(text):                            # split at the semicolons outside braces
            depth += (ch == "{") - (ch == "}")
            if ch == ";" and depth == 0:
                statements.append(text[start:i].strip())
                start = i + 1
        if depth != 0 or text[start:].strip():
            raise CDeclError(f"unterminated declaration: {text[start:].strip()[:60]!r}")
        for s in statements:
            if (m := _STRUCT.fullmatch(s)) and m.group(1) == m.group(3):
                self._struct(m.group(1), m.group(2))
            elif (m := _OPAQUE.fullmatch(s)) and m.group(1) == m.group(2):
                self.opaque.add(m.group(1))
            elif m := _CALLBACK.fullmatch(s):
                res, args = self._signature(m.group(1), m.group(3))
                self.callbacks[m.group(2)] = C.CFUNCTYPE(res, *args)
            elif m := _FUNCTION.fullmatch(s):
                self.functions[m.group(2)] = self._signature(m.group(1), m.group(3))
            else:
                raise CDeclError(f"cannot read declaration {s[:80]!r}")
        return self
