"""Reader of the C subset that ``include/mit_hip.h`` is written in, into ctypes.

It understands exactly what that header uses — comments, the include guard, the ``extern "C"`` block, ``#define NAME <integer>``, enums
with explicit values, ``typedef struct X { ... } X;`` and plain prototypes — and raises ``HeaderError`` naming the text on anything
else: a binding that silently skipped a declaration would be worse than none.
"""
from __future__ import annotations

import ctypes as C
import re


class HeaderError(ValueError):
    pass


SCALARS = {"char": C.c_char, "short": C.c_short, "int": C.c_int, "unsigned": C.c_uint, "float": C.c_float, "double": C.c_double,
           "int8_t": C.c_int8, "int16_t": C.c_int16, "int32_t": C.c_int32, "int64_t": C.c_int64,
           "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64}

_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"
_ITEMS = [
    ("cpp", re.compile(r'#[ \t]*(?:ifn?def[ \t]+\w+|endif|include[ \t]*<[\w./]+>|define[ \t]+(\w+)(?:[ \t]+(%s))?)[ \t]*$' % _INT, re.M)),
    ("extern", re.compile(r'extern\s+"C"\s*\{')),
    ("close", re.compile(r"\}")),
    ("enum", re.compile(r"enum\s+\w+\s*\{([^{}]*)\}\s*;")),
    ("struct", re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")),
    ("func", re.compile(r"((?:const\s+)?\w+\b\s*\*?)\s*(\w+)\s*\(([^(){};]*)\)\s*;")),
]
_SPACE = re.compile(r"\s*")
_DECL = re.compile(r"(?:const\s+)?(\w+)\b\s*(.*)", re.S)
_DECLARATOR = re.compile(r"(\*?)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?")


def parse(text: str):
    """Header text -> ``(constants, structs, functions, enums)``: ``#define`` name -> int, struct name -> ``ctypes.Structure`` class,
    function name -> ``(restype, argtypes)``, enumerator name -> int.

    The one pointer rule of the binding: ``char *`` is ``c_char_p``, every other pointer (parameter, return value or field; to a struct, a
    scalar or ``void``) is ``c_void_p``, which takes None, an integer address, ``byref(...)``, ``pointer(...)`` and ctypes arrays alike."""
    constants, structs, functions, enums = {}, {}, {}, {}

    def ctype(base: str, pointer: bool, extent, what: str, void_ok: bool = False):
        if base in SCALARS or base in structs:
            t = (C.c_char_p if base == "char" else C.c_void_p) if pointer else SCALARS.get(base) or structs[base]
        elif base == "void" and (pointer or void_ok):
            t = C.c_void_p if pointer else None
        else:
            raise HeaderError(f"unknown type {base!r} in {what!r}")
        if extent is None:
            return t
        if not re.fullmatch(_INT, extent) and extent not in constants:
            raise HeaderError(f"array extent {extent!r} is neither an integer nor a #define in {what!r}")
        return t * (constants[extent] if extent in constants else int(extent, 0))

    def declarators(decl: str):
        """``const T *a, b[4]`` -> [(name, ctype), ...]"""
        decl = decl.strip()
        m = _DECL.fullmatch(decl)
        out = []
        for d in m.group(2).split(",") if m else [""]:
            dm = _DECLARATOR.fullmatch(d.strip())
            if not dm:
                raise HeaderError(f"cannot read the declaration {decl!r}")
            out.append((dm.group(2), ctype(m.group(1), bool(dm.group(1)), dm.group(3), decl)))
        return out

    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    pos, open_blocks = 0, 0
    while True:
        pos = _SPACE.match(text, pos).end()
        if pos == len(text):
            break
        for kind, rx in _ITEMS:
            m = rx.match(text, pos)
            if m:
                break
        else:
            raise HeaderError(f"cannot read the declaration at {text[pos:pos + 80].splitlines()[0]!r}")
        pos = m.end()
        if kind == "cpp" and m.group(2) is not None:
            constants[m.group(1)] = int(m.group(2), 0)
        elif kind in ("extern", "close"):
            open_blocks += 1 if kind == "extern" else -1
            if open_blocks < 0:
                raise HeaderError("unbalanced '}'")
        elif kind == "enum":
            for item in filter(None, (s.strip() for s in m.group(1).split(","))):
                em = re.fullmatch(r"(\w+)\s*=\s*(%s)" % _INT, item)
                if not em:
                    raise HeaderError(f"enumerator without an explicit integer value: {item!r}")
                enums[em.group(1)] = int(em.group(2), 0)
        elif kind == "struct":
            name, body, alias = m.groups()
            if name != alias or name in structs:
                raise HeaderError(f"typedef struct {name} is named {alias}, or declared twice")
            fields = [f for decl in body.split(";") if decl.strip() for f in declarators(decl)]
            structs[name] = type(name, (C.Structure,), {"_fields_": fields})
        elif kind == "func":
            ret, name, params = m.groups()
            if "[" in params or name in functions:
                raise HeaderError(f"array parameter in the prototype of {name}, or a second prototype of it: {params.strip()!r}")
            params = [] if params.strip() in ("", "void") else [declarators(p) for p in params.split(",")]
            restype = ctype(_DECL.fullmatch(ret).group(1), ret.endswith("*"), None, m.group(0), void_ok=True)
            functions[name] = (restype, [p[0][1] for p in params])
    if open_blocks:
        raise HeaderError('unclosed extern "C" block')
    return constants, structs, functions, enums
