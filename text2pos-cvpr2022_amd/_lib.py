"""ctypes binding of libt2p_hip.so (C ABI: include/t2p.h and its extensions include/t2p_serve.h, include/t2p_select.h).

The product path has no CPU fallback: if the HIP library is missing or fails a call, this raises.
torch is imported first so that the library binds to the HIP runtime (libamdhip64.so.7) torch already loaded --
one runtime per process, which is what makes torch's device pointers and streams valid inside the kernels.
"""
import ctypes as C
import os
import re

import torch  # noqa: F401  (must precede CDLL: shares torch's libamdhip64)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("T2P_LIB") or os.path.join(_HERE, "libt2p_hip.so")  # T2P_LIB: A/B builds of the same ABI
HEADER = os.path.join(_HERE, "..", "include", "t2p.h")   # the one statement of every signature, struct and limit
SERVE_HEADER = os.path.join(_HERE, "..", "include", "t2p_serve.h")   # the serving extension: its own version and record
SELECT_HEADER = os.path.join(_HERE, "..", "include", "t2p_select.h")   # distinct candidates: likewise


class T2PError(RuntimeError):
    pass


# The binding's type rule.  Scalars map to their ctypes twins; `const t2p_x*` to POINTER(X), so a call checks the struct it is
# handed; `char*` to c_char_p; every other pointer and t2p_stream_t to c_void_p (device pointers travel as integers).
# `double` by value is a parameter only (t2p_select.h's `sep`): no function returns one.
_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "size_t": C.c_size_t,
            "float": C.c_float, "double": C.c_double}
_POINTEES = set(_SCALARS) | {"void", "char", "double", "uint8_t", "uint16_t", "uint64_t", "t2p_stream_t"}
_DECLARATOR = re.compile(r"((?:\*\s*(?:const\b\s*)?)*)(?!const\b)(\w+)\s*(?:\[\s*(\d+)\s*\])?")


def _ctype(base, stars, structs, decl):
    if not stars and (base in _SCALARS or base == "t2p_stream_t"):
        return _SCALARS.get(base, C.c_void_p)
    if stars == 1 and base == "char":
        return C.c_char_p
    if stars == 1 and base in structs:
        return C.POINTER(structs[base])
    if stars and (base in _POINTEES or base in structs):
        return C.c_void_p
    raise T2PError(f"include/t2p.h: unknown type in `{decl}`")


def _declare(decl, structs):
    """`[const] T d1, d2`, every declarator with its own `*`s and an optional `[n]` -> [(name, ctype)]."""
    head = re.match(r"(?:const\s+)?(\w+)\b", decl)
    found = [_DECLARATOR.fullmatch(d.strip()) for d in decl[head.end():].split(",")] if head else [None]
    if not all(found):
        raise T2PError(f"include/t2p.h: cannot read the declaration `{decl}`")
    types = [_ctype(head.group(1), m.group(1).count("*"), structs, decl) for m in found]
    return [(m.group(2), t * int(m.group(3)) if m.group(3) else t) for m, t in zip(found, types)]


def parse_header(text):
    """(defines, structs, symbols) of a header in t2p.h's dialect of C: integer `#define T2P_*`, `typedef struct` of scalars,
    pointers and small arrays, and prototypes.  Anything else raises T2PError naming the declaration; nothing is guessed."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {m.group(1): int(m.group(2) or m.group(3), 0) for m in re.finditer(
        r"^[ \t]*#[ \t]*define[ \t]+(T2P_\w+)[ \t]+(?:\((-\d+)\)|(0[xX][0-9a-fA-F]+|\d+))[ \t]*$", text, re.M)}
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    text = re.sub(r'extern\s+"C"\s*\{(.*)\}', r"\1", text, flags=re.S)
    structs, symbols = {}, {}

    def struct(m):
        decls = [d.strip() for d in m.group(1).split(";")]
        if decls.pop() or not decls:
            raise T2PError(f"include/t2p.h: cannot read the body of struct `{m.group(2)}`")
        fields = [f for d in decls for f in _declare(" ".join(d.split()), structs)]
        name = "".join(part.capitalize() for part in m.group(2).split("_")[1:])
        structs[m.group(2)] = type(name, (C.Structure,), {"_fields_": fields})
        return ""

    text = re.sub(r"typedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    for stmt in (" ".join(s.split()) for s in text.split(";")):
        if stmt in ("", "typedef void* t2p_stream_t"):
            continue
        m = re.fullmatch(r"(?:const )?(\w+) ?(\**) ?\b(t2p_\w+) ?\((.*)\)", stmt)
        if not m:
            raise T2PError(f"include/t2p.h: cannot read the declaration `{stmt}`")
        base, stars, name, params = m.groups()
        if (base, stars) == ("double", ""):
            raise T2PError(f"include/t2p.h: unknown type in `{stmt}`")
        res = None if (base, stars) == ("void", "") else _ctype(base, len(stars), structs, stmt)
        args = [t for p in params.split(",") if params != "void" for _, t in _declare(p.strip(), structs)]
        if any(issubclass(t, C.Array) for t in args):
            raise T2PError(f"include/t2p.h: array parameter in `{stmt}`")
        symbols[name] = (res, args)
    return defines, structs, symbols


with open(HEADER) as _f:
    DEFINES, STRUCTS, SYMBOLS = parse_header(_f.read())   # SYMBOLS: name -> (restype, argtypes)
ABI_VERSION = DEFINES["T2P_ABI_VERSION"]
CellWeights, CellConfig, CellTrace, MatchWeights, TextWeights = (
    STRUCTS["t2p_" + n] for n in ("cell_weights", "cell_config", "cell_trace", "match_weights", "text_weights"))

with open(SERVE_HEADER) as _f:    # same dialect, same parser; t2p.h's structs are not repeated there
    SERVE_DEFINES, _serve_structs, SERVE_SYMBOLS = parse_header(_f.read())
if _serve_structs or set(SERVE_SYMBOLS) & set(SYMBOLS):
    raise T2PError("include/t2p_serve.h: declares a struct or repeats a symbol of include/t2p.h")
SERVE_ABI_VERSION = SERVE_DEFINES["T2P_SERVE_ABI_VERSION"]

with open(SELECT_HEADER) as _f:
    SELECT_DEFINES, _select_structs, SELECT_SYMBOLS = parse_header(_f.read())
if _select_structs or set(SELECT_SYMBOLS) & (set(SYMBOLS) | set(SERVE_SYMBOLS)):
    raise T2PError("include/t2p_select.h: declares a struct or repeats a symbol of include/t2p.h or include/t2p_serve.h")
SELECT_ABI_VERSION = SELECT_DEFINES["T2P_SELECT_ABI_VERSION"]

_lib = None


def lib() -> C.CDLL:
    """Load libt2p_hip.so (once).  Raises if it has not been built -- there is no fallback path."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise T2PError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                "(python __graft_entry__.py build, or python text2pos-cvpr2022_amd/build.py)")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in list(SYMBOLS.items()) + list(SERVE_SYMBOLS.items()) + list(SELECT_SYMBOLS.items()):
            fn = getattr(handle, name)  # AttributeError if the export is missing
            fn.restype, fn.argtypes = res, args
        if handle.t2p_abi_version() != ABI_VERSION:
            raise T2PError(f"libt2p_hip.so ABI {handle.t2p_abi_version()} != binding ABI {ABI_VERSION}")
        if handle.t2p_serve_abi_version() != SERVE_ABI_VERSION:
            raise T2PError(f"libt2p_hip.so serve ABI {handle.t2p_serve_abi_version()} != binding serve ABI {SERVE_ABI_VERSION}")
        if handle.t2p_select_abi_version() != SELECT_ABI_VERSION:
            raise T2PError(f"libt2p_hip.so select ABI {handle.t2p_select_abi_version()} != binding select ABI {SELECT_ABI_VERSION}")
        _lib = handle
    return _lib


def check(rc: int, what: str):
    if rc != 0:
        msg = lib().t2p_last_error().decode("utf-8", "replace")
        raise T2PError(f"{what} failed (rc={rc}): {msg}")
