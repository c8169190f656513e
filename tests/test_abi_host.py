"""The C ABI is stated once, in include/t2p.h; _lib.py reads it.  Checked here, for every export and struct at once:
the generated ctypes layouts against the host C compiler's, the generated binding against its recorded form
(tests/golden/abi.json), the constructs the parser refuses, and the built library against the header."""
import ctypes as C
import json
import os
import shutil
import subprocess

import pytest

from text2pos_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "tests", "golden", "abi.json")
_KINDS = {None: "void", C.c_int32: "int32", C.c_int64: "int64", C.c_uint32: "uint32", C.c_size_t: "size_t", C.c_float: "float",
          C.c_char_p: "char*"}


def _kind(t, structs):
    """One word per ctypes type; every pointer that is not a `const t2p_x*` is "ptr", whatever class the binding gives it."""
    if t in _KINDS:
        return _KINDS[t]
    target = getattr(t, "_type_", None)
    return {cls: cname + "*" for cname, cls in structs.items()}.get(target, "ptr")


def abi_record(lib=_lib, structs=None):
    """What tests/golden/abi.json holds.  To regenerate: json.dump(abi_record(), open(RECORD, "w"), indent=0, sort_keys=True)."""
    structs = structs or lib.STRUCTS
    fields = lambda cls: [[n, _kind(getattr(t, "_type_", t) if issubclass(t, C.Array) else t, structs),
                           t._length_ if issubclass(t, C.Array) else 0] for n, t in cls._fields_]
    return {"version": lib.ABI_VERSION,
            "structs": {cname: fields(cls) for cname, cls in structs.items()},
            "symbols": {name: [_kind(res, structs)] + [_kind(a, structs) for a in args] for name, (res, args) in lib.SYMBOLS.items()}}


def _host_cc():
    for cc in ("cc", "gcc", "clang", "/opt/rocm/llvm/bin/clang", "/opt/rocm/lib/llvm/bin/clang"):
        if shutil.which(cc):
            return shutil.which(cc)
    return None


def test_struct_layouts_match_the_host_compiler(tmp_path):
    cc = _host_cc()
    if cc is None:
        pytest.skip("no host C compiler")
    lines = ['#include <stdio.h>', '#include "t2p.h"', "int main(void) {"]
    for cname, cls in _lib.STRUCTS.items():
        lines.append(f'  printf("{cname} . %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname} {n} %zu %zu\\n", offsetof({cname}, {n}), sizeof((({cname}*)0)->{n}));' for n, _ in cls._fields_]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines + ["  return 0;", "}", ""]))
    subprocess.run([cc, "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    theirs = [ln.split() for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    ours = []
    for cname, cls in _lib.STRUCTS.items():
        ours.append([cname, ".", str(C.sizeof(cls))])
        ours += [[cname, n, str(getattr(cls, n).offset), str(getattr(cls, n).size)] for n, _ in cls._fields_]
    assert ours == theirs
    assert [len(cls._fields_) for cls in _lib.STRUCTS.values()] == [59, 19, 14, 27, 6] and len(ours) == 5 + 125


def test_binding_equals_the_recorded_abi():
    with open(RECORD) as f:
        want = json.load(f)
    got = json.loads(json.dumps(abi_record()))
    changed = [f"{part}.{k}" for part in ("structs", "symbols") for k in want[part] if got[part].get(k) != want[part][k]]
    if got["version"] == want["version"]:
        assert not changed, f"{changed} differ from tests/golden/abi.json at ABI {want['version']}: bump T2P_ABI_VERSION and regenerate"
    assert got == want, "include/t2p.h declares what tests/golden/abi.json does not hold: regenerate the record"


@pytest.mark.parametrize("decl, named", [
    ("int t2p_f(unsigned x);", "unsigned x"),                                       # a type outside the table
    ("int t2p_f(const t2p_nobody* p);", "t2p_nobody* p"),                           # a struct nobody declared
    ("double t2p_f(void);", "double t2p_f"),                                        # known as a pointee only
    ("int t2p_f(void (*cb)(int), int n);", "(*cb)"),                                # function pointer
    ("typedef struct t2p_s { int32_t flags : 3; } t2p_s;", "flags : 3"),            # bit-field
    ("typedef struct t2p_s { struct { float x; } in; } t2p_s;", "struct t2p_s"),    # nested struct
    ("int t2p_f(int32_t n;", "t2p_f(int32_t n"),                                    # unbalanced parentheses
    ("int t2p_f(int32_t n));", "int32_t n)"),
    ("int t2p_f(float v[3]);", "t2p_f(float v[3])"),                                # array parameter: decays in C, not guessed
    ("typedef int t2p_handle;", "t2p_handle"),                                      # a typedef the rule does not know
])
def test_parser_refuses_what_it_does_not_know(decl, named):
    with pytest.raises(_lib.T2PError, match="include/t2p.h") as e:
        _lib.parse_header("int t2p_abi_version(void);\n" + decl + "\n")
    assert named in str(e.value)


def test_parser_reads_the_headers_constructs():
    defines, structs, symbols = _lib.parse_header("""
        #define T2P_A 7 /* decimal */
        #define T2P_B 0x1F
        #define T2P_C (-3)
        #define T2P_SKIPPED ((size_t)1 << 20)
        typedef struct t2p_s { const float *a, *b; float c, d[3]; uint8_t* e[3]; const int32_t* f; } t2p_s;
        const char* t2p_name(void);  // comment
        void t2p_g(const t2p_s* s, uint8_t* const* rows /*[3]*/, char* buf, size_t n, t2p_stream_t stream);
    """)
    assert defines == {"T2P_A": 7, "T2P_B": 31, "T2P_C": -3}
    S = structs["t2p_s"]
    assert S.__name__ == "S" and S._fields_ == [("a", C.c_void_p), ("b", C.c_void_p), ("c", C.c_float), ("d", C.c_float * 3),
                                                ("e", C.c_void_p * 3), ("f", C.c_void_p)]
    assert symbols == {"t2p_name": (C.c_char_p, []),
                       "t2p_g": (None, [C.POINTER(S), C.c_void_p, C.c_char_p, C.c_size_t, C.c_void_p])}


def test_library_resolves_every_symbol_at_the_headers_version():
    handle = _lib.lib()
    assert len(_lib.SYMBOLS) >= 72
    for name, (res, args) in _lib.SYMBOLS.items():
        fn = getattr(handle, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert handle.t2p_abi_version() == _lib.ABI_VERSION == _lib.DEFINES["T2P_ABI_VERSION"]
