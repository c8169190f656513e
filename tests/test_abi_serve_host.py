"""The serving extension of the C ABI (include/t2p_serve.h) is held the way tests/test_abi_host.py holds include/t2p.h: the binding
_lib.py generates from the header against its recorded form (tests/golden/abi_serve.json, the form test_abi_host.abi_record writes),
a changed signature at the same version must fail, and the built library resolves every symbol at the header's version.  t2p.h,
its record and T2P_ABI_VERSION do not move when the extension does."""
import ctypes as C
import json
import os

import pytest

from text2pos_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "tests", "golden", "abi_serve.json")
_KINDS = {None: "void", C.c_int32: "int32", C.c_int64: "int64", C.c_uint32: "uint32", C.c_size_t: "size_t", C.c_float: "float",
          C.c_char_p: "char*"}


def _kind(t):
    """One word per ctypes type, as in tests/test_abi_host.py; a `const t2p_x*` names its struct, every other pointer is "ptr"."""
    if t in _KINDS:
        return _KINDS[t]
    return {cls: cname + "*" for cname, cls in _lib.STRUCTS.items()}.get(getattr(t, "_type_", None), "ptr")


def serve_record(defines=None, symbols=None):
    """What tests/golden/abi_serve.json holds.  To regenerate: json.dump(serve_record(), open(RECORD, "w"), indent=0, sort_keys=True)."""
    defines, symbols = defines or _lib.SERVE_DEFINES, symbols or _lib.SERVE_SYMBOLS
    return {"version": defines["T2P_SERVE_ABI_VERSION"], "structs": {},
            "symbols": {name: [_kind(res)] + [_kind(a) for a in args] for name, (res, args) in symbols.items()}}


def _compare(got, want):
    """tests/test_abi_host.py::test_binding_equals_the_recorded_abi's rule."""
    changed = [f"symbols.{k}" for k in want["symbols"] if got["symbols"].get(k) != want["symbols"][k]]
    if got["version"] == want["version"]:
        assert not changed, f"{changed} differ from tests/golden/abi_serve.json at serve ABI {want['version']}: bump T2P_SERVE_ABI_VERSION and regenerate"
    assert got == want, "include/t2p_serve.h declares what tests/golden/abi_serve.json does not hold: regenerate the record"


def _recorded():
    with open(RECORD) as f:
        return json.load(f)


def test_binding_equals_the_recorded_serve_abi():
    want = _recorded()
    _compare(json.loads(json.dumps(serve_record())), want)
    assert want["version"] == _lib.SERVE_ABI_VERSION == 1
    assert want["symbols"]["t2p_sim_topk_prior"] == ["int32"] + ["ptr"] * 7 + ["int64", "int64", "int32", "int32", "int64", "ptr", "ptr", "ptr",
                                                                              "size_t", "ptr"]
    assert want["symbols"]["t2p_serve_abi_version"] == ["int32"]


def test_a_changed_signature_at_the_same_version_fails():
    with open(_lib.SERVE_HEADER) as f:
        text = f.read()
    assert "int32_t dim, int32_t k, int64_t index_offset" in text
    for old, new in (("int32_t dim, int32_t k, int64_t index_offset", "int64_t dim, int32_t k, int64_t index_offset"),     # a widened scalar
                     ("const double* query_radius,", "double* query_radius, float scale,"),                             # an argument more
                     ("const double* cell_box,", "")):                                                                   # one less
        defines, structs, symbols = _lib.parse_header(text.replace(old, new, 1))
        assert not structs and defines["T2P_SERVE_ABI_VERSION"] == 1
        with pytest.raises(AssertionError, match="bump T2P_SERVE_ABI_VERSION"):
            _compare(json.loads(json.dumps(serve_record(defines, symbols))), _recorded())
    # at a new version the same change asks for a new record instead
    defines, _, symbols = _lib.parse_header(text.replace("T2P_SERVE_ABI_VERSION 1", "T2P_SERVE_ABI_VERSION 2", 1).replace("const double* cell_box,", "", 1))
    with pytest.raises(AssertionError, match="regenerate the record"):
        _compare(json.loads(json.dumps(serve_record(defines, symbols))), _recorded())
    # and the unchanged header passes
    defines, _, symbols = _lib.parse_header(text)
    _compare(json.loads(json.dumps(serve_record(defines, symbols))), _recorded())


def test_the_header_is_an_extension_in_the_same_dialect():
    with open(_lib.SERVE_HEADER) as f:
        text = f.read()
    assert '#include "t2p.h"' in text and "#define T2P_SERVE_ABI_VERSION 1" in text and "int t2p_serve_abi_version(void);" in text
    # t2p.h and what is generated from it stay what they were: the extension repeats none of its names
    assert not set(_lib.SERVE_SYMBOLS) & set(_lib.SYMBOLS) and not set(_lib.SERVE_DEFINES) & set(_lib.DEFINES)
    assert "t2p_sim_topk_prior" not in _lib.SYMBOLS and "T2P_SERVE_ABI_VERSION" not in _lib.DEFINES
    with open(_lib.HEADER) as f:
        assert "t2p_serve.h" in f.read().split("#ifndef T2P_H")[0]          # the opening comment points to it
    with open(os.path.join(ROOT, "text2pos-cvpr2022_amd", "csrc", "api.hip")) as f:
        assert '#include "../../include/t2p_serve.h"' in f.read()           # the file that defines the exports is held to it


def test_library_resolves_every_serve_symbol_at_the_headers_version():
    handle = _lib.lib()
    assert set(_lib.SERVE_SYMBOLS) == {"t2p_serve_abi_version", "t2p_sim_topk_prior"}
    for name, (res, args) in _lib.SERVE_SYMBOLS.items():
        fn = getattr(handle, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert handle.t2p_serve_abi_version() == _lib.SERVE_ABI_VERSION == _lib.SERVE_DEFINES["T2P_SERVE_ABI_VERSION"]
    assert handle.t2p_abi_version() == _lib.ABI_VERSION == 33
