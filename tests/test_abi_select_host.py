"""The distinct-candidates extension of the C ABI (include/t2p_select.h) is held the way tests/test_abi_serve_host.py holds
include/t2p_serve.h: the binding _lib.py generates from the header against its recorded form (tests/golden/abi_select.json), a
changed signature at the same version must fail, and the built library resolves every symbol at the header's version.  t2p.h,
t2p_serve.h, their records and versions do not move when this extension does."""
import ctypes as C
import json
import os

import pytest

from text2pos_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORD = os.path.join(ROOT, "tests", "golden", "abi_select.json")
_KINDS = {None: "void", C.c_int32: "int32", C.c_int64: "int64", C.c_uint32: "uint32", C.c_size_t: "size_t", C.c_float: "float",
          C.c_double: "double", C.c_char_p: "char*"}


def _kind(t):
    """One word per ctypes type, as in tests/test_abi_host.py; a `const t2p_x*` names its struct, every other pointer is "ptr"."""
    if t in _KINDS:
        return _KINDS[t]
    return {cls: cname + "*" for cname, cls in _lib.STRUCTS.items()}.get(getattr(t, "_type_", None), "ptr")


def select_record(defines=None, symbols=None):
    """What tests/golden/abi_select.json holds.  To regenerate: json.dump(select_record(), open(RECORD, "w"), indent=0, sort_keys=True)."""
    defines, symbols = defines or _lib.SELECT_DEFINES, symbols or _lib.SELECT_SYMBOLS
    return {"version": defines["T2P_SELECT_ABI_VERSION"], "structs": {},
            "symbols": {name: [_kind(res)] + [_kind(a) for a in args] for name, (res, args) in symbols.items()}}


def _compare(got, want):
    """tests/test_abi_host.py::test_binding_equals_the_recorded_abi's rule."""
    changed = [f"symbols.{k}" for k in want["symbols"] if got["symbols"].get(k) != want["symbols"][k]]
    if got["version"] == want["version"]:
        assert not changed, f"{changed} differ from tests/golden/abi_select.json at select ABI {want['version']}: bump T2P_SELECT_ABI_VERSION and regenerate"
    assert got == want, "include/t2p_select.h declares what tests/golden/abi_select.json does not hold: regenerate the record"


def _recorded():
    with open(RECORD) as f:
        return json.load(f)


def test_binding_equals_the_recorded_select_abi():
    want = _recorded()
    _compare(json.loads(json.dumps(select_record())), want)
    assert want["version"] == _lib.SELECT_ABI_VERSION == 1
    assert want["symbols"]["t2p_topk_distinct"] == ["int32", "ptr", "ptr", "int64", "int32", "int64", "int64", "ptr", "ptr", "double", "int32",
                                                    "ptr", "ptr", "ptr", "ptr", "ptr"]
    assert want["symbols"]["t2p_select_abi_version"] == ["int32"]


def test_a_changed_signature_at_the_same_version_fails():
    with open(_lib.SELECT_HEADER) as f:
        text = f.read()
    assert "double sep, int32_t k," in text
    for old, new in (("double sep, int32_t k,", "float sep, int32_t k,"),                                  # a narrowed scalar
                     ("const int32_t* cell_group,", "const int32_t* cell_group, int32_t n_groups,"),       # an argument more
                     ("int32_t* exhausted,", "")):                                                         # one less
        assert text.count(old) == 1
        defines, structs, symbols = _lib.parse_header(text.replace(old, new, 1))
        assert not structs and defines["T2P_SELECT_ABI_VERSION"] == 1
        with pytest.raises(AssertionError, match="bump T2P_SELECT_ABI_VERSION"):
            _compare(json.loads(json.dumps(select_record(defines, symbols))), _recorded())
    # at a new version the same change asks for a new record instead
    defines, _, symbols = _lib.parse_header(text.replace("T2P_SELECT_ABI_VERSION 1", "T2P_SELECT_ABI_VERSION 2", 1).replace("int32_t* exhausted,", "", 1))
    with pytest.raises(AssertionError, match="regenerate the record"):
        _compare(json.loads(json.dumps(select_record(defines, symbols))), _recorded())
    # and the unchanged header passes
    defines, _, symbols = _lib.parse_header(text)
    _compare(json.loads(json.dumps(select_record(defines, symbols))), _recorded())


def test_the_header_is_an_extension_in_the_same_dialect():
    with open(_lib.SELECT_HEADER) as f:
        text = f.read()
    assert '#include "t2p.h"' in text and "#define T2P_SELECT_ABI_VERSION 1" in text and "int t2p_select_abi_version(void);" in text
    # t2p.h, t2p_serve.h and what is generated from them stay what they were: the extension repeats none of their names
    earlier_symbols, earlier_defines = set(_lib.SYMBOLS) | set(_lib.SERVE_SYMBOLS), set(_lib.DEFINES) | set(_lib.SERVE_DEFINES)
    assert not set(_lib.SELECT_SYMBOLS) & earlier_symbols and not set(_lib.SELECT_DEFINES) & earlier_defines
    assert "t2p_topk_distinct" not in earlier_symbols and "T2P_SELECT_ABI_VERSION" not in earlier_defines
    assert _lib.ABI_VERSION == 33 and _lib.SERVE_ABI_VERSION == 1
    csrc = os.path.join(ROOT, "text2pos-cvpr2022_amd", "csrc")
    for name in ("api.hip", "distinct.hip"):                # the files that define the exports are held to the header
        with open(os.path.join(csrc, name)) as f:
            assert '#include "../../include/t2p_select.h"' in f.read(), name


def test_library_resolves_every_select_symbol_at_the_headers_version():
    handle = _lib.lib()
    assert set(_lib.SELECT_SYMBOLS) == {"t2p_select_abi_version", "t2p_topk_distinct"}
    for name, (res, args) in _lib.SELECT_SYMBOLS.items():
        fn = getattr(handle, name)
        assert fn.restype is res and list(fn.argtypes) == args, name
    assert handle.t2p_select_abi_version() == _lib.SELECT_ABI_VERSION == _lib.SELECT_DEFINES["T2P_SELECT_ABI_VERSION"]
    assert handle.t2p_serve_abi_version() == _lib.SERVE_ABI_VERSION and handle.t2p_abi_version() == _lib.ABI_VERSION


def test_every_refused_argument_is_named_without_a_gpu():
    """The entry point checks its arguments before it touches the device: each refusal is T2P_E_ARG with the argument's name."""
    handle = _lib.lib()
    buf = (C.c_double * 64)()                               # never read: every call below is refused first
    p = C.c_void_p(C.addressof(buf))
    null = C.c_void_p(0)

    def call(pool_idx=p, pool_score=p, nq=1, pool=8, n_cells=20, cell_xy=p, sep=1.0, k=4, out_idx=p, out_score=p, n_valid=p, exhausted=p):
        rc = handle.t2p_topk_distinct(pool_idx, pool_score, nq, pool, n_cells, 0, cell_xy, null, sep, k, out_idx, out_score, n_valid,
                                      exhausted, null)
        return rc, handle.t2p_last_error().decode()

    for kw, word in ((dict(k=0), "k=0"), (dict(k=9), "k=9 exceeds pool=8"), (dict(pool=1025, k=4), "pool=1025"),
                     (dict(sep=-1.0), "sep=-1"), (dict(sep=float("nan")), "sep="), (dict(pool_idx=null), "pool_idx"),
                     (dict(pool_score=null), "pool_score"), (dict(cell_xy=null), "cell_xy"), (dict(out_idx=null), "out_idx"),
                     (dict(out_score=null), "out_score"), (dict(n_valid=null), "n_valid"), (dict(exhausted=null), "exhausted"),
                     (dict(n_cells=0), "n_cells"), (dict(nq=-1), "nq")):
        rc, msg = call(**kw)
        assert rc == -1 and msg.startswith("topk_distinct:") and word in msg, (kw, rc, msg)
    assert call(nq=0)[0] == 0                               # no queries: nothing to launch, no error
