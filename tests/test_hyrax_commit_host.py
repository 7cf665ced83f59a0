"""reef_hyrax_commit and reef_hyrax_eval_comm_own without a GPU (include/reef_msm.h 3i): the header declares them, the ctypes binding
and INTEGRATION.md's Rust block agree with it kind for kind, the ABI version stays 7, and the Python front-end has both calls.  (The
place of eval_comm_own in the call order is host/proof_order_selftest's, run by tests/test_replay_prove_host.py.)"""
import ctypes
import os
import re

from abi_text import header_prototypes, rust_kind, split_top, strip_comments

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("reef_hyrax_commit", "reef_hyrax_eval_comm_own")
_CTYPES = {ctypes.c_void_p: "ptr", ctypes.c_int: "i32", ctypes.c_size_t: "usize", ctypes.c_bool: "bool", None: "void"}


def _ctypes_kind(t):
    if t in _CTYPES:
        return _CTYPES[t]
    return "ptr" if issubclass(t, (ctypes._Pointer, ctypes.c_void_p)) else str(t)


def test_the_header_declares_both_calls():
    protos = header_prototypes()
    assert protos["reef_hyrax_commit"] == ("i32", ["ptr", "ptr", "ptr", "ptr", "ptr", "i32"])
    assert protos["reef_hyrax_eval_comm_own"] == ("i32", ["ptr", "ptr"])


def test_the_binding_declares_them_with_the_headers_kinds_and_the_library_exports_them():
    from reef_amd import _ffi
    lib = _ffi.load()
    protos = header_prototypes()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for name in SYMBOLS:
        assert name in _ffi.declared_symbols() and hasattr(raw, name), name
        fn = getattr(lib, name)
        assert fn.argtypes is not None, f"{name} is not bound in reef_amd/_ffi.py"
        assert (_ctypes_kind(fn.restype), [_ctypes_kind(a) for a in fn.argtypes]) == protos[name], name
    assert lib.reef_abi_version() == _ffi.ABI_VERSION == 7


def test_integration_declares_them_in_rust():
    protos = header_prototypes()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    seen = set()
    for f in re.finditer(r"\bfn\s+(reef_hyrax_\w+)\s*\(((?:[^;{}()\[\]]|\[[^\]]*\])*?)\)\s*(?:->\s*([^;{]+?))?\s*;", doc, flags=re.S):
        name, args, ret = f.group(1), strip_comments(f.group(2)), (f.group(3) or "void").strip()
        if name in SYMBOLS:
            assert (rust_kind(ret), [rust_kind(a.split(":", 1)[1]) for a in split_top(args)]) == protos[name], name
            seen.add(name)
    assert seen == set(SYMBOLS), sorted(set(SYMBOLS) - seen)


def test_the_front_end_has_both_calls():
    from reef_amd.hyrax import HyraxEval
    assert callable(HyraxEval.commit) and callable(HyraxEval.eval_comm_own)


def test_null_handles_are_refused_before_any_device_is_touched():
    from reef_amd import _ffi
    lib = _ffi.load()
    assert lib.reef_hyrax_commit(None, None, None, None, None, 0) == 1 and b"null" in lib.reef_last_error()
    assert lib.reef_hyrax_eval_comm_own(None, None) == 1 and b"null" in lib.reef_last_error()
