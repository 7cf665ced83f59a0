"""reef_doc_transform (include/reef_msm.h 3l) without a GPU: the reference model against written-out cases, char_map, the bindings
against the header, the argument errors that are found before any device call, and the host program that checks the C++ char_map."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import doc_model as M
from abi_text import ROOT, header_prototypes, rust_kind, split_top, strip_comments
from reef_amd import _ffi, doc


# ---- the model against written-out cases

def test_model_ab_over_abc():
    assert M.doc_transform("abc", "ab") == [0, 1, 5, 4]
    syms, info = M.transform(b"ab", M.BYTES, doc.char_map("abc"), 5, 4)
    assert syms == [0, 1, 5, 4] and info == {"chars": 2, "kept": 2, "padded": 4, "bad": 0, "first_bad": 2, "malformed_at": 2}


def test_model_empty_document():
    for ab in ("", "abc", "x" * 100):
        assert M.doc_transform(ab, "") == [len(ab) + 2, len(ab) + 1]
        assert M.transform(b"", M.BYTES, doc.char_map(ab), len(ab) + 2, len(ab) + 1)[0] == [len(ab) + 2, len(ab) + 1]


@pytest.mark.parametrize("k", [1, 2, 4, 12])
def test_model_padding_rule(k):
    """padded is the plain next power of two of kept + 2: exact at 2^k, doubled at 2^k + 1"""
    for total, want in ((1 << k, 1 << k), ((1 << k) + 1, 2 << k)):
        if total < 2:
            continue
        out = M.doc_transform("a", "a" * (total - 2))
        assert len(out) == want and out[:total - 2] == [0] * (total - 2) and out[total - 2:total] == [3, 2] and not any(out[total:])
        assert M.transform(b"a" * (total - 2), M.BYTES, None, 3, 2)[1]["padded"] == want


def test_model_padding_is_not_the_reference_f32_quirk():
    """costs.rs:10-15 rounds 2^24 + 1 down through f32; the library does not (include/reef_msm.h 3l)"""
    assert M.next_pow2((1 << 24) + 1) == 1 << 25


def test_model_0x1a_maps_to_eof():
    assert M.doc_transform("abc", "a\x1ab") == [0, 5, 1, 5, 4, 0, 0, 0]
    assert M.doc_transform("a\x1ab", "\x1a")[0] == 5                    # also when the alphabet lists it: the EOF insert comes last
    assert M.transform(b"\x1a", M.BYTES, None, 130, 129)[0] == [130, 130, 129, 0]
    assert M.transform(b"\x1a", M.UTF8, None, 7, 6)[0] == [7, 7, 6, 0]


def test_model_duplicate_takes_the_later_index():
    assert M.doc_transform("abca", "a") == [3, 6, 5, 0]
    assert doc.char_map("abca")[ord("a")] == 3


def test_model_own_alphabets():
    assert M.transform(b"A\x7f", M.BYTES, None, 130, 129)[0] == [65, 127, 130, 129]
    assert M.transform(b"\x80", M.BYTES, None, 130, 129)[1]["bad"] == 1
    text = "\ud7ff\ue000\U0010ffff".encode("utf-8")
    assert M.transform(text, M.UTF8, None, 0x10F802, 0x10F801)[0][:3] == [0xD7FF, 0xD800, 0x10F7FF]


def test_model_malformed_is_the_decoders_start():
    assert M.transform(b"ab\xc0\x80", M.UTF8, None, 9, 8) == (None, {"malformed_at": 2})
    assert M.transform(b"\xe2\x82", M.UTF8, None, 9, 8) == (None, {"malformed_at": 0})


def test_char_map_with_remap_and_drop():
    m = doc.char_map("abc")
    assert m.dtype == np.uint32 and m.shape == (ord("c") + 1,)
    assert [m[ord(c)] for c in "abc"] == [0, 1, 2] and m[0x1A] == 5 and m[0] == doc.DOC_BAD and m[ord("A")] == doc.DOC_BAD
    assert int((m == doc.DOC_BAD).sum()) == m.size - 4
    assert doc.char_map("")[0x1A] == 2 and doc.char_map("").size == 0x1B
    m = doc.char_map("ABC", remap={"a": "A", "b": "B", "z": "Z"})              # CaseInsensitive
    assert m[ord("a")] == 0 and m[ord("b")] == 1 and m[ord("c")] == doc.DOC_BAD and m[ord("z")] == doc.DOC_BAD and m.size == ord("z") + 1
    m = doc.char_map("ab", remap={"a": "b", "b": "a"})                          # looked up before either side is written
    assert m[ord("a")] == 1 and m[ord("b")] == 0
    m = doc.char_map("a b", remap={"\t": " "}, drop=" \n")                      # IgnoreWhitespace
    assert m[ord("a")] == 0 and m[ord("b")] == 2 and m[ord(" ")] == doc.DOC_DROP and m[ord("\n")] == doc.DOC_DROP and m[ord("\t")] == 1
    m = doc.char_map("A\u00e9\u20ac\U0001f600")
    assert m.size == 0x1F601 and m[0x1F600] == 3 and m[0xD800] == doc.DOC_BAD and m[0x1A] == 6
    # the map drives the model the way the transforms drive the reference
    assert M.transform(b"a B\tc", M.BYTES, doc.char_map("ABC", remap={"a": "A", "c": "C"}, drop=" \t"), 5, 4)[0] == [0, 1, 2, 5, 4, 0, 0, 0]


def test_narrowest_width():
    assert doc.narrowest(4, doc.DOC_BYTES, doc.char_map("ACGT")) == 1
    assert doc.narrowest(128, doc.DOC_BYTES, None) == 1 and doc.narrowest(254, doc.DOC_BYTES, None) == 2
    assert doc.narrowest(300, doc.DOC_UTF8, np.arange(300, dtype=np.uint32)) == 2
    assert doc.narrowest(0x10F800, doc.DOC_UTF8, None) == 4


# ---- the bindings

def test_binding_and_rust_declaration_match_the_header():
    protos = header_prototypes()
    assert protos["reef_doc_transform"] == ("i32", ["ptr", "usize", "i32", "i32", "ptr", "usize", "u32", "u32", "ptr", "u32", "usize", "i32", "ptr"])
    fn = _ffi.load().reef_doc_transform
    kinds = {ctypes.c_int: "i32", ctypes.c_uint32: "u32", ctypes.c_uint64: "usize", ctypes.c_void_p: "ptr"}
    assert [kinds.get(t, "ptr") for t in fn.argtypes] == protos["reef_doc_transform"][1] and fn.restype is ctypes.c_int
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    m = re.search(r"\bfn\s+reef_doc_transform\s*\(([^;{}]*?)\)\s*->\s*([^;{]+?)\s*;", text, flags=re.S)
    assert m, "INTEGRATION.md does not declare reef_doc_transform"
    assert (rust_kind(m.group(2)), [rust_kind(a.split(":", 1)[1]) for a in split_top(strip_comments(m.group(1)))]) == protos["reef_doc_transform"]
    body = re.search(r"#\[repr\(C\)\]\s*(?:pub\s+)?struct\s+ReefDocInfo\s*\{(.*?)\}", text, flags=re.S).group(1)
    fields = [f.split(":")[0].replace("pub", "").strip() for f in split_top(strip_comments(body))]
    assert fields == [n for n, _ in _ffi.DocInfo._fields_] == ["chars", "kept", "padded", "bad", "first_bad", "malformed_at"]
    hdr = open(_ffi.HEADER).read()
    assert "REEF_DOC_DROP 0xFFFFFFFEu" in hdr and "REEF_DOC_BAD  0xFFFFFFFFu" in hdr and "REEF_DOC_BYTES = 0" in hdr and "REEF_DOC_UTF8  = 1" in hdr
    assert (doc.DOC_BYTES, doc.DOC_UTF8, doc.DOC_DROP, doc.DOC_BAD) == (0, 1, 0xFFFFFFFE, 0xFFFFFFFF)
    assert "reef_doc_transform" in _ffi.declared_symbols() and int(re.search(r"#define REEF_ABI_VERSION (\d+)", hdr).group(1)) == 7


def test_doc_info_is_48_bytes():
    assert ctypes.sizeof(_ffi.DocInfo) == 48


def _call(text=b"abc", nbytes=None, text_loc=0, encoding=0, map_=None, eof=130, eps=129, elem_bytes=1, out_loc=0, cap=8, text_ptr=None):
    lib = _ffi.load()
    buf = np.frombuffer(text, dtype=np.uint8)
    out = np.full(cap * 4, 0xAB, dtype=np.uint8)
    info = _ffi.DocInfo()
    st = lib.reef_doc_transform(buf.ctypes.data if text_ptr is None else text_ptr, len(text) if nbytes is None else nbytes, text_loc, encoding,
                                None if map_ is None else map_.ctypes.data, 0 if map_ is None else map_.size, eof, eps, out.ctypes.data, elem_bytes, cap,
                                out_loc, ctypes.byref(info))
    assert (out == 0xAB).all()                       # nothing is written on any of these paths
    return st, lib.reef_last_error()


def test_text_independent_argument_errors_come_before_any_device_call():
    """REEF_ERR_ARG (1) with or without a GPU: were the device asked first, a machine without one would say REEF_ERR_NO_GPU (3)"""
    assert _call(elem_bytes=3)[0] == 1 and b"elem_bytes" in _call(elem_bytes=3)[1]
    assert _call(elem_bytes=0)[0] == 1 and _call(elem_bytes=8)[0] == 1
    assert _call(eof=256, elem_bytes=1)[0] == 1 and b"fit" in _call(eof=256, elem_bytes=1)[1]        # a symbol too wide for elem_bytes
    assert _call(eps=65536, elem_bytes=2)[0] == 1
    wide = np.array([0, 1, 300, doc.DOC_DROP, doc.DOC_BAD], dtype=np.uint32)
    assert _call(map_=wide, elem_bytes=1)[0] == 1 and b"map[2]" in _call(map_=wide, elem_bytes=1)[1]
    assert _call(encoding=doc.DOC_UTF8, elem_bytes=2, eof=9, eps=8)[0] == 1                           # the UTF-8 alphabet needs 4 bytes
    assert _call(encoding=2)[0] == 1 and b"encoding" in _call(encoding=2)[1]
    assert _call(encoding=-1)[0] == 1
    assert _call(text_loc=2)[0] == 1 and _call(out_loc=5)[0] == 1
    assert _call(nbytes=1 << 32)[0] == 1 and b"2^32" in _call(nbytes=1 << 32)[1]
    assert _call(text_ptr=0, nbytes=3)[0] == 1                                                        # a null text with bytes
    assert _call(text_loc=1, text_ptr=0x1008)[0] == 1 and b"aligned" in _call(text_loc=1, text_ptr=0x1008)[1]


def test_fails_loudly_without_a_gpu():
    if _ffi.load().reef_device_count() > 0:
        pytest.skip("a GPU is present")
    st, msg = _call()
    assert st == 3 and b"no HIP device" in msg                                                        # REEF_ERR_NO_GPU, not a crash
    with pytest.raises(_ffi.ReefError) as e:
        doc.transform(b"ACGT", doc.DOC_BYTES, 4, doc.char_map("ACGT"))
    assert e.value.status == 3
    with pytest.raises(_ffi.ReefError):
        doc.doc_transform("abc", b"ab")


# ---- the host program

def test_doc_map_selftest_passes():
    exe = os.path.join(os.path.dirname(_ffi.LIB_PATH), "doc_map_selftest")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "doc_map_selftest ok" in out.stdout, out.stdout + out.stderr
    mk = open(os.path.join(_ffi.CSRC, "host", "Makefile")).read()
    assert re.search(r"doc_map_selftest\.cpp -I\$\(INC\) -o \$@", mk), "the self-test links no library"
