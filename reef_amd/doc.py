"""A document's bytes -> alphabet symbols on the device (include/reef_msm.h 3l: reef_doc_transform): Reef's doc_transform
(src/backend/framework.rs:978-1011) over the characters read_doc hands it.  This module builds the character map with the reference's
rules and marshals buffers; the decoding, the lookup and the compaction happen in libreef_msm.so on the GPU.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Iterable, List, Optional, Tuple, Union

import numpy as np

from . import _ffi
from ._ffi import DOC_BAD, DOC_BYTES, DOC_DROP, DOC_UTF8, REEF_DEVICE, REEF_HOST, DocInfo, check  # noqa: F401
from .msm import DeviceBuffer

_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32}
# the largest symbol of an encoding's own alphabet (map=None): AsciiParser's 0..127, Utf8Parser's every scalar value in order
_OWN_MAX = {DOC_BYTES: 127, DOC_UTF8: 0x10FFFF - 0x800}


def char_map(alphabet: str, remap: Optional[Dict[str, str]] = None, drop: Iterable[str] = ()) -> np.ndarray:
    """The map reef_doc_transform takes, indexed by code point (for REEF_DOC_BYTES: by byte value), with doc_transform's rules: a
    character's symbol is its position in `alphabet`, a later duplicate overriding an earlier one; 0x1A gives len(alphabet) + 2 (EOF,
    inserted last: it overrides the alphabet's own entry); everything else is DOC_BAD.  `remap` {from: to} are the characters a
    transform rewrites before the lookup (CaseInsensitive: 'a' -> 'A'): they take the entry of what they become.  `drop` are the
    characters a transform filters out (IgnoreWhitespace): DOC_DROP, whatever else is said about them."""
    remap = dict(remap or {})
    drop = list(drop)
    points = [ord(c) for c in alphabet] + [ord(c) for c in remap] + [ord(c) for c in remap.values()] + [ord(c) for c in drop] + [0x1A]
    m = np.full(max(points) + 1, DOC_BAD, dtype=np.uint32)
    for i, c in enumerate(alphabet):
        m[ord(c)] = i
    m[0x1A] = len(alphabet) + 2
    looked_up = {src: m[ord(dst)] for src, dst in remap.items()}
    for src, v in looked_up.items():
        m[ord(src)] = v
    for c in drop:
        m[ord(c)] = DOC_DROP
    return m


def _text(text, nbytes: Optional[int]) -> Tuple[int, Optional[int], int, object]:
    """(loc, ptr, nbytes, what to keep alive) of a document: bytes-like or a uint8 numpy array (host), or a DeviceBuffer"""
    if isinstance(text, DeviceBuffer):
        n = text.nbytes if nbytes is None else nbytes
        if n > text.nbytes:
            raise ValueError(f"the device buffer holds {text.nbytes} bytes, not {n}")
        return REEF_DEVICE, text.ptr, n, text
    a = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray, memoryview)) else np.ascontiguousarray(text)
    if a.dtype != np.uint8:
        raise TypeError("the text is bytes, a uint8 numpy array or a reef_amd.msm.DeviceBuffer")
    n = a.size if nbytes is None else nbytes
    if n > a.size:
        raise ValueError(f"the text holds {a.size} bytes, not {n}")
    return REEF_HOST, (a.ctypes.data if a.size else None), n, a


def narrowest(alphabet_len: int, encoding: int, map: Optional[np.ndarray]) -> int:
    """the narrowest elem_bytes that holds every symbol a call can write"""
    top = alphabet_len + 2
    if map is None:
        top = max(top, _OWN_MAX[encoding])
    else:
        real = map[map < DOC_DROP]
        if real.size:
            top = max(top, int(real.max()))
    return 1 if top < 1 << 8 else 2 if top < 1 << 16 else 4


def transform(text, encoding: int, alphabet_len: int, map: Optional[np.ndarray] = None, elem_bytes: Optional[int] = None,
              out: Union[None, np.ndarray, DeviceBuffer] = None, *, nbytes: Optional[int] = None, measure_only: bool = False):
    """-> (symbols, info).  EOF is alphabet_len + 2 and EPSILON alphabet_len + 1, as doc_transform numbers them.  symbols: `out` (a
    DeviceBuffer, or a numpy array of the element width) filled with info['padded'] symbols; with out=None a new DeviceBuffer when the text
    is one, a numpy array of exactly `padded` symbols otherwise.  symbols is None when nothing was written: malformed UTF-8, a character
    outside the alphabet (info says which), or measure_only."""
    lib = _ffi.load()
    loc, ptr, n, keep = _text(text, nbytes)
    m = None if map is None else np.ascontiguousarray(map, dtype=np.uint32)
    eb = narrowest(alphabet_len, encoding, m) if elem_bytes is None else elem_bytes
    view = None
    if measure_only:
        out_loc, out_ptr, cap = REEF_HOST, None, 0
    elif out is None:
        cap = 2
        while cap < n + 2:                      # kept <= nbytes: the padded length cannot exceed this
            cap <<= 1
        if loc == REEF_DEVICE:
            out = DeviceBuffer(cap * eb)
            out_loc, out_ptr = REEF_DEVICE, out.ptr
        else:
            view = np.empty(cap, dtype=_DTYPES[eb])
            out_loc, out_ptr = REEF_HOST, view.ctypes.data
    elif isinstance(out, DeviceBuffer):
        out_loc, out_ptr, cap = REEF_DEVICE, out.ptr, out.nbytes // eb
    else:
        if out.dtype != _DTYPES[eb] or not out.flags["C_CONTIGUOUS"]:
            raise TypeError(f"out must be a C-contiguous {np.dtype(_DTYPES[eb])} array for elem_bytes = {eb}")
        out_loc, out_ptr, cap = REEF_HOST, out.ctypes.data, out.size
    info = DocInfo()
    check(lib.reef_doc_transform(ptr, n, loc, encoding, None if m is None else m.ctypes.data, 0 if m is None else m.size, alphabet_len + 2,
                                 alphabet_len + 1, out_ptr, eb, cap, out_loc, ctypes.byref(info)))
    del keep
    d = {k: int(getattr(info, k)) for k, _ in DocInfo._fields_}
    d["elem_bytes"] = eb
    if measure_only or d["malformed_at"] < n or d["bad"]:
        return None, d
    return (view[:d["padded"]] if view is not None else out), d


def doc_transform(ab: str, doc_bytes, encoding: int = DOC_BYTES) -> List[int]:
    """framework.rs:978 under its own name: the symbols of the document over alphabet `ab`, then EOF, EPSILON and zeros up to a power of
    two, as a list.  Where the reference panics (a character outside the alphabet; for UTF-8, read_to_string's error) this raises."""
    symbols, info = transform(doc_bytes, encoding, len(ab), char_map(ab))
    if symbols is None:
        if info["bad"]:
            raise ValueError(f"Character in document that's not in alphabet (byte offset {info['first_bad']}, {info['bad']} in all)")
        raise ValueError(f"the document is not UTF-8 (valid up to byte {info['malformed_at']})")
    return [int(v) for v in symbols]
