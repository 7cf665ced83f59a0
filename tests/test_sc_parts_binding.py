"""reef_sc_set_table_parts at the boundary, without a device: the entry is declared, the ctypes reef_sc_part has the header's fields
in the header's order and sizes, the constants agree, and the Python front-end refuses symbol types it would have to wrap."""
import ctypes
import os
import re

import numpy as np
import pytest

from abi_text import ROOT, strip_comments
from reef_amd import _ffi

_C_TYPES = {"uint32_t": ctypes.c_uint32, "size_t": ctypes.c_size_t, "int": ctypes.c_int, "const void *": ctypes.c_void_p}


def _header():
    return strip_comments(open(os.path.join(ROOT, "include", "reef_msm.h")).read())


def test_the_entry_is_declared_and_bound():
    assert "reef_sc_set_table_parts" in _ffi.declared_symbols()
    fn = _ffi.load().reef_sc_set_table_parts                     # loads without a GPU
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 3 and fn.argtypes[1]._type_ is _ffi.ScPart


def test_the_ctypes_part_has_the_headers_fields():
    body = re.search(r"typedef struct\s*\{([^{}]*)\}\s*reef_sc_part\s*;", _header()).group(1)
    fields = []
    for decl in body.split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        m = re.fullmatch(r"(.*?[\s\*])(\w+)", decl)
        fields.append((m.group(2), _C_TYPES[m.group(1).strip()]))
    assert fields == list(_ffi.ScPart._fields_), (fields, _ffi.ScPart._fields_)
    assert [ctypes.sizeof(t) for _, t in fields] == [4, 4, 8, 8, 4]
    assert ctypes.sizeof(_ffi.ScPart) == 32                      # on this ABI: 4 + 4 + 8 + 8 + 4, padded to the pointer's alignment
    assert [getattr(_ffi.ScPart, n).offset for n, _ in fields] == [0, 4, 8, 16, 24]


def test_the_constants_agree_with_the_header():
    hdr = _header()
    assert int(re.search(r"#define\s+REEF_SC_MAX_PARTS\s+(\d+)", hdr).group(1)) == _ffi.SC_MAX_PARTS == 8
    kinds = dict((k, int(v)) for k, v in re.findall(r"(REEF_SC_PART_\w+)\s*=\s*(\d+)", hdr))
    assert kinds == {"REEF_SC_PART_FE": _ffi.SC_PART_FE, "REEF_SC_PART_SYMBOLS": _ffi.SC_PART_SYMBOLS, "REEF_SC_PART_FILL": _ffi.SC_PART_FILL}
    assert sorted(kinds.values()) == [0, 1, 2]


def test_the_front_end_builds_the_descriptors_and_refuses_what_it_would_have_to_wrap():
    from reef_amd.sumcheck import sc_part_descriptors
    q1 = (1 << 254) + 12345
    descs, keep = sc_part_descriptors([("fe", [3, q1]), ("fill", 7, 100), ("symbols", np.arange(5, dtype=np.uint16)),
                                       ("symbols", 0x1000, np.uint32, 9), ("symbols", np.zeros(0, dtype=np.uint8))])
    assert [(d.kind, d.elem_bytes, d.count, d.loc) for d in descs] == [(0, 0, 2, 0), (2, 0, 100, 0), (1, 2, 5, 0), (1, 4, 9, 1), (1, 1, 0, 0)]
    assert descs[3].data == 0x1000 and descs[4].data is None and len(keep) == 5
    assert ctypes.string_at(descs[1].data, 32) == (7).to_bytes(32, "little")
    assert ctypes.string_at(descs[0].data + 32, 32) == q1.to_bytes(32, "little")
    for dtype in (np.int8, np.int32, np.int64, np.uint64, np.float32):
        with pytest.raises(ValueError):
            sc_part_descriptors([("symbols", np.zeros(4, dtype=dtype))])
        with pytest.raises(ValueError):
            sc_part_descriptors([("symbols", 0x1000, dtype, 4)])
    with pytest.raises(ValueError):
        sc_part_descriptors([("symbols", [1, 2, 3])])
    with pytest.raises(ValueError):
        sc_part_descriptors([("rows", 1)])
