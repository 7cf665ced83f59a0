"""reef_doc_transform (include/reef_msm.h 3l) on the device, bit-exact against the model (tests/doc_model.py; Python's strict decoder is the
UTF-8 authority).  The lengths straddle every boundary the kernels have: the 16 bytes of a lane, the 64 lanes of a wave, the 4096-byte tile
(4095 / 4096 / 4097), several tiles, and 2^22 + 7 bytes = 1025 tiles, one more than the scan takes in a single step (1024)."""
import ctypes
import functools

import numpy as np
import pytest

import doc_model as M
from reef_amd import _ffi, doc
from reef_amd.msm import DeviceBuffer

pytestmark = pytest.mark.gpu

TILE = 4096
LENGTHS = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5, 65539, 2 ** 22 + 7]
DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32}
POISON = 0xA5


def run(text: bytes, encoding, map_, eof, eps, elem_bytes, route, cap=None, extra=1, measure=False):
    """One call.  route 'host': host text in, host symbols out; 'device': device in, device out.  The output buffer holds cap + extra elements
    and is poisoned first.  -> (status, info as a dict, the whole buffer as an array of the element type)"""
    lib = _ffi.load()
    n = len(text)
    if cap is None:
        cap = M.next_pow2(n + 2)
    host_out = np.full((cap + extra) * elem_bytes, POISON, dtype=np.uint8)
    src = np.frombuffer(text, dtype=np.uint8) if n else np.zeros(16, dtype=np.uint8)
    info = _ffi.DocInfo()
    m_ptr, m_len = (None, 0) if map_ is None else (map_.ctypes.data, map_.size)
    if route == "host":
        st = lib.reef_doc_transform(src.ctypes.data, n, 0, encoding, m_ptr, m_len, eof, eps, None if measure else host_out.ctypes.data, elem_bytes,
                                    cap, 0, ctypes.byref(info))
        got = host_out
    else:
        d_text, d_out = DeviceBuffer.from_host(src), DeviceBuffer.from_host(host_out)
        st = lib.reef_doc_transform(d_text.ptr, n, 1, encoding, m_ptr, m_len, eof, eps, None if measure else d_out.ptr, elem_bytes, cap, 1,
                                    ctypes.byref(info))
        got = d_out.to_host(host_out.shape, dtype=np.uint8)
        d_text.free()
        d_out.free()
    return st, {k: int(getattr(info, k)) for k, _ in _ffi.DocInfo._fields_}, got.view(DTYPES[elem_bytes])


def poison_of(elem_bytes):
    return int.from_bytes(bytes([POISON]) * elem_bytes, "little")


def check(text, encoding, map_, eof, eps, elem_bytes, route):
    want, winfo = M.transform_array(text, encoding, map_, eof, eps)
    st, info, got = run(text, encoding, map_, eof, eps, elem_bytes, route)
    assert st == 0, _ffi.load().reef_last_error()
    if "chars" not in winfo:                                          # malformed: that is all the contract says
        assert info["malformed_at"] == winfo["malformed_at"] < len(text)
    else:
        assert info == winfo, (info, winfo)
    if want is None:
        assert (got == poison_of(elem_bytes)).all(), "nothing may be written"
        return
    p = winfo["padded"]
    assert np.array_equal(got[:p], want.astype(DTYPES[elem_bytes])), np.nonzero(got[:p] != want)[0][:8]
    assert (got[p:] == poison_of(elem_bytes)).all(), "written past padded"


# ---- texts and maps, made once

def dna_map():
    m = np.full(256, M.BAD, dtype=np.uint32)
    for i, c in enumerate(b"ACGT"):
        m[c] = i
    return m


def space_drop_map():
    m = np.full(256, M.BAD, dtype=np.uint32)
    m[:128] = np.arange(128)
    m[0x20] = M.DROP
    return m


@functools.lru_cache(maxsize=None)
def bytes_texts(n):
    """(DNA, 7-bit, letters with runs of spaces at the start, at the end and across every 4096-byte boundary, all spaces)"""
    rng = np.random.default_rng(1000 + n)
    dna = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes()
    seven = rng.integers(0, 128, n, dtype=np.uint8).tobytes()
    sp = rng.integers(0x41, 0x5B, n, dtype=np.uint8)
    sp[rng.random(n) < 0.1] = 0x20
    sp[:min(n, 5)] = 0x20
    sp[max(0, n - 7):] = 0x20
    for b in range(TILE, n, TILE):
        sp[max(0, b - 3):b + 4] = 0x20
        if b > 100000:
            break                                                     # (every boundary of the small texts, the first 25 of the large one)
    return dna, seven, sp.tobytes(), b" " * n


POOL = [0x41, 0xE9, 0x20AC, 0x1F600, 0xD7FF, 0xE000, 0x10FFFF]
LOW_POOL = [0x41, 0x7F, 0x80, 0xE9, 0x100, 0x12B]


def utf8_text(n, shift, pool, seed):
    """`shift` ASCII bytes, then characters from the pool: n bytes or as many below n as a character boundary allows"""
    rng = np.random.default_rng(seed)
    body = np.array(pool, dtype="<u4")[rng.integers(0, len(pool), max(0, n - shift))].tobytes().decode("utf-32-le").encode("utf-8")
    cut = max(0, n - shift)
    while cut > 0 and cut < len(body) and (body[cut] & 0xC0) == 0x80:
        cut -= 1
    text = b"xyz"[:min(shift, n)] + body[:cut]
    text.decode("utf-8")                                              # well formed by construction
    return text


@functools.lru_cache(maxsize=None)
def drop_e9_map():
    m = np.arange(0x110000, dtype=np.uint32)
    m[0xE9] = M.DROP
    m[0x1A] = 0x110002
    return m


def map_300():
    return ((np.arange(300, dtype=np.uint32) * 7 + 3) % 300).astype(np.uint32)


# ---- BYTES

@pytest.mark.parametrize("elem_bytes", [1, 2, 4])
@pytest.mark.parametrize("n", LENGTHS)
def test_bytes(gpu_lib, n, elem_bytes):
    dna, seven, spaced, spaces = bytes_texts(n)
    for route in ("host", "device"):
        check(dna, M.BYTES, dna_map(), 6, 5, elem_bytes, route)
        check(seven, M.BYTES, None, 130, 129, elem_bytes, route)
        check(spaced, M.BYTES, space_drop_map(), 130, 129, elem_bytes, route)
        check(spaces, M.BYTES, space_drop_map(), 130, 129, elem_bytes, route)


# ---- UTF-8

@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("n", LENGTHS)
def test_utf8(gpu_lib, n, shift):
    text = utf8_text(n, shift, POOL, 7 * n + shift)
    low = utf8_text(n, shift, LOW_POOL, 11 * n + shift)
    for route in ("host", "device"):
        check(text, M.UTF8, None, 0x10F802, 0x10F801, 4, route)
        check(low, M.UTF8, map_300(), 302, 301, 2, route)
        check(text, M.UTF8, drop_e9_map(), 0x110002, 0x110001, 4, route)


# ---- padded

@pytest.mark.parametrize("elem_bytes", [1, 2, 4])
@pytest.mark.parametrize("k", [1, 4, 12])
def test_padded(gpu_lib, k, elem_bytes):
    """kept + 2 = 2^k - 1, 2^k, 2^k + 1 (2^1 - 1 = 1 cannot be: kept + 2 >= 2); the zero tail to its last element, one element past it untouched"""
    for total in ((1 << k) - 1, 1 << k, (1 << k) + 1):
        if total < 2:
            continue
        text = b"a" * (total - 2)
        for route in ("host", "device"):
            st, info, got = run(text, M.BYTES, None, 200, 199, elem_bytes, route, cap=4 << k)
            p = M.next_pow2(total)
            assert st == 0 and info["kept"] == total - 2 and info["padded"] == p
            assert (got[:total - 2] == ord("a")).all() and got[total - 2] == 200 and got[total - 1] == 199
            assert (got[total:p] == 0).all() and (got[p:] == poison_of(elem_bytes)).all()


# ---- measure only, capacity

def test_measure_only_and_capacity(gpu_lib):
    text = utf8_text(5000, 1, POOL, 3)
    want, winfo = M.transform_array(text, M.UTF8, None, 0x10F802, 0x10F801)
    for route in ("host", "device"):
        st, info, got = run(text, M.UTF8, None, 0x10F802, 0x10F801, 4, route, measure=True)
        assert st == 0 and info == winfo and (got == poison_of(4)).all()
        st, info, got = run(text, M.UTF8, None, 0x10F802, 0x10F801, 4, route, cap=winfo["padded"] - 1)
        msg = gpu_lib.reef_last_error()
        assert st == 1 and info == winfo and (got == poison_of(4)).all()                        # REEF_ERR_ARG, info filled, nothing written
        assert str(winfo["padded"]).encode() in msg and str(winfo["padded"] - 1).encode() in msg
        st, info, got = run(text, M.UTF8, None, 0x10F802, 0x10F801, 4, route, cap=winfo["padded"])
        assert st == 0 and np.array_equal(got[:winfo["padded"]], want)


def test_front_end_chooses_the_width_and_the_place(gpu_lib):
    text = bytes_texts(4097)[0]
    want, winfo = M.transform_array(text, M.BYTES, dna_map(), 6, 5)
    sym, info = doc.transform(text, doc.DOC_BYTES, 4, dna_map())
    assert info["elem_bytes"] == 1 and sym.dtype == np.uint8 and np.array_equal(sym, want)
    d_text = DeviceBuffer.from_host(np.frombuffer(text, dtype=np.uint8))
    d_sym, info = doc.transform(d_text, doc.DOC_BYTES, 4, dna_map(), elem_bytes=2, nbytes=len(text))
    assert isinstance(d_sym, DeviceBuffer) and np.array_equal(d_sym.to_host((info["padded"],), dtype=np.uint16), want)
    assert doc.doc_transform("abc", b"ab") == [0, 1, 5, 4] and doc.doc_transform("abc", b"") == [5, 4]
    assert doc.doc_transform("a\u20acb", "b\u20aca".encode(), doc.DOC_UTF8) == [2, 1, 0, 5, 4, 0, 0, 0]
    with pytest.raises(ValueError, match="not in alphabet"):
        doc.doc_transform("abc", b"abd")
    with pytest.raises(ValueError, match="not UTF-8"):
        doc.doc_transform("abc", b"ab\xff", doc.DOC_UTF8)


# ---- bad characters

BAD_LEN = 3 * TILE + 100


@pytest.mark.parametrize("where", [[0], [BAD_LEN - 1], [TILE - 1], [TILE], [TILE - 1, TILE], [3 * TILE + 50], [0, 5000, BAD_LEN - 1],
                                   [2 * TILE - 1, 2 * TILE, 3 * TILE + 1, 3 * TILE + 99]])
def test_bad_characters(gpu_lib, where):
    text = bytearray(bytes_texts(BAD_LEN)[0])
    for i in where:
        text[i] = ord("N")
    for route in ("host", "device"):
        for eb in (1, 4):
            check(bytes(text), M.BYTES, dna_map(), 6, 5, eb, route)
    st, info, _ = run(bytes(text), M.BYTES, dna_map(), 6, 5, 1, "device")
    assert st == 0 and info["bad"] == len(where) and info["first_bad"] == where[0]


def test_a_character_beyond_the_map_is_bad(gpu_lib):
    text = utf8_text(5000, 0, LOW_POOL, 5) + "\u20ac".encode() + b"A" * 10
    short = np.arange(100, dtype=np.uint32)
    raw = bytes_texts(5000)[1][:4200] + bytes([200]) + b"AAAA"
    for route in ("host", "device"):
        check(text, M.UTF8, map_300(), 302, 301, 2, route)
        check(raw, M.BYTES, short, 130, 129, 1, route)
    assert M.transform_array(text, M.UTF8, map_300(), 302, 301)[1]["bad"] == 1
    assert M.transform_array(raw, M.BYTES, short, 130, 129)[1]["bad"] > 1


# ---- malformed UTF-8

FORMS = {   # name: (bytes, index of the byte that goes to the end of a tile, must it end the text)
    "80": (b"\x80", 0, False),
    "C0 80": (b"\xc0\x80", 0, False),
    "C2 at the end": (b"\xc2", 0, True),
    "E0 80 80": (b"\xe0\x80\x80", 0, False),
    "E2 82 at the end": (b"\xe2\x82", 0, True),
    "ED A0 80": (b"\xed\xa0\x80", 0, False),
    "F0 80 80 80": (b"\xf0\x80\x80\x80", 0, False),
    "F4 90 80 80": (b"\xf4\x90\x80\x80", 0, False),
    "F5 80 80 80": (b"\xf5\x80\x80\x80", 0, False),
    "FF": (b"\xff", 0, False),
    "E2 82 41": (b"\xe2\x82\x41", 0, False),
    "a valid character and one more continuation byte": (b"\xc3\xa9\x80", 0, False),
}


@pytest.mark.parametrize("name", list(FORMS))
def test_malformed_utf8(gpu_lib, name):
    form, lead, at_end = FORMS[name]
    valid = utf8_text(300, 1, POOL, 9)
    suffix = b"" if at_end else "xyz\u20ac".encode()
    placements = [form, valid + form + suffix, b"a" * (TILE - 1 - lead) + form + suffix,
                  b"a" * (2 * TILE - 5) + "\u20ac".encode() + b"a" * (TILE + 1 - lead) + form + suffix]      # the lead byte ends the third tile
    assert len(placements[2]) - len(suffix) - len(form) + lead == TILE - 1 and len(placements[3]) - len(suffix) - len(form) + lead == 3 * TILE - 1
    for text in placements:
        with pytest.raises(UnicodeDecodeError) as e:
            text.decode("utf-8")
        for route in ("host", "device"):
            st, info, got = run(text, M.UTF8, None, 0x10F802, 0x10F801, 4, route)
            assert st == 0 and info["malformed_at"] == e.value.start, (name, len(text), info, e.value.start)
            assert (got == poison_of(4)).all()


# ---- the chain the symbols are for

def test_chain_into_hyrax_and_merkle(gpu_lib):
    """bytes -> reef_doc_transform to device memory -> reef_hyrax_create(z_loc = REEF_DEVICE) -> commit at 2^6 x 2^6, and reef_merkle_create from the
    same kind of buffer (elem_bytes 4): equal to the same calls fed from host symbols"""
    from oracle import merkle_oracle as MO
    from oracle import pasta_ref as R
    from reef_amd import merkle, msm
    from reef_amd.hyrax import HyraxEval
    text = bytes_texts(4000)[0]
    want, winfo = M.transform_array(text, M.BYTES, dna_map(), 6, 5)
    assert winfo["padded"] == 4096
    d_text = DeviceBuffer.from_host(np.frombuffer(text, dtype=np.uint8))
    d_sym, info = doc.transform(d_text, doc.DOC_BYTES, 4, dna_map(), nbytes=len(text))
    assert info["padded"] == 4096 and info["elem_bytes"] == 1
    gens = R.gen_bases_ap(0, 7, 3, 64)
    h = R.gen_bases_ap(0, 0xB11D, 1, 1)[0].copy()
    blinds = list(range(3, 67))
    with msm.MsmContext(0, gens, bucket_groups=1) as key:
        with HyraxEval(0, d_sym, 12, 6, row_blinds=blinds, n=4096, elem_bytes=1) as from_device:
            got = from_device.commit(key, h)
        with HyraxEval(0, want.astype(np.uint8), 12, 6, row_blinds=blinds) as from_host:
            assert got == from_host.commit(key, h)
    d_sym4, info = doc.transform(d_text, doc.DOC_BYTES, 4, dna_map(), elem_bytes=4, nbytes=len(text))
    pp = MO.standin_params()
    args = (pp.t, pp.rf, pp.rp, pp.rc, pp.mds, pp.tag_leaf, pp.tag_node)
    with merkle.ResidentMerkleCommitment.new("pallas", d_sym4, *args, n=info["padded"]) as dev_tree, \
            merkle.ResidentMerkleCommitment.new("pallas", want, *args) as host_tree:
        assert dev_tree.commitment == host_tree.commitment and dev_tree.n == host_tree.n == 4096
