"""reef_msm_rows_symbols_wide (K2 from 16- and 32-bit document symbols; run_rows_symbols_wide, reef_amd/csrc/engine.inc) on the rows of
tests/wide_symbols.py: all 2^b - 1, all zero, a lone 2^(b-1) at the last index, the plane edges 255 / 256 / 257 / 65535 / 65536 / 65537 cut to b
bits, and uniform symbols.  Every result is compared bit-exactly, on the compressed encoding, with the C oracle's cref.row_msm on the same values
as 4-limb scalars (the plane split itself is pinned against the oracle by tests/test_rows_symbols_wide_host.py).

The route: P = ceil(b / 8) byte planes; tables of 256 multiples of 256^p * G_j for the P - 1 full planes and 2^(b - 8(P-1)) for the top one,
cached per (b, row_len) in the buffers the byte entry's block tables use (one set at a time); P entries a symbol (k_sym_entries_wide), then the
byte entry's tail (k_accum0, partial merge, k_final, blind)."""

import numpy as np
import pytest

from oracle.pasta_oracle import CURVES
from wide_symbols import as_scalars, as_symbols, batch

pytestmark = pytest.mark.gpu
CID = {"pallas": 0, "vesta": 1}
U16_WIDTHS = (1, 8, 9, 12, 16)
U32_WIDTHS = (8, 16, 17, 24, 25, 32)


def mismatch(got: bytes, want: bytes):
    """None when equal; otherwise the rows that differ (row i of a batch is family FAMILY_NAMES[i % 5])."""
    if got == want:
        return None
    return [i for i in range(len(want) // 32) if got[32 * i:32 * i + 32] != want[32 * i:32 * i + 32]] or "length"


def ints_of(limbs) -> list:
    return [sum(int(x) << (64 * k) for k, x in enumerate(row)) for row in limbs]


@pytest.fixture(scope="module")
def keys(cref):
    """Per curve: the longest key any test here needs (shorter ones are prefixes) and the blinding generator."""
    return {name: (cref.gen_bases_ap(cid, 77, 13, 1100), cref.gen_bases_ap(cid, 0xB11D, 1, 1)[0].copy()) for name, cid in CID.items()}


@pytest.fixture(scope="module")
def ref(cref, keys):
    """case(name, b, rows, row_len) -> (values, blinds, blinds in Montgomery form, expected rows without blinds, with blinds): computed once
    per case and shared, never written to."""
    cache = {}

    def case(name, b, rows, row_len):
        k = (name, b, rows, row_len)
        if k not in cache:
            cid, r = CID[name], CURVES[name].order
            bases, h = keys[name]
            vals = batch(b, rows, row_len)
            sc = as_scalars(vals)
            bl = cref.gen_scalars(cid, 0xB1 + b, rows, mont=False)             # full-width blinds, canonical
            bl_mont = as_scalars(ints_of(bl), r, mont=True)
            kb = bases[:row_len].copy()
            plain = cref.compress(cid, cref.row_msm(cid, kb, sc, rows, row_len, mont=False, threads=8))
            blinded = cref.compress(cid, cref.row_msm(cid, kb, sc, rows, row_len, h=h, blinds=bl, mont=False, threads=8))
            for a in (bl, bl_mont):
                a.setflags(write=False)
            cache[k] = (tuple(vals), bl, bl_mont, plain, blinded)
        return cache[k]
    return case


def check_case(ctx, name, dtype, b, rows, row_len, ref, keys, what=""):
    """Without blinds, with canonical blinds, with blinds in Montgomery form."""
    from reef_amd import msm
    cid, h = CID[name], keys[name][1]
    vals, bl, bl_mont, plain, blinded = ref(name, b, rows, row_len)
    sym = as_symbols(vals, dtype)
    got = msm.compress(cid, ctx.msm_rows_symbols_wide(sym, rows, row_len, b))
    assert mismatch(got, plain) is None, (what, name, dtype, b, rows, row_len, "rows that differ", mismatch(got, plain))
    got = msm.compress(cid, ctx.msm_rows_symbols_wide(sym, rows, row_len, b, blinds=bl, h=h, blinds_are_mont=False))
    assert mismatch(got, blinded) is None, (what, name, dtype, b, rows, row_len, "blinds, rows that differ", mismatch(got, blinded))
    got = msm.compress(cid, ctx.msm_rows_symbols_wide(sym, rows, row_len, b, blinds=bl_mont, h=h, blinds_are_mont=True))
    assert mismatch(got, blinded) is None, (what, name, dtype, b, rows, row_len, "mont blinds, rows that differ", mismatch(got, blinded))


# ------------------------------------------------------------------ widths and element sizes ----
@pytest.mark.parametrize("dtype,widths", [(np.uint16, U16_WIDTHS), (np.uint32, U32_WIDTHS)], ids=["u16", "u32"])
@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_every_plane_count_and_top_plane_width(name, dtype, widths, gpu_lib, cref, keys, ref):
    """rows = 5 (the five families), row_len = 300.  P = 1 (b <= 8), 2 (9..16), 3 (17..24), 4 (25..32); top planes of 1, 4 and 8 bits."""
    from reef_amd import msm
    with msm.MsmContext(CID[name], keys[name][0][:300].copy(), bucket_groups=1) as ctx:
        for b in widths:
            check_case(ctx, name, dtype, b, 5, 300, ref, keys)


@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_narrow_symbols_agree_with_the_byte_entry(name, gpu_lib, cref, keys, ref):
    """b <= 8 given as uint16 and as uint32 (one plane, k = 1) against reef_msm_rows_symbols (blocks of 9 / b generators), byte for byte."""
    from reef_amd import msm
    cid, h = CID[name], keys[name][1]
    with msm.MsmContext(cid, keys[name][0][:300].copy(), bucket_groups=1) as ctx:
        for b in (1, 3, 5, 8):
            vals, bl, _, plain, blinded = ref(name, b, 5, 300)
            byte_plain = msm.compress(cid, ctx.msm_rows_symbols(as_symbols(vals, np.uint8), 5, 300, b))
            byte_blind = msm.compress(cid, ctx.msm_rows_symbols(as_symbols(vals, np.uint8), 5, 300, b, blinds=bl, h=h, blinds_are_mont=False))
            assert byte_plain == plain and byte_blind == blinded, b
            for dtype in (np.uint16, np.uint32):
                sym = as_symbols(vals, dtype)
                assert msm.compress(cid, ctx.msm_rows_symbols_wide(sym, 5, 300, b)) == byte_plain, (b, dtype)
                assert msm.compress(cid, ctx.msm_rows_symbols_wide(sym, 5, 300, b, blinds=bl, h=h, blinds_are_mont=False)) == byte_blind, (b, dtype)


# ------------------------------------------------------------------ shapes ----
@pytest.mark.parametrize("rows", [1, 2, 70])
@pytest.mark.parametrize("row_len", [1, 3, 64, 257])
def test_small_and_ragged_shapes(row_len, rows, gpu_lib, cref, keys, ref):
    """70 rows reach k_final's second block and a ragged last wave; row_len = 1 and 3 leave most of a wave of k_sym_entries_wide idle."""
    from reef_amd import msm
    name = "pallas" if (rows + row_len) % 2 else "vesta"
    with msm.MsmContext(CID[name], keys[name][0][:row_len].copy(), bucket_groups=1) as ctx:
        check_case(ctx, name, np.uint16, 12, rows, row_len, ref, keys)
        check_case(ctx, name, np.uint32, 25, rows, row_len, ref, keys)


def test_more_than_one_block_of_every_kernel(gpu_lib, cref, keys, ref):
    """row_len = 600, rows = 37: 22200 symbols (87 blocks of k_sym_entries_wide), 2 and 3 planes."""
    from reef_amd import msm
    with msm.MsmContext(0, keys["pallas"][0][:600].copy(), bucket_groups=1) as ctx:
        check_case(ctx, "pallas", np.uint16, 16, 37, 600, ref, keys)
        check_case(ctx, "pallas", np.uint32, 17, 37, 600, ref, keys)


def test_rows_shorter_than_the_key(gpu_lib, cref, keys, ref):
    """row_len = 300 on a 500-point key: the plane generators and tables cover the prefix only."""
    from reef_amd import msm
    with msm.MsmContext(1, keys["vesta"][0][:500].copy(), bucket_groups=1) as ctx:
        check_case(ctx, "vesta", np.uint16, 12, 5, 300, ref, keys)
        check_case(ctx, "vesta", np.uint32, 32, 5, 300, ref, keys)


# ------------------------------------------------------------------ key kinds ----
@pytest.mark.parametrize("kind,opts,n", [("plain", dict(bucket_groups=0), 300), ("shifted", dict(bucket_groups=1), 300),
                                         ("shifted-4-groups", dict(window_bits=9, bucket_groups=4), 300),
                                         ("byte-tables", dict(bucket_groups=1, byte_tables=1), 1100)])
def test_every_kind_of_key_gives_its_generators_from_table_zero(kind, opts, n, gpu_lib, cref, keys, ref):
    from reef_amd import msm
    name = "pallas"
    with msm.MsmContext(CID[name], keys[name][0][:n].copy(), **opts) as ctx:
        if kind == "byte-tables":
            assert ctx.has_byte_tables()
        elif kind == "shifted-4-groups":
            assert (ctx.plan()["window_bits"], ctx.plan()["bucket_groups"]) == (9, 4)
        elif kind == "plain":
            assert ctx.plan()["tables"] == 1
        for b in (12, 16):
            check_case(ctx, name, np.uint16, b, 5, n, ref, keys, kind)


# ------------------------------------------------------------------ the doubling branch through a plane table ----
@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_equal_points_meet_in_the_accumulator(name, gpu_lib, cref):
    """B_j = (1 + j) G, so 256 B_0 = B_255: with s_0 = 256 and s_255 = 1 the row's only two non-identity entries are the same point, one
    from plane 1 and one from plane 0, and xyzz_add must double.  Second row: 512 B_0 = 2 B_255."""
    from reef_amd import msm
    cid, n = CID[name], 300
    bases = cref.gen_bases_ap(cid, 1, 1, n)
    vals = [0] * (2 * n)
    vals[0], vals[255], vals[n], vals[n + 255] = 256, 1, 512, 2
    want = cref.compress(cid, cref.row_msm(cid, bases, as_scalars(vals), 2, n, mont=False))
    twice = cref.compress(cid, np.stack([cref.scalar_mul(cid, bases[255], 2), cref.scalar_mul(cid, bases[255], 4)]))
    assert want == twice
    with msm.MsmContext(cid, bases, bucket_groups=1) as ctx:
        for dtype, b in ((np.uint16, 10), (np.uint16, 16), (np.uint32, 10), (np.uint32, 32)):
            got = msm.compress(cid, ctx.msm_rows_symbols_wide(as_symbols(vals, dtype), 2, n, b))
            assert mismatch(got, want) is None, (dtype, b, mismatch(got, want))


# ------------------------------------------------------------------ the table cache ----
def test_wide_and_byte_tables_take_turns_on_one_context(gpu_lib, cref, keys, ref):
    """The wide tables and the byte entry's block tables share the context's buffers, one set at a time, keyed by planes as well as (bits, row_len)."""
    from reef_amd import msm
    name = "pallas"
    cid, (bases, h) = CID[name], keys[name]

    def byte_call(ctx, rows, step):
        vals, bl, _, _, blinded = ref(name, 3, rows, 500)
        got = msm.compress(cid, ctx.msm_rows_symbols(as_symbols(vals, np.uint8), rows, 500, 3, blinds=bl, h=h, blinds_are_mont=False))
        assert mismatch(got, blinded) is None, (step, mismatch(got, blinded))

    with msm.MsmContext(cid, bases[:500].copy(), bucket_groups=1) as ctx:
        check_case(ctx, name, np.uint16, 12, 5, 500, ref, keys, 1)           # builds the wide tables for (12, 500)
        check_case(ctx, name, np.uint16, 12, 2, 500, ref, keys, 2)           # cached
        byte_call(ctx, 600, 3)                                               # the byte entry rebuilds its own (3, 500)
        check_case(ctx, name, np.uint32, 12, 5, 500, ref, keys, 4)           # and the wide entry its own again
        check_case(ctx, name, np.uint16, 16, 5, 500, ref, keys, 5)           # another width: same planes, a wider top plane
        check_case(ctx, name, np.uint16, 12, 5, 300, ref, keys, 6)           # another row length
        byte_call(ctx, 4, 7)                                                 # a byte batch too small to pay through reef_msm_rows, asked for directly
        vals, bl, _, _, blinded = ref(name, 12, 5, 500)                      # reef_msm_rows at width 12: `single`, no tables
        for bits in (0, 12):
            got = msm.compress(cid, ctx.msm_rows(as_scalars(vals), 5, 500, is_mont=False, max_scalar_bits=bits, blinds=bl, h=h))
            assert mismatch(got, blinded) is None, (8, bits, mismatch(got, blinded))


# ------------------------------------------------------------------ memory places ----
@pytest.mark.parametrize("dtype,b", [(np.uint16, 12), (np.uint32, 25)], ids=["u16", "u32"])
def test_symbols_blinds_and_results_on_the_host_and_on_the_device(dtype, b, gpu_lib, cref, keys, ref):
    from reef_amd import msm
    name, rows, row_len = "vesta", 5, 300
    cid, (bases, h) = CID[name], keys[name]
    vals, bl, _, plain, blinded = ref(name, b, rows, row_len)
    sym = as_symbols(vals, dtype)
    with msm.MsmContext(cid, bases[:row_len].copy(), bucket_groups=1) as ctx:
        d_sym, d_bl, d_h = msm.DeviceBuffer.from_host(sym), msm.DeviceBuffer.from_host(bl), msm.DeviceBuffer.from_host(h)
        eb = sym.dtype.itemsize
        # device symbols, blinds and h; result to the host and to the device
        got = msm.compress(cid, ctx.msm_rows_symbols_wide(d_sym, rows, row_len, b, elem_bytes=eb, blinds=d_bl, h=d_h, blinds_are_mont=False))
        assert mismatch(got, blinded) is None
        d_out = msm.DeviceBuffer(96 * rows)
        ctx.msm_rows_symbols_wide(d_sym, rows, row_len, b, elem_bytes=eb, blinds=d_bl, h=d_h, blinds_are_mont=False, out=d_out)
        ctx.sync()
        assert mismatch(msm.compress(cid, d_out.to_host((rows, 12))), blinded) is None
        # host symbols, blinds and h; result to the device
        ctx.msm_rows_symbols_wide(sym, rows, row_len, b, blinds=bl, h=h, blinds_are_mont=False, out=d_out)
        ctx.sync()
        assert mismatch(msm.compress(cid, d_out.to_host((rows, 12))), blinded) is None
        ctx.msm_rows_symbols_wide(d_sym, rows, row_len, b, elem_bytes=eb, out=d_out)
        ctx.sync()
        assert mismatch(msm.compress(cid, d_out.to_host((rows, 12))), plain) is None
        with pytest.raises(ValueError):
            ctx.msm_rows_symbols_wide(d_sym, rows, row_len, b, elem_bytes=eb, blinds=bl, h=h)      # blinds live where the symbols live
        assert ctx.msm_rows_symbols_wide(sym, 0, row_len, b).shape == (0, 12)                          # rows == 0: nothing to do


def test_bits_above_symbol_bits_are_ignored(gpu_lib, cref, keys, ref):
    from reef_amd import msm
    name, rows, row_len, b = "pallas", 5, 300, 9
    cid = CID[name]
    vals, _, _, plain, _ = ref(name, b, rows, row_len)
    dirty16 = as_symbols([v | 0x8000 | ((j % 3) << 12) for j, v in enumerate(vals)], np.uint16)
    dirty32 = as_symbols([v | 0x80000000 | ((j % 5) << 9) for j, v in enumerate(vals)], np.uint32)
    with msm.MsmContext(cid, keys[name][0][:row_len].copy(), bucket_groups=1) as ctx:
        assert mismatch(msm.compress(cid, ctx.msm_rows_symbols_wide(dirty16, rows, row_len, b)), plain) is None
        assert mismatch(msm.compress(cid, ctx.msm_rows_symbols_wide(dirty32, rows, row_len, b)), plain) is None


# ------------------------------------------------------------------ argument errors ----
def test_argument_errors_name_their_cause(gpu_lib, cref, keys):
    from reef_amd import _ffi, msm
    lib = gpu_lib
    bases, h = keys["pallas"]
    sym = np.zeros(2 * 300, dtype=np.uint32)
    bl = np.zeros((2, 4), dtype=np.uint64)
    out = np.zeros((2, 12), dtype=np.uint64)

    def call(ctx, elem_bytes=2, rows=2, row_len=300, bits=9, blinds=None, hh=None, s=sym):
        return lib.reef_msm_rows_symbols_wide(ctx._h, s.ctypes.data, elem_bytes, rows, row_len, _ffi.REEF_HOST, bits, blinds, hh, True,
                                              out.ctypes.data, _ffi.REEF_HOST)

    with msm.MsmContext(0, bases[:300].copy(), bucket_groups=0) as ctx:
        assert call(ctx) == 0
        for eb in (1, 3):
            assert call(ctx, elem_bytes=eb) == 1 and b"elem_bytes" in lib.reef_last_error(), eb
        assert call(ctx, bits=0) == 1 and b"symbol_bits" in lib.reef_last_error()
        assert call(ctx, bits=17) == 1 and b"symbol_bits" in lib.reef_last_error()
        assert call(ctx, elem_bytes=4, bits=17) == 0
        assert call(ctx, elem_bytes=4, bits=33) == 1 and b"symbol_bits" in lib.reef_last_error()
        assert call(ctx, row_len=301, rows=1) == 1 and b"exceeds the key length" in lib.reef_last_error()
        assert call(ctx, blinds=bl.ctypes.data) == 1 and b"null" in lib.reef_last_error()
        assert call(ctx, blinds=bl.ctypes.data, hh=h.ctypes.data) == 0
    n = 1 << 17                                                                # (3 * 256 + 256) * 2^17 = 2^27 table points: beyond the cap of 2^26
    big = np.zeros(n, dtype=np.uint32)
    with msm.MsmContext(0, msm.gen_bases(0, 5, 3, n, device=True), n, bucket_groups=0) as ctx:
        assert call(ctx, elem_bytes=4, rows=1, row_len=n, bits=32, s=big) == 1 and b"tables too large" in lib.reef_last_error()
        assert call(ctx, elem_bytes=4, rows=1 << 13, row_len=n, bits=9, s=big) == 1 and b"too many row entries" in lib.reef_last_error()   # 2^13 * 2^17 * 2 = 2^31


# ------------------------------------------------------------------ the provider ----
def test_provider_commits_a_uint16_document_as_it_commits_field_elements(gpu_lib, cref, keys):
    """2^12 symbols at b = 10 (64 rows of 64): HyraxPC.commit_symbols on the uint16 document = HyraxPC.commit on the values as field elements."""
    from reef_amd import msm
    from reef_amd.provider import CommitmentGens, HyraxPC
    name = "pallas"
    cid, r, (bases, h) = CID[name], CURVES[name].order, keys[name]
    vals = batch(10, 64, 64)
    bl = cref.gen_scalars(cid, 0xB1, 64, mont=True)
    gens = CommitmentGens(cid, bases[:64].copy(), h)
    try:
        pc = HyraxPC(gens)
        want_pts, want_comp = pc.commit(as_scalars(vals, r, mont=True), bl, is_mont=True, max_scalar_bits=10)
        got_pts, got_comp = pc.commit_symbols(as_symbols(vals, np.uint16), bl, 10)
        assert bytes(got_comp) == bytes(want_comp)
        assert cref.to_affine(cid, got_pts).tobytes() == cref.to_affine(cid, want_pts).tobytes()
        assert bytes(pc.commit_symbols(as_symbols(vals, np.uint32), bl, 10)[1]) == bytes(want_comp)
        with pytest.raises(ValueError, match="does not fit symbol_bits"):
            pc.commit_symbols(as_symbols(vals, np.uint16), bl, 9)
    finally:
        gens.close()
    grouped = CommitmentGens(cid, bases[:64].copy(), h, devices=[0, 0])
    try:
        with pytest.raises(ValueError, match="wide symbols are not split over devices yet"):
            HyraxPC(grouped).commit_symbols(as_symbols(vals, np.uint16), bl, 10)
    finally:
        grouped.close()
