"""reef_msm_rows_symbols_wide without a GPU (include/reef_msm.h, K2 from 16- and 32-bit document symbols): the library exports the entry and
guards a NULL context, the plane split the kernel implements (tests/wide_symbols.py: a symbol is the sum of its bytes times powers of 256, so a
row is a plain sum over the plane generators 256^p * G_j) agrees with the C oracle's row_msm on the symbols themselves, and
HyraxPC.commit_symbols refuses what it would otherwise wrap: another dtype, and values that do not fit symbol_bits."""

import numpy as np
import pytest

from wide_symbols import FAMILY_NAMES, as_scalars, as_symbols, families, plane_split, planes_of

ROWS, ROW_LEN = 3, 40


def test_library_exports_the_entry_and_refuses_a_null_context():
    from reef_amd import _ffi
    lib = _ffi.load()
    assert hasattr(lib, "reef_msm_rows_symbols_wide")
    sym = np.zeros(4, dtype=np.uint16)
    out = np.zeros((1, 12), dtype=np.uint64)
    st = lib.reef_msm_rows_symbols_wide(None, sym.ctypes.data, 2, 1, 4, _ffi.REEF_HOST, 9, None, None, True, out.ctypes.data, _ffi.REEF_HOST)
    assert st == 1, st                                                      # REEF_ERR_ARG
    assert lib.reef_last_error()


def test_plane_split_is_a_partition_of_the_symbol():
    for b in (1, 8, 9, 16, 17, 24, 25, 32):
        vals = families(b, ROW_LEN)["rand"] + families(b, ROW_LEN)["edges"]
        for r, row in enumerate(plane_split(vals, ROW_LEN, b)):
            assert len(row) == planes_of(b) * ROW_LEN
            back = [0] * ROW_LEN
            for p, j, byte in row:
                assert 0 <= byte < 256 and p < planes_of(b)
                back[j] += byte << (8 * p)
            assert back == vals[r * ROW_LEN:(r + 1) * ROW_LEN]
            top = [byte for p, _, byte in row if p == planes_of(b) - 1]
            assert max(top) < 1 << (b - 8 * (planes_of(b) - 1))                 # the top plane's table holds 2^(b - 8(P-1)) multiples only


@pytest.fixture(scope="module")
def plane_gens(cref):
    """Per curve: G_j = the first ROW_LEN points of the GPU tests' key, and 256^p * G_j for p < 4, each made by the oracle's scalar_mul."""
    out = {}
    for cid in (0, 1):
        g = cref.gen_bases_ap(cid, 77, 13, ROW_LEN)
        planes = [g]
        for p in (1, 2, 3):
            planes.append(cref.to_affine(cid, np.stack([cref.scalar_mul(cid, g[j], 256 ** p) for j in range(ROW_LEN)])))
        out[cid] = np.ascontiguousarray(np.concatenate(planes))
        out[cid].setflags(write=False)
    return out


@pytest.mark.parametrize("cid", [0, 1])
@pytest.mark.parametrize("family", FAMILY_NAMES)
def test_plane_model_equals_the_row_msm_of_the_symbols(family, cid, cref, plane_gens):
    """ROWS rows of one family (seeds 0, 1, 2) at every width whose plane count or top plane differs."""
    for b in (1, 8, 9, 12, 16, 17, 24, 25, 32):
        P = planes_of(b)
        vals = []
        for i in range(ROWS):
            vals += families(b, ROW_LEN, seed=0x51DE + i)[family]
        want = cref.compress(cid, cref.row_msm(cid, plane_gens[cid][:ROW_LEN].copy(), as_scalars(vals), ROWS, ROW_LEN, mont=False))
        digits = []
        for row in plane_split(vals, ROW_LEN, b):
            d = [0] * (P * ROW_LEN)
            for p, j, byte in row:
                d[p * ROW_LEN + j] = byte
            digits += d
        got = cref.compress(cid, cref.row_msm(cid, plane_gens[cid][:P * ROW_LEN].copy(), as_scalars(digits), ROWS, P * ROW_LEN, mont=False))
        assert got == want, (family, b)
        if family == "zero":
            assert want == bytes(32 * ROWS)


def test_commit_symbols_refuses_other_dtypes_and_values_that_do_not_fit():
    """HyraxPC.check_symbols is what commit_symbols runs first, before any device call."""
    from reef_amd.provider import HyraxPC
    with pytest.raises(ValueError, match="uint8, uint16 or uint32"):
        HyraxPC.check_symbols(np.arange(16, dtype=np.int64), 8)
    with pytest.raises(ValueError, match="does not fit symbol_bits"):
        HyraxPC.check_symbols(as_symbols([0, 511, 512, 3], np.uint16), 9)
    with pytest.raises(ValueError, match="does not fit symbol_bits"):
        HyraxPC.check_symbols(as_symbols([0, 200], np.uint8), 7)
    with pytest.raises(ValueError, match="symbol_bits = 17"):
        HyraxPC.check_symbols(as_symbols([0, 1], np.uint16), 17)
    ok = HyraxPC.check_symbols(np.array([[0, 511], [256, 3]], dtype=np.uint16), 9)
    assert ok.dtype == np.uint16 and ok.shape == (4,)

    class Gens:                                                              # commit_symbols itself, on a provider that never reaches a device
        h = np.zeros(8, dtype=np.uint64)

        def __len__(self):
            return 4

        def _context(self):
            raise AssertionError("device call before the check")
        _on_devices = _context
        _devices = None
    pc = HyraxPC(Gens())
    bl = np.zeros((2, 4), dtype=np.uint64)
    with pytest.raises(ValueError):
        pc.commit_symbols(np.zeros(4, dtype=np.int64), bl, 8)
    with pytest.raises(ValueError):
        pc.commit_symbols(as_symbols([0, 1, 2, 1024], np.uint16), bl, 10)
