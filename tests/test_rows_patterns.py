"""No GPU: the adversarial rows of tests/row_patterns.py are what they claim to be, and the C oracle (cref.row_msm) is right on them -- checked
against the definition sum_i k_i * P_i + blind * H in plain Python integers (oracle.pasta_oracle) -- before tests/test_gpu_rows_widths.py compares a
kernel with it."""
import numpy as np
import pytest

from oracle.pasta_oracle import CURVES
from row_patterns import PATTERN_NAMES, ROW_PRIORITY, batch, boundary_widths, patterns, repeat_digit, to_limbs, window_of

CID = {"pallas": 0, "vesta": 1}


@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_patterns_hold_their_width_at_every_b(name):
    """Every b in 1..255: all values below min(2^b, r), and a value of exactly b bits in the batch."""
    r = CURVES[name].order
    for b in range(1, 256):
        rows = patterns(b, 37, r)
        assert tuple(rows) == PATTERN_NAMES
        flat = [v for row in rows.values() for v in row]
        assert len(flat) == 5 * 37
        assert all(0 <= v < r and v < (1 << b) for v in flat), b
        assert max(v.bit_length() for v in flat) == b, b
        assert rows["ones"][0].bit_length() == b and rows["lone"][-1].bit_length() == b, b
        for rows_n in (1, 2, 3, 7):                                  # every batch, whatever its row count, starts with the row that fixes the width
            got = batch(b, rows_n, 37, r)
            assert len(got) == rows_n * 37 and got[:37] == rows["ones"] and max(v.bit_length() for v in got) == b


@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_pattern_rows_have_the_described_shape(name):
    r = CURVES[name].order
    row_len = 70                                                    # four full cycles of c_j and a ragged fifth
    assert [window_of(j) for j in range(18)] == list(range(2, 18)) + [2, 3]
    for b in (1, 2, 7, 12, 13, 14, 26, 64, 65, 130, 254, 255):
        rows = patterns(b, row_len, r)
        top = r - 1 if b == 255 else (1 << b) - 1
        assert rows["ones"] == [top] * row_len
        assert rows["lone"] == [0] * (row_len - 1) + [1 << (b - 1)]
        assert rows["rand"] == patterns(b, row_len, r)["rand"]      # a fixed seed ...
        assert b < 7 or rows["rand"] != patterns(b, row_len, r, seed=1)["rand"]   # ... that matters
        for pname, extra in (("half", 0), ("half+1", 1)):
            for j, v in enumerate(rows[pname]):
                c = window_of(j)
                digit = (1 << (c - 1)) + extra
                full = sum(digit << pos for pos in range(0, b, c)) & ((1 << b) - 1)
                assert full == repeat_digit(digit, c, b)
                if full < r:
                    assert v == full, (b, j)
                    # every whole window below b holds the digit itself
                    assert all(((v >> pos) & ((1 << c) - 1)) == digit for pos in range(0, b - c + 1, c)), (b, j)
                else:                                               # b = 255 only: the top bit gives way, the digits below it stay
                    assert b == 255 and v == full - (1 << 254), (b, j)
    assert set(ROW_PRIORITY) == set(PATTERN_NAMES) and ROW_PRIORITY[0] == "ones"
    assert boundary_widths(13) == [9, 12, 13, 14, 25, 26, 27, 246, 247, 248, 254, 255]
    assert boundary_widths(7) == [9, 12, 13, 14, 15, 25, 26, 27, 251, 252, 253, 254, 255]


def test_limbs_and_montgomery_form():
    r = CURVES["pallas"].order
    vals = [0, 1, (1 << 64) - 1, 1 << 64, r - 1, (1 << 254) + 5]
    limbs = to_limbs(vals)
    assert limbs.dtype == np.uint64 and limbs.shape == (6, 4) and limbs.flags["C_CONTIGUOUS"] and limbs.flags["WRITEABLE"]
    assert [sum(int(x) << (64 * i) for i, x in enumerate(row)) for row in limbs] == vals
    mont = to_limbs(vals, r, mont=True)
    assert [sum(int(x) << (64 * i) for i, x in enumerate(row)) for row in mont] == [v * (1 << 256) % r for v in vals]


@pytest.mark.parametrize("b", [1, 12, 13, 26, 27, 254, 255])
@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_c_oracle_equals_the_big_integer_sum_on_the_patterns(name, b, cref):
    """cref.row_msm on the five pattern rows (row_len = 40, blinds on, both scalar forms) against sum_i k_i * P_i + blind * H by
    double-and-add over Python integers."""
    C, cid = CURVES[name], CID[name]
    r = C.order
    row_len = 40
    bases = cref.gen_bases_ap(cid, 0xA11CE, 3, row_len)
    h = cref.gen_bases_ap(cid, 0xB11D, 1, 1)[0].copy()
    pts = [C.affine_from_bytes(bases[i].tobytes()) for i in range(row_len)]
    hpt = C.affine_from_bytes(h.tobytes())
    assert all(C.is_on_curve(p) for p in pts) and C.is_on_curve(hpt)
    flat = batch(b, 5, row_len, r)
    blinds = [cref.limbs_to_int(x) for x in cref.gen_scalars(cid, 0xB1 + b, 5, mont=False)]
    blinds[1] = 0                                                   # a row whose blind term vanishes
    want = b"".join(C.compress(C.add(C.msm_naive(flat[i * row_len:(i + 1) * row_len], pts), C.mul(blinds[i], hpt))) for i in range(5))
    want_nb = b"".join(C.compress(C.msm_naive(flat[i * row_len:(i + 1) * row_len], pts)) for i in range(5))
    for mont in (False, True):
        sc, bl = to_limbs(flat, r, mont), to_limbs(blinds, r, mont)
        assert cref.compress(cid, cref.row_msm(cid, bases, sc, 5, row_len, h=h, blinds=bl, mont=mont, threads=2)) == want, mont
        assert cref.compress(cid, cref.row_msm(cid, bases, sc, 5, row_len, mont=mont, threads=2)) == want_nb, mont
