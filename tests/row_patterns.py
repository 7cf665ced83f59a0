"""Adversarial scalar rows for the width-dependent routes of reef_msm_rows (K2): every scalar is a Python integer below
min(2^b, r), and every batch holds a scalar of exactly b bits, so that a measured width (k_max_bits) and a declared one
(max_scalar_bits = b) agree.  Shared by tests/test_rows_patterns.py (no GPU: the generator and the oracle on these inputs) and
tests/test_gpu_rows_widths.py (the kernels against the oracle)."""
import random

import numpy as np

PATTERN_NAMES = ("ones", "lone", "half", "half+1", "rand")
# Batches of fewer than five rows take the patterns in this order: the row that fixes the width and carries through every window
# first, then the digits that must be negated, then the width hanging on one lane.
ROW_PRIORITY = ("ones", "half+1", "lone", "half", "rand")


def window_of(j: int) -> int:
    """c_j = 2 + (j mod 16): the window size index j of a "half" / "half+1" row is aligned to; 2..17 covers every window the engine can choose
    for a row MSM (the single signed window has 2..13 bits, a plain key at most 11, a pre-shifted key its own 2..17 at these sizes)."""
    return 2 + (j % 16)


def repeat_digit(digit: int, c: int, b: int) -> int:
    """`digit` at every multiple of c bits, cut to b bits."""
    v = 0
    for pos in range(0, b, c):
        v |= digit << pos
    return v & ((1 << b) - 1)


def patterns(b: int, row_len: int, r: int, seed: int = 0x5EED) -> dict:
    """Five rows of row_len scalars < min(2^b, r), 1 <= b <= 255, by name:
      ones    2^b - 1 everywhere (r - 1 for b = 255): a carry through every window of every size
      lone    2^(b-1) at the last index, zero elsewhere: the width hangs on one lane of the last, ragged wave
      half    index j: the digit 2^(c_j - 1) at stride c_j, cut to b bits -- the top bucket, which must NOT be negated
      half+1  index j: the digit 2^(c_j - 1) + 1 at stride c_j, cut to b bits -- the smallest digit that MUST be negated
      rand    uniform below min(2^b, r), fixed seed
    For b = 255 a cut that is not below r loses its top bit (r is just above 2^254, so the digits below bit 254 stay as they are)."""
    assert 1 <= b <= 255 and row_len >= 1
    bound = min(1 << b, r)

    def fit(v):
        return v if v < bound else v & ((1 << (b - 1)) - 1)

    half = [fit(repeat_digit(1 << (c - 1), c, b)) for c in range(2, 18)]             # sixteen distinct values, by window size
    half1 = [fit(repeat_digit((1 << (c - 1)) + 1, c, b)) for c in range(2, 18)]
    rng = random.Random(seed * 1000 + b)
    rows = {
        "ones": [bound - 1] * row_len,
        "lone": [0] * (row_len - 1) + [1 << (b - 1)],
        "half": [half[window_of(j) - 2] for j in range(row_len)],
        "half+1": [half1[window_of(j) - 2] for j in range(row_len)],
        "rand": [rng.randrange(bound) for _ in range(row_len)],
    }
    assert tuple(rows) == PATTERN_NAMES
    return rows


def batch(b: int, rows: int, row_len: int, r: int) -> list:
    """rows * row_len integers, row-major: the pattern rows in ROW_PRIORITY order, cycled (every "rand" row after the first draws from
    a seed of its own).  Row 0 is always "ones", so every batch holds a scalar of exactly b bits."""
    first = patterns(b, row_len, r)
    out = []
    for i in range(rows):
        name = ROW_PRIORITY[i % 5]
        out += first[name] if i < 5 or name != "rand" else patterns(b, row_len, r, seed=0x5EED + i)[name]
    return out


def to_limbs(values, r: int = 0, mont: bool = False) -> np.ndarray:
    """Integers -> (n, 4) uint64 limbs, little-endian; mont: v * 2^256 mod r, the ABI's Montgomery form (is_mont = True)."""
    if mont:
        values = [(v << 256) % r for v in values]
    raw = b"".join(v.to_bytes(32, "little") for v in values)
    return np.frombuffer(raw, dtype="<u8").reshape(-1, 4).astype(np.uint64)


def boundary_widths(c: int) -> list:
    """The widths at which a route or a window count changes: the fixed ones (around the symbol tables' 8, the single window's
    12 / 13, two and three 13-bit windows, the top), and k*c - 1, k*c, k*c + 1 for a key's own window c at k = 2 and at the
    largest k with k*c < 255 (W = ceil((b + 1) / c) steps at b = k*c)."""
    ws = {9, 12, 13, 14, 25, 26, 27, 254, 255}
    for k in (2, (255 - 1) // c):
        ws |= {k * c - 1, k * c, k * c + 1}
    return sorted(w for w in ws if 1 <= w <= 255)
