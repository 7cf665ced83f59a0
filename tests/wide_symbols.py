"""Inputs for reef_msm_rows_symbols_wide (K2 from 16- and 32-bit document symbols) and the plane split the kernel implements, in plain
Python.  Shared by tests/test_rows_symbols_wide_host.py (no GPU: the model against the oracle) and tests/test_gpu_rows_symbols_wide.py."""
import random

import numpy as np

from row_patterns import to_limbs

FAMILY_NAMES = ("ones", "zero", "lone", "edges", "rand")
PLANE_EDGES = (255, 256, 257, 65535, 65536, 65537)


def families(b: int, row_len: int, seed: int = 0x51DE) -> dict:
    """Five rows of row_len symbols < 2^b, 1 <= b <= 32, by name:
      ones   2^b - 1 everywhere: every plane's last table entry
      zero   all zero: the identity row (or blind * H)
      lone   2^(b-1) at the last index, zero elsewhere: the top plane's top bit on one lane of the last, ragged wave
      edges  255, 256, 257, 65535, 65536, 65537 cut to b bits, repeated: bytes that are all ones, zero and one on either side of a plane
      rand   uniform below 2^b, fixed seed"""
    assert 1 <= b <= 32 and row_len >= 1
    mask = (1 << b) - 1
    rng = random.Random(seed * 1000 + b)
    rows = {
        "ones": [mask] * row_len,
        "zero": [0] * row_len,
        "lone": [0] * (row_len - 1) + [1 << (b - 1)],
        "edges": [PLANE_EDGES[j % 6] & mask for j in range(row_len)],
        "rand": [rng.randrange(1 << b) for _ in range(row_len)],
    }
    assert tuple(rows) == FAMILY_NAMES
    return rows


def batch(b: int, rows: int, row_len: int) -> list:
    """rows * row_len integers, row-major: one row of each family, cycled (every "rand" row after the first draws from a seed of its own)."""
    first = families(b, row_len)
    out = []
    for i in range(rows):
        name = FAMILY_NAMES[i % 5]
        out += first[name] if i < 5 or name != "rand" else families(b, row_len, seed=0x51DE + i)[name]
    return out


def as_symbols(values, dtype) -> np.ndarray:
    """The integers as the array the entry takes (uint16 / uint32; uint8 for the byte entry); every value must fit."""
    assert all(0 <= v < 1 << (8 * np.dtype(dtype).itemsize) for v in values)
    return np.array(values, dtype=dtype)


def as_scalars(values, r: int = 0, mont: bool = False) -> np.ndarray:
    """The same values as 4-limb scalars for the oracle."""
    return to_limbs(values, r, mont)


def planes_of(b: int) -> int:
    return (b + 7) // 8


def plane_split(values, row_len: int, b: int) -> list:
    """symbols (row-major, any number of rows) -> per row the list of (plane, j, byte): byte_p of the symbol at column j, masked to b bits first.
    sum_j s_j G_j = sum over the triples of byte * (256^plane * G_j)."""
    assert len(values) % row_len == 0
    mask, P = (1 << b) - 1, planes_of(b)
    out = []
    for r0 in range(0, len(values), row_len):
        out.append([(p, j, ((values[r0 + j] & mask) >> (8 * p)) & 0xFF) for j in range(row_len) for p in range(P)])
    return out
