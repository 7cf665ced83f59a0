"""The SYNTHETIC R1CS matrices of the timing scripts (time_nifs.py, time_spartan.py, time_spartan_open.py): 2-4 entries per row,
coefficients drawn from +1, small values and full-width values (one in eight), and long rows of 10^4 entries.  They say nothing
about Reef's real matrices."""
import numpy as np


def synthetic_matrix(rng, n, nz, long_rows):
    lens = rng.integers(2, 5, size=n)
    lens[long_rows] = 10000
    rows = np.repeat(np.arange(n, dtype=np.uint32), lens)
    cols = rng.integers(0, nz, size=rows.shape[0], dtype=np.uint32)
    kind = rng.integers(0, 8, size=rows.shape[0])
    vals = np.zeros((rows.shape[0], 4), dtype=np.uint64)
    vals[:, 0] = np.where(kind < 4, 1, rng.integers(2, 1 << 16, size=rows.shape[0]))     # +1, or a small value
    full = kind == 7                                                                       # one in eight: full width (< 2^250)
    vals[full] = rng.integers(0, 1 << 62, size=(int(full.sum()), 4), dtype=np.uint64)
    return rows, cols, vals, int(full.sum())
