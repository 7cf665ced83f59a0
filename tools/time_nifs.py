"""Row N6: one NIFS step per shape on the device, host to host (reef_amd.nifs; include/reef_msm.h 3f).

    python tools/time_nifs.py [reps] [--quick]

Shapes: the secondary circuit (11 376 constraints) and the primary of cfg3 / cfg4 / cfg5 (27 790 / 39 484 / 1 032 421 rows:
tests/golden/replay_shapes.json).  The matrices are SYNTHETIC: 2-4 entries per row and matrix, coefficients drawn from +-1,
small values and full-width values (one in eight), and four long rows of 10^4 entries; num_vars = num_cons, num_io = 2.
They say nothing about Reef's real matrices.  Per shape: commit_T (of which the MSM of T alone, host to host), fold and
check_relaxed, median of `reps` calls, and the algorithmic bytes of each pass with their share of 8 TB/s of HBM.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import pasta_ref as R                     # noqa: E402
from reef_amd.msm import MsmContext                    # noqa: E402
from reef_amd.nifs import Nifs                         # noqa: E402
from _synthetic import synthetic_matrix                # noqa: E402

SHAPES = [("secondary", 11376), ("cfg3", 27790), ("cfg4", 39484), ("cfg5", 1032421)]
HBM = 8e12


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t) * 1e3)
    return statistics.median(ts)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
    shapes = SHAPES[:2] if "--quick" in sys.argv else SHAPES
    print(f"# tools/time_nifs.py: one NIFS step per shape, Pallas (scalars in Fq), SYNTHETIC matrices (2-4 entries per row and matrix, "
          f"four rows of 10^4 entries), median of {reps} calls, host to host; bytes are algorithmic, share of 8 TB/s")
    rng = np.random.default_rng(1)
    for name, n in shapes:
        nv, nio = n, 2
        nz = nv + 1 + nio
        long_rows = rng.choice(n, size=4, replace=False)
        nnz = general = 0
        with Nifs(0, n, nv, nio) as nf:
            for k in range(3):
                r, c, v, g = synthetic_matrix(rng, n, nz, long_rows)
                nf.set_matrix(k, r, c, v)
                nnz += r.shape[0]
                general += g
            w = rng.integers(0, 1 << 62, size=(nv, 4), dtype=np.uint64)
            x = rng.integers(0, 1 << 62, size=(nio, 4), dtype=np.uint64)
            one = np.array([[1, 0, 0, 0]], dtype=np.uint64)
            nf.set_running(w, None, one, x)
            bases = R.gen_bases_ap(0, 42, 5, n)
            with MsmContext(0, bases) as key:
                t_host = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
                key.msm(t_host, is_mont=False)
                nf.commit_t(key, w, x)                    # warm: the long-row list, the key's stream
                nf.fold(3)
                commit = timed(lambda: nf.commit_t(key, w, x), reps)
                msm_only = timed(lambda: key.msm(t_host, is_mont=False), reps)

                def step():
                    nf.commit_t(key, w, x)
                    nf.fold(12345)
                step_ms = timed(step, reps)
                check = timed(nf.check_relaxed, reps)
        fold = step_ms - commit
        # T pass: row pointers (3 matrices), {col, class} per entry, general coefficients, z1 and z2 at every entry, T out
        t_bytes = 3 * 4 * (n + 1) + 8 * nnz + 32 * general + 2 * 32 * nnz + 32 * n
        f_bytes = 3 * 32 * nz + 3 * 32 * n                     # z1 += r z2 and E += r T: two reads and a write each
        c_bytes = 3 * 4 * (n + 1) + 8 * nnz + 32 * general + 32 * nnz + 32 * n
        print(f"{name:9s} rows {n:8d}  nnz {nnz:9d} (general {general:8d})  commit_T {commit:8.3f} ms (MSM alone {msm_only:8.3f} ms)  "
              f"fold {fold:7.3f} ms  check_relaxed {check:7.3f} ms  |  bytes: T pass {t_bytes / 1e6:8.2f} MB = {t_bytes / HBM * 1e6:7.1f} us "
              f"at 8 TB/s, fold {f_bytes / 1e6:7.2f} MB = {f_bytes / HBM * 1e6:6.1f} us, check {c_bytes / 1e6:8.2f} MB = {c_bytes / HBM * 1e6:7.1f} us")


if __name__ == "__main__":
    main()
