"""The verifier's matrix evaluations (reef_spartan_eval_matrices, include/reef_msm.h 3k) host to host.

    python tools/time_spartan_verify.py [reps] [log2 pad ...] [--curve 0|1]      -> text lines (profiles/r11_spartan_verify_timing.txt)

Per curve and padded size (num_cons_pad = num_vars_pad = 2^14, 2^15, 2^16, 2^20 unless given): a NIFS ctx with SYNTHETIC matrices only
(tools/_synthetic.py: 2-4 entries per row and matrix, one coefficient in eight full-width, four long rows of 10^4 entries; num_cons =
num_vars = the padded size minus 3, num_io = 2) and NO running instance -- a verifier's ctx.  They say nothing about Reef's real
matrices.  Reported: the call at a random point, median / min / max over `reps` calls after three warm ones, and the algorithmic
bytes of one call computed from the shape -- per entry the {col, class} word and a 32-byte gather of a column weight, 32 bytes more
for a general coefficient's side-table entry; per row three row pointers and eq(r_x)[row]; the two eq tables written once -- with
the GB/s they give at the median.  The host side of the comparison is `reef_replay cfgN prove` (verify_evals_host_ms_*: the loop of
the host check on one core).  Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script at one size."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from reef_amd import _ffi, msm                         # noqa: E402
from reef_amd.nifs import Nifs                         # noqa: E402
from reef_amd.verify import matrix_evals               # noqa: E402
from _synthetic import synthetic_matrix                # noqa: E402

WARM = 3


def main():
    args = sys.argv[1:]
    curves = (0, 1)
    if "--curve" in args:
        k = args.index("--curve")
        curves = (int(args[k + 1]),)
        del args[k:k + 2]
    nums = [int(a) for a in args if a.isdigit()]
    reps = nums[0] if nums else 30
    sizes = nums[1:] or [14, 15, 16, 20]
    print(f"# {_ffi.load().reef_version().decode()}, library sources {_ffi.library_sources_sha16()}: reef_spartan_eval_matrices host to host on a ctx "
          f"with matrices only, SYNTHETIC matrices (tools/_synthetic.py), num_cons = num_vars = pad - 3, {WARM} warm calls then {reps} calls; ms")
    rng = np.random.default_rng(1)
    for curve in curves:
        p = msm.SCALAR_MODULUS[curve]
        for lg in sizes:
            pad = 1 << lg
            n, nio = pad - 3, 2
            nz = n + 1 + nio
            long_rows = rng.choice(n, size=4, replace=False)
            nnz = general = 0
            with Nifs(curve, n, n, nio) as nf:
                for k in range(3):
                    r, c, v, full = synthetic_matrix(rng, n, nz, long_rows)
                    nf.set_matrix(k, r, c, v)
                    nnz += r.shape[0]
                    general += full
                rand = lambda: int.from_bytes(rng.bytes(40), "little") % p
                r_x, r_y = [rand() for _ in range(lg)], [rand() for _ in range(lg + 1)]
                ts = []
                for i in range(WARM + reps):
                    t0 = time.perf_counter()
                    matrix_evals(nf, pad, pad, r_x, r_y)
                    if i >= WARM:
                        ts.append((time.perf_counter() - t0) * 1e3)
            med = statistics.median(ts)
            nbytes = nnz * (8 + 32) + general * 32 + n * (3 * 4 + 32) + (n + nz) * 32
            print(f"{'pallas' if curve == 0 else 'vesta ':6s} pad 2^{lg:2d}  rows {n:8d}  nnz {nnz:9d} ({general} general)  eval_matrices median {med:7.3f} "
                  f"min {min(ts):7.3f} max {max(ts):7.3f} ms  algorithmic {nbytes / 1e6:8.2f} MB -> {nbytes / med / 1e6:7.1f} GB/s  "
                  f"({med * 1e6 / nnz:6.2f} ns/entry)", flush=True)


if __name__ == "__main__":
    main()
