"""Row N5: the two sum-checks of the final SNARK on the device, host to host (reef_amd.spartan; include/reef_msm.h 3g).

    python tools/time_spartan.py [reps] [--quick]

Per curve and padded size (num_cons_pad = num_vars_pad = 2^14, 2^15, 2^16, 2^20): a NIFS ctx with SYNTHETIC matrices (the
generator of tools/_synthetic.py: 2-4 entries per row and matrix, one coefficient in eight full-width, four long rows of 10^4
entries; num_cons = num_vars = the padded size minus 3, num_io = 2) and a random running instance.  They say nothing about
Reef's real matrices.  Reported: begin (the row pass, eq(tau), round 0), the mean outer round, outer_claims, inner_begin (the ABC
pass and round 0), the mean inner round, inner_claims and the whole prove, each the median over `reps` proves, host to host.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run of this script."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from reef_amd.nifs import Nifs                         # noqa: E402
from reef_amd.spartan import Spartan                   # noqa: E402
from _synthetic import synthetic_matrix                # noqa: E402

SIZES = [14, 15, 16, 20]


def one_prove(sp, ncp, nvp, rng):
    """One whole prove with random challenges below 2^250; returns the wall time of each call in ms."""
    ell_x, ell_y = ncp.bit_length() - 1, (2 * nvp).bit_length() - 1
    ch = [int(rng.integers(0, 1 << 62)) << 188 | int(rng.integers(0, 1 << 62)) for _ in range(ell_x + ell_y + 1)]
    t = {"begin": [], "outer_round": [], "outer_claims": [], "inner_begin": [], "inner_round": [], "inner_claims": []}

    def call(name, fn, *a):
        t0 = time.perf_counter()
        fn(*a)
        t[name].append((time.perf_counter() - t0) * 1e3)
    call("begin", sp.begin, ncp, nvp, ch[:ell_x])
    for k in range(ell_x - 1):
        call("outer_round", sp.outer_round, ch[k])
    call("outer_claims", sp.outer_claims, ch[ell_x - 1])
    call("inner_begin", sp.inner_begin, ch[ell_x])
    for k in range(ell_y - 1):
        call("inner_round", sp.inner_round, ch[ell_x + 1 + k])
    call("inner_claims", sp.inner_claims, ch[-1])
    return {k: statistics.mean(v) for k, v in t.items()}, sum(sum(v) for v in t.values())


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
    sizes = SIZES[:2] if "--quick" in sys.argv else SIZES
    print(f"# tools/time_spartan.py: one prove of both sum-checks per curve and padded size, SYNTHETIC matrices (tools/time_nifs.py's "
          f"generator), num_cons = num_vars = pad - 3, median over {reps} proves, host to host, ms; rounds are the mean call of the prove")
    rng = np.random.default_rng(1)
    for curve in (0, 1):
        for lg in sizes:
            pad = 1 << lg
            n, nio = pad - 3, 2
            nz = n + 1 + nio
            long_rows = rng.choice(n, size=4, replace=False)
            nnz = 0
            with Nifs(curve, n, n, nio) as nf:
                for k in range(3):
                    r, c, v, _ = synthetic_matrix(rng, n, nz, long_rows)
                    nf.set_matrix(k, r, c, v)
                    nnz += r.shape[0]
                w = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
                e = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
                x = rng.integers(0, 1 << 62, size=(nio, 4), dtype=np.uint64)
                u = np.array([[7, 0, 0, 0]], dtype=np.uint64)
                nf.set_running(w, e, u, x)
                sp = Spartan(nf)
                one_prove(sp, pad, pad, rng)                      # warm: the workspace, the long-column list
                runs = [one_prove(sp, pad, pad, rng) for _ in range(reps)]
            med = {k: statistics.median(r[0][k] for r in runs) for k in runs[0][0]}
            total = statistics.median(r[1] for r in runs)
            print(f"{'pallas' if curve == 0 else 'vesta ':6s} pad 2^{lg:2d}  nnz {nnz:9d}  begin {med['begin']:7.3f}  outer round {med['outer_round']:6.3f} "
                  f"x {lg - 1:2d}  outer_claims {med['outer_claims']:6.3f}  inner_begin (ABC) {med['inner_begin']:7.3f}  inner round "
                  f"{med['inner_round']:6.3f} x {lg:2d}  inner_claims {med['inner_claims']:6.3f}  total {total:7.3f} ms")


if __name__ == "__main__":
    main()
