"""Times the verifier's matrix evaluations at m points in ONE reef_spartan_eval_matrices_batch call (include/reef_msm.h 3o) against the
code that existed: a loop of m reef_spartan_eval_matrices calls (3k), timed as a whole in the same run.

    python tools/time_spartan_verify_batch.py [reps] [log2 pad ...] [--curve 0|1]   -> text lines (profiles/r21_spartan_eval_batch_timing.txt)

Per curve and padded size (num_cons_pad = num_vars_pad = 2^14, 2^16, 2^20 unless given): a NIFS ctx with SYNTHETIC matrices only
(tools/_synthetic.py, as tools/time_spartan_verify.py makes them: num_cons = num_vars = pad - 3, num_io = 2, four long rows of 10^4
entries) and no running instance.  They say nothing about Reef's real matrices.  m = 1, 2, 16, 64 random points.  Both routes are C
calls on arguments marshalled beforehand, host to host; before anything is timed the tool asserts that they return the same bytes.
Three warm calls of each route, then `reps` (30) timed ones, the routes alternately; ms: median, p10, min, max.  The workspace budget
is the default, under which 2^20 x 64 runs in groups: reef_spartan_eval_matrices_batch_last_info is printed for every cell.
The condition, per cell with m >= 2: median(batch) <= p10(loop) -- the loop's own spread and nothing else.  For m = 1 the batch does
the single call's work by another route: its median may exceed the single call's median by at most that call's max - min in the same
run.  A cell that misses is marked FAILS; none is left out.  Kernel times come from a separate `rocprofv3 --kernel-trace --stats`
run of this script at one size."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from reef_amd import _ffi, msm                         # noqa: E402
from reef_amd._fe import _arr                          # noqa: E402
from reef_amd.nifs import Nifs                         # noqa: E402
from _synthetic import synthetic_matrix                # noqa: E402

WARM = 3
MS = (1, 2, 16, 64)
lib = _ffi.load()


def batch_call(nf, pad, xs, ys, m):
    """one reef_spartan_eval_matrices_batch call on arguments marshalled once: () -> the 3 m results' bytes"""
    xa, ya, out = _arr([x for r in xs[:m] for x in r]), _arr([y for r in ys[:m] for y in r]), np.zeros((3 * m, 4), np.uint64)

    def run(_keep=(xa, ya, out)):
        _ffi.check(lib.reef_spartan_eval_matrices_batch(nf._h, pad, pad, xa.ctypes.data, ya.ctypes.data, m, False, out.ctypes.data))
        return out.tobytes()
    return run


def loop_call(nf, pad, xs, ys, m):
    """the parent commit's route: m reef_spartan_eval_matrices calls"""
    xa, ya, out = [_arr(r) for r in xs[:m]], [_arr(r) for r in ys[:m]], np.zeros((3 * m, 4), np.uint64)

    def run(_keep=(xa, ya, out)):
        for t in range(m):
            _ffi.check(lib.reef_spartan_eval_matrices(nf._h, pad, pad, xa[t].ctypes.data, ya[t].ctypes.data, False, out[3 * t:].ctypes.data))
        return out.tobytes()
    return run


def stats(ts):
    ts = sorted(ts)
    return statistics.median(ts), ts[len(ts) // 10], ts[0], ts[-1]


def fmt(s):
    return f"median {s[0]:9.3f} p10 {s[1]:9.3f} min {s[2]:9.3f} max {s[3]:9.3f}"


def main():
    args = sys.argv[1:]
    curves = (0, 1)
    if "--curve" in args:
        k = args.index("--curve")
        curves = (int(args[k + 1]),)
        del args[k:k + 2]
    nums = [int(a) for a in args if a.isdigit()]
    reps = nums[0] if nums else 30
    sizes = nums[1:] or [14, 16, 20]
    print(f"# {lib.reef_version().decode()}, library sources {_ffi.library_sources_sha16()}: A~, B~, C~ at m points host to host on a ctx with "
          f"matrices only, SYNTHETIC matrices (tools/_synthetic.py), num_cons = num_vars = pad - 3.  batch: one reef_spartan_eval_matrices_batch "
          f"call; loop: m reef_spartan_eval_matrices calls, timed as a whole (the parent commit's code).  {WARM} warm calls of each, then {reps} "
          f"timed, the routes alternately; ms.  Condition: m >= 2: median(batch) <= p10(loop); m = 1: median(batch) - median(single) <= "
          f"max(single) - min(single).")
    failed = []
    rng = np.random.default_rng(1)
    for curve in curves:
        p = msm.SCALAR_MODULUS[curve]
        cname = "pallas" if curve == 0 else "vesta "
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
                rand = lambda: int.from_bytes(rng.bytes(40), "little") % p
                xs = [[rand() for _ in range(lg)] for _ in range(max(MS))]
                ys = [[rand() for _ in range(lg + 1)] for _ in range(max(MS))]
                for m in MS:
                    batch, loop = batch_call(nf, pad, xs, ys, m), loop_call(nf, pad, xs, ys, m)
                    for _ in range(WARM):
                        want = loop()
                        assert batch() == want, f"pad 2^{lg}, m = {m}: the routes disagree"
                    tb, tl = [], []
                    for _ in range(reps):
                        t0 = time.perf_counter()
                        batch()
                        tb.append((time.perf_counter() - t0) * 1e3)
                        t0 = time.perf_counter()
                        loop()
                        tl.append((time.perf_counter() - t0) * 1e3)
                    info = nf.eval_batch_last_info()
                    bs, ls = stats(tb), stats(tl)
                    if m == 1:
                        ok = bs[0] - ls[0] <= ls[3] - ls[2]
                        rule = f"batch - single {bs[0] - ls[0]:+.3f} against the single call's spread {ls[3] - ls[2]:.3f}"
                    else:
                        ok = bs[0] <= ls[1]
                        rule = f"loop/batch {ls[0] / bs[0]:6.2f}"
                    print(f"{cname} pad 2^{lg:2d} nnz {nnz:9d} m={m:2d}  batch {fmt(bs)} per point {bs[0] / m:8.3f} | loop {fmt(ls)} per point "
                          f"{ls[0] / m:8.3f} | {rule} | groups {info['groups']} x {info['points_per_group']} points, tables "
                          f"{info['workspace_bytes'] / 1e6:.1f} MB | {'ok' if ok else 'FAILS the condition'}", flush=True)
                    if not ok:
                        failed.append(f"{cname.strip()} 2^{lg} m={m}")
    print("# every cell meets its condition" if not failed else "# cells that FAIL their condition: " + ", ".join(failed))


if __name__ == "__main__":
    main()
