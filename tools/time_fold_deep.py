"""The deep fold (reef_fold_deep, reef_msm_ctx_create_folded) and the arguments with their late rounds on a folded key
(reef_hyrax_set_small_key, reef_spartan_open_set_small_key), timed; writes profiles/r17_fold_deep_timing.txt.

    python tools/time_fold_deep.py [--parent DIR] [--out FILE]     every step below as a child process under its own time limit, chained
    python tools/time_fold_deep.py --fold [reps]       reef_fold_deep and reef_msm_ctx_create_folded host to host
    python tools/time_fold_deep.py --kernels LOGN      (under rocprofv3 --kernel-trace --stats) the same calls at n = 2^LOGN, for the per-kernel times
    python tools/time_fold_deep.py --hyrax [reps]      the whole Hyrax argument at R = 2^11 and 2^13, switch off and at every target size
    python tools/time_fold_deep.py --open [reps]       the whole opening at n = 2^16 and 2^20, the same

Pallas throughout.  n = 2^11, 2^13, 2^16, 2^20; target sizes 256, 512, 1024, 4096 (those below n); source keys plain (default options)
and pre-shifted (bucket_groups = 1).  Every figure is the median over `reps` repetitions in one process, with the spread (min .. max)
beside it; the folded key of a repetition is a fresh one (made and destroyed inside it), the challenges are fresh random scalars.  The
"off" column of the arguments is the run of tools/time_hyrax_eval.py / tools/time_spartan_open.py (their functions are called); with
--parent DIR those two tools of another checkout (the parent commit, built) run in the same job and their output goes into the file."""
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

P = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001   # Pallas scalars (Fq)
LOGNS = (11, 13, 16, 20)
TARGETS = (256, 512, 1024, 4096)


def rand_fe(rng):
    return (int(rng.integers(1, 1 << 62)) << 188 | int(rng.integers(0, 1 << 62))) % P


def med(xs):
    return f"{statistics.median(xs):8.3f} ({min(xs):7.3f} .. {max(xs):7.3f})"


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def fold_calls(key, k, n_k, rng, reps, out_dev):
    """(reef_fold_deep to a device buffer, reef_msm_ctx_create_folded with bucket_groups = 1 and its destruction), ms per repetition"""
    fold, create = [], []
    for _ in range(reps):
        w1s, w2s = [rand_fe(rng) for _ in range(k)], [rand_fe(rng) for _ in range(k)]
        fold.append(timed(lambda: key.fold_deep(w1s, w2s, out_dev))[0])
        ms, small = timed(lambda: key.folded(w1s, w2s))
        create.append(ms)
        small.close()
    return fold, create


def step_fold(reps):
    from reef_amd import msm
    rng = np.random.default_rng(17)
    print(f"# reef_fold_deep (result left on the device) and reef_msm_ctx_create_folded (bucket_groups = 1: nibble tables up to 1024 points, "
          f"pre-shifted tables above), host to host, ms: median (min .. max) over {reps} calls with fresh challenges, one warm-up call before")
    for lg in LOGNS:
        n = 1 << lg
        bases = msm.gen_bases(0, 42, 5, n)
        for groups, kind in ((0, "plain"), (1, "pre-shifted")):
            with msm.MsmContext(0, bases, bucket_groups=groups) as key:
                for target in TARGETS:
                    if target >= n:
                        continue
                    k = lg - (target.bit_length() - 1)
                    out_dev = msm.DeviceBuffer(64 * target)
                    fold_calls(key, k, target, rng, 1, out_dev)
                    fold, create = fold_calls(key, k, target, rng, reps, out_dev)
                    out_dev.free()
                    print(f"n 2^{lg:2d}  source {kind:11s}  target {target:4d} (k = {k:2d})  fold_deep {med(fold)}  create_folded {med(create)}", flush=True)
    # what the folded key's own tables cost: a key of `target` given points made the ordinary way (the deep fold is the difference)
    for target in TARGETS:
        bases = msm.gen_bases(0, 42, 5, target)
        dev = msm.DeviceBuffer.from_host(bases)
        ts = []
        for _ in range(reps + 1):
            ms, key = timed(lambda: msm.MsmContext(0, dev, target, bucket_groups=1))
            ts.append(ms)
            key.close()
        print(f"reef_msm_ctx_create of {target:4d} device points, bucket_groups = 1 (the tables of the folded key alone)  {med(ts[1:])}", flush=True)


def step_kernels(lg):
    """a fixed number of calls for rocprofv3's kernel statistics: 5 deep folds and 5 folded keys of 1024 points from a pre-shifted key"""
    from reef_amd import msm
    rng = np.random.default_rng(5)
    n = 1 << lg
    with msm.MsmContext(0, msm.gen_bases(0, 42, 5, n), bucket_groups=1) as key:
        out_dev = msm.DeviceBuffer(64 * 1024)
        fold_calls(key, lg - 10, 1024, rng, 5, out_dev)


def kernel_stats(lg, limit):
    """per-kernel mean device time of step_kernels(lg) from rocprofv3's statistics, as text lines"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
               sys.executable, os.path.abspath(__file__), "--kernels", str(lg)]
        run = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if run.returncode != 0:
            return run.returncode, [f"rocprofv3 failed with {run.returncode}: {run.stderr[-400:]}"]
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return 1, ["rocprofv3 left no kernel_stats.csv"]
        import csv
        lines = [f"# kernels of 5 reef_fold_deep + 5 reef_msm_ctx_create_folded calls, n = 2^{lg}, pre-shifted source, 1024 folded points "
                 f"(rocprofv3 --kernel-trace --stats): calls, mean us, share of the device time"]
        for row in csv.DictReader(open(files[0])):
            name = row["Name"].split("(")[0].replace("void reef::", "")
            lines.append(f"  {name:44s} calls {int(row['Calls']):4d}  mean {float(row['AverageNs']) / 1e3:9.1f} us  {float(row['Percentage']):5.1f} %")
        return 0, lines


def step_hyrax(reps):
    from reef_amd import msm
    from reef_amd.hyrax import HyraxEval, factored_lens
    from time_hyrax_eval import one_argument
    rng = np.random.default_rng(3)
    print(f"# the whole Hyrax argument (eval_begin .. finish, random challenges, no h term), 2^num_vars random 1-byte symbols, host to host, ms: "
          f"median (min .. max) over {reps} arguments after one warm-up; small_key off = the run of tools/time_hyrax_eval.py")
    for num_vars in (22, 25):
        left, right = factored_lens(num_vars)
        n = 1 << right
        z = rng.integers(0, 256, size=1 << num_vars, dtype=np.uint64).astype(np.uint8)
        point = [rand_fe(rng) for _ in range(num_vars)]
        bases = msm.gen_bases(0, 42, 5, n)
        q = msm.gen_bases(0, 1000003, 1, 1)[0]
        for groups, kind in ((0, "plain"), (1, "pre-shifted")):
            with HyraxEval(0, z, num_vars) as hx, msm.MsmContext(0, bases, bucket_groups=groups) as key:
                for ns in (0,) + tuple(t for t in TARGETS if t < n):
                    hx.set_small_key(ns)
                    one_argument(hx, key, point, q, rng)
                    totals = [one_argument(hx, key, point, q, rng)[1] for _ in range(reps)]
                    print(f"R 2^{right:2d} (num_vars {num_vars})  source {kind:11s}  small_key {ns if ns else 'off':>4}  total {med(totals)}", flush=True)


def step_open(reps):
    from reef_amd import msm
    from reef_amd.nifs import Nifs
    from reef_amd.spartan import Opening, Spartan
    from _synthetic import synthetic_matrix
    from time_spartan import one_prove
    from time_spartan_open import one_opening
    rng = np.random.default_rng(2)
    print(f"# the whole batched opening (begin .. finish, random challenges) after one prove of the sum-checks, SYNTHETIC matrices, n = pad, key with "
          f"default options, host to host, ms: median (min .. max) over {reps} openings after one warm-up; small_key off = the run of tools/time_spartan_open.py")
    for lg in (16, 20):
        pad = 1 << lg
        n, nio = pad - 3, 2
        nz = n + 1 + nio
        long_rows = rng.choice(n, size=4, replace=False)
        bases = msm.gen_bases(0, 42, 5, pad)
        q = msm.gen_bases(0, 1000003, 1, 1)[0]
        with Nifs(0, n, n, nio) as nf, msm.MsmContext(0, bases) as key:
            for k in range(3):
                r, c, v, _ = synthetic_matrix(rng, n, nz, long_rows)
                nf.set_matrix(k, r, c, v)
            w = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
            e = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
            x = rng.integers(0, 1 << 62, size=(nio, 4), dtype=np.uint64)
            nf.set_running(w, e, np.array([[7, 0, 0, 0]], dtype=np.uint64), x)
            one_prove(Spartan(nf), pad, pad, rng)
            op = Opening(nf)
            kind = "pre-shifted" if key.plan()["bucket_groups"] == 1 else "plain"
            for ns in (0,) + TARGETS:
                op.set_small_key(ns)
                one_opening(op, key, pad, q, rng)
                totals = [one_opening(op, key, pad, q, rng)[1] for _ in range(reps)]
                print(f"n 2^{lg:2d}  source {kind:11s}  small_key {ns if ns else 'off':>4}  total {med(totals)}", flush=True)


def child(args, limit, cwd=ROOT, script=None):
    """one step as a process of its own under `timeout`; (exit status, its output)"""
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, script or os.path.abspath(__file__)] + args
    run = subprocess.run(cmd, capture_output=True, text=True, cwd=cwd)
    tail = [ln for ln in run.stdout.splitlines() if ln.strip()]
    if run.returncode != 0:
        tail.append(f"exit status {run.returncode}: {run.stderr[-600:]}")
    return run.returncode, tail


def main():
    argv = sys.argv[1:]
    reps = next((int(a) for a in argv if a.isdigit()), None)
    if "--fold" in argv:
        return step_fold(reps or 9)
    if "--kernels" in argv:
        return step_kernels(int(argv[argv.index("--kernels") + 1]))
    if "--hyrax" in argv:
        return step_hyrax(reps or 9)
    if "--open" in argv:
        return step_open(reps or 7)
    from reef_amd import _ffi
    out_path = argv[argv.index("--out") + 1] if "--out" in argv else os.path.join(ROOT, "profiles", "r17_fold_deep_timing.txt")
    parent = os.path.abspath(argv[argv.index("--parent") + 1]) if "--parent" in argv else None
    lines = [f"# tools/time_fold_deep.py on library sources {_ffi.library_sources_sha16()} ({_ffi.load().reef_version().decode()}); Pallas; every step a "
             f"process of its own"]
    steps = [(lambda: child(["--fold"], 300)), (lambda: child(["--hyrax"], 240)), (lambda: child(["--open"], 420))]
    steps += [(lambda lg=lg: kernel_stats(lg, 180)) for lg in LOGNS]
    if parent:
        for tool, args, limit in (("time_hyrax_eval.py", ["9"], 240), ("time_spartan_open.py", ["7"], 500)):
            steps.append(lambda tool=tool, args=args, limit=limit: (lambda rc_lines: (rc_lines[0], [f"# the parent commit's tools/{tool} in the same job, on the same MI355X:"] + rc_lines[1]))(
                child(args, limit, cwd=parent, script=os.path.join(parent, "tools", tool))))
    rc = 0
    for step in steps:                                   # chained: a step that fails or runs out of time ends the run
        rc, text = step()
        lines += text + [""]
        open(out_path, "w").write("\n".join(lines))
        if rc != 0:
            break
    print("\n".join(lines))
    return rc


if __name__ == "__main__":
    sys.exit(main() or 0)
