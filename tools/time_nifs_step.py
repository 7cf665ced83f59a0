"""A step's two commitments on a resident NIFS ctx, host to host: the parent's two calls against reef_nifs_commit_step.

    python tools/time_nifs_step.py [reps] [--quick] [--no-prove] [--no-kernels] [--out PATH]     (writes profiles/r16_nifs_step_timing.txt)
    python tools/time_nifs_step.py --one                                                         (what the rocprofv3 pass runs)

Form A: reef_msm of a host W2 (comm_W), then reef_nifs_commit_T of the same host W2 (comm_T): two uploads, two waits.
Form B: reef_nifs_commit_step: one upload, one pass over z2, the two rows committed together, one wait.
Per curve the replay's shapes (tests/golden/replay_shapes.json; num_vars = num_cons): the primary of cfg3 / cfg4 / cfg5 on Pallas, the
secondary (11 376) on Vesta, and the same lengths on the other curve except cfg5's.  Key kinds: pre (pre-shifted tables, the bucket
pipeline), plain (no precompute) and tables (byte tables; keys of at most 2^16 points).  A and B alternate in one process after a warm-up;
median, minimum and maximum of `reps` calls each.  Beside them, on the same key and scalars already on the device: one reef_msm_rows of
the two rows (max_scalar_bits = 255) against two reef_msm of one row each -- what decides the route commit_step takes for a key kind.
The matrices are SYNTHETIC (tools/_synthetic.py).  Kernel times of the new kernels come from one rocprofv3 --kernel-trace --stats pass
of its own over `--one`; the prove leg's ms_per_step with and without `paired` from this process."""
import csv
import glob
import os
import shutil
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import pasta_ref as R                     # noqa: E402
from reef_amd.msm import DeviceBuffer, MsmContext      # noqa: E402
from reef_amd.nifs import Nifs                         # noqa: E402
from _synthetic import synthetic_matrix                # noqa: E402

SHAPES = [(0, "cfg3 primary", 27790), (0, "secondary length", 11376), (0, "cfg4 primary", 39484), (0, "cfg5 primary", 1032421),
          (1, "cfg3 length", 27790), (1, "secondary", 11376), (1, "cfg4 length", 39484)]
KINDS = {"pre": dict(bucket_groups=1, byte_tables=2), "plain": dict(bucket_groups=4), "tables": dict(bucket_groups=1, byte_tables=1)}
NEW_KERNELS = ("k_nifs_import_step", "k_nifs_export_running", "k_nifs_rows_short", "k_nifs_rows_long", "k_nifs_rows_finish", "k_fe_import")


def ms(fn):
    t = time.perf_counter()
    fn()
    return (time.perf_counter() - t) * 1e3


def mmm(xs):
    return "median %7.3f  min %7.3f  max %7.3f" % (statistics.median(xs), min(xs), max(xs))


def make_ctx(curve, n, rng):
    nio = 2
    nf = Nifs(curve, n, n, nio)
    long_rows = rng.choice(n, size=4, replace=False)
    for k in range(3):
        r, c, v, _ = synthetic_matrix(rng, n, n + 1 + nio, long_rows)
        nf.set_matrix(k, r, c, v)
    w = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
    x = rng.integers(0, 1 << 62, size=(nio, 4), dtype=np.uint64)
    nf.set_running(w, None, np.array([[1, 0, 0, 0]], dtype=np.uint64), x)
    return nf, rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64), x


def measure_shape(curve, what, n, kinds, reps, lines):
    rng = np.random.default_rng(n + curve)
    nf, w2, x2 = make_ctx(curve, n, rng)
    bases = R.gen_bases_ap(curve, 42, 5, n)
    rows_host = np.ascontiguousarray(np.vstack([w2, rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)]))
    d_rows = DeviceBuffer.from_host(rows_host)
    d_row1 = DeviceBuffer.from_host(rows_host[n:])
    lines.append("")
    lines.append("## %s, %s: num_cons = num_vars = %d, W2 = %.2f MB" % (("pallas", "vesta")[curve], what, n, 32 * n / 1e6))
    with nf:
        for kind in kinds:
            if kind == "tables" and n > (1 << 16):
                lines.append("%-6s  no byte tables for a key of %d points" % (kind, n))
                continue
            with MsmContext(curve, bases, **KINDS[kind]) as key:
                assert key.has_byte_tables() == (kind == "tables")

                def form_a():
                    cw = key.msm(w2, is_mont=False)
                    return cw, nf.commit_t(key, w2, x2)

                def form_b():
                    return nf.commit_step(key, w2, x2)
                (aw, at), (bw, bt) = form_a(), form_b()                     # warm: the long-row list, the key's workspaces, both routes
                if not (np.array_equal(aw, bw) and np.array_equal(at, bt)):
                    aw, at, bw, bt = (R.compress(curve, p) for p in (aw, at, bw, bt))
                    if (aw, at) != (bw, bt):
                        sys.exit("%s %s: the two forms give different points" % (what, kind))
                for _ in range(3):
                    form_a()
                    form_b()
                ta, tb, tw, tt = [], [], [], []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    key.msm(w2, is_mont=False)
                    t1 = time.perf_counter()
                    nf.commit_t(key, w2, x2)
                    t2 = time.perf_counter()
                    tw.append((t1 - t0) * 1e3)
                    tt.append((t2 - t1) * 1e3)
                    ta.append((t2 - t0) * 1e3)
                    tb.append(ms(form_b))
                # the rows alone, scalars on the device: one batch of two rows against two single rows
                out2 = np.zeros((2, 12), dtype=np.uint64)
                pair = lambda: key.msm_rows(d_rows, 2, n, is_mont=False, max_scalar_bits=255, out=out2)     # noqa: E731
                single = lambda: (key.msm(d_rows, is_mont=False, n=n), key.msm(d_row1, is_mont=False, n=n))     # noqa: E731
                for _ in range(3):
                    pair()
                    single()
                tp, ts = [], []
                for _ in range(reps):
                    tp.append(ms(pair))
                    ts.append(ms(single))
                a, b = statistics.median(ta), statistics.median(tb)
                spread = max(ta) - min(ta)
                lines.append("%-6s  A  reef_msm + commit_T   %s   (reef_msm %s | commit_T %s)" % (kind, mmm(ta), mmm(tw), mmm(tt)))
                lines.append("%-6s  B  commit_step           %s   B - A on the medians %+.3f ms (B / A = %.3f); spread of A (max - min) %.3f ms: %s" %
                             (kind, mmm(tb), b - a, b / a, spread, "within the rule" if b - a <= spread else "B IS SLOWER THAN THE RULE ALLOWS"))
                lines.append("%-6s  rows alone, device scalars: one batch of two rows %s | two single rows %s -> %s" %
                             (kind, mmm(tp), mmm(ts), "the batch" if statistics.median(tp) < statistics.median(ts) else "single rows"))
    d_rows.free()
    d_row1.free()


def one():
    """The rocprofv3 pass: cfg3's shapes on a pre-shifted key, five calls of each form, commit_running and check_fresh."""
    for curve, n in ((0, 27790), (1, 11376)):
        rng = np.random.default_rng(n)
        nf, w2, x2 = make_ctx(curve, n, rng)
        with nf, MsmContext(curve, R.gen_bases_ap(curve, 42, 5, n), **KINDS["pre"]) as key:
            for _ in range(5):
                key.msm(w2, is_mont=False)
                nf.commit_t(key, w2, x2)
                nf.fold(7)
                nf.commit_step(key, w2, x2)
                nf.check_fresh()
                nf.fold(7)
                nf.commit_running(key)


def kernel_lines(tmp):
    shutil.rmtree(tmp, ignore_errors=True)
    p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--one"],
                       capture_output=True, text=True, timeout=600)
    traces = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
    if p.returncode != 0 or not traces:
        return ["rocprofv3 pass failed (exit %d): %s" % (p.returncode, p.stderr[-400:].replace("\n", " | "))]
    by = {}
    with open(traces[0]) as f:
        for row in csv.DictReader(f):
            by.setdefault(row["Kernel_Name"], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    out = []
    for name in sorted(by):
        if any(k in name for k in NEW_KERNELS):
            v = by[name]
            out.append("%-110s calls %4d  us: %s" % (name[:110], len(v), mmm(v)))
    return out


def prove_lines(cfgs):
    from reef_amd import replay
    out = []
    for cfg in cfgs:
        replay.run_prove(cfg)                                               # warm
        d, p = replay.run_prove(cfg), replay.run_prove(cfg, paired=True)
        d2, p2 = replay.run_prove(cfg), replay.run_prove(cfg, paired=True)
        assert p["paired"] is True and p["proof_checked"] and "paired" not in d
        out.append("%s  ms_per_step: default %.3f, %.3f (commit_w %.3f + nifs %.3f)   paired %.3f, %.3f (nifs %.3f)   steps %d" %
                   (cfg, d["ms_per_step"], d2["ms_per_step"], d2["commit_w_ms_per_step"], d2["nifs_ms_per_step"], p["ms_per_step"], p2["ms_per_step"],
                    p2["nifs_ms_per_step"], d["steps"]))
    return out


def main():
    args = sys.argv[1:]
    if "--one" in args:
        return one()
    reps = next((int(a) for a in args if a.isdigit()), 20)
    quick = "--quick" in args
    out_path = args[args.index("--out") + 1] if "--out" in args else os.path.join(ROOT, "profiles", "r16_nifs_step_timing.txt")
    from reef_amd import _ffi
    lines = ["# tools/time_nifs_step.py on one MI355X, library sources %s: a step's comm_W and comm_T on a resident NIFS ctx, host to host, ms." % _ffi.library_sources_sha16(),
             "# A = reef_msm(host W2) then reef_nifs_commit_T(host W2) (the parent's two calls); B = reef_nifs_commit_step.  Alternating in one process after a",
             "# warm-up, %d calls each; SYNTHETIC matrices (2-4 entries per row and matrix, four rows of 10^4 entries), full-width scalars." % reps,
             "# Rule: B - A on the medians must not exceed the spread (max - min) the file shows for A."]
    for curve, what, n in (SHAPES[:2] + SHAPES[5:6] if quick else SHAPES):
        measure_shape(curve, what, n, ("pre", "plain") if n > (1 << 16) else ("pre", "plain", "tables"), reps, lines)
        print("\n".join(lines[-12:]), file=sys.stderr, flush=True)
    if "--no-prove" not in args:
        lines += ["", "## the prove leg (reef_amd.replay.run_prove), both curves together, from this process: two runs each after a warm one"]
        lines += prove_lines(("cfg3",) if quick else ("cfg3", "cfg4", "cfg5"))
    if "--no-kernels" not in args:
        lines += ["", "## kernel time from one rocprofv3 --kernel-trace --stats pass of its own over `--one` (cfg3's two shapes, pre-shifted keys, five steps of each form)"]
        lines += kernel_lines(os.path.join(os.environ.get("TMPDIR", "/tmp"), "time_nifs_step_trace"))
    text = "\n".join(lines) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
