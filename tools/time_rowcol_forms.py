#!/usr/bin/env python3
"""The row / column sums of the bucket reduction: four waves per sum (k_reduce_rowcol_coop) against several sums per wave
(k_reduce_rowcol<C, LPS>), measured on one MI355X in ONE job.  Writes the lines of profiles/r17_rowcol_forms.txt.

    python tools/time_rowcol_forms.py --parent DIR [--stages bound,ab,lps,pmc,trace,alone] [--out FILE]

DIR is a checkout of the PARENT commit with its libraries built (python __graft_entry__.py there): the old side of every A/B runs
from it, the new side from this tree.  Stages, in the order they decide something:

  bound   the kill criterion, BEFORE any kernel: the parent's experiment build as shipped against REEF_MSM_SKIP_REDUCE=2 (row / column
          sums not run, timing only), alternated three times at the bench's plan, three MSMs in flight
  ab      the headline: bench.py --steps 20 --warmup 5 --no-cpu-baseline, parent's release build and this tree's alternated, three lines
          each; the first pair also dumps its results (canonical affine) and compares them byte for byte
  lps     this tree's experiment build with REEF_MSM_ROWCOL = 0 (four waves) / 64 / 32 / 16 forced, alternated three times
  pmc     SQ_INSTS_VALU per launch of the reduction kernels (a rocprofv3 --pmc run of its own per form, no tracing domain beside it)
  trace   durations of the reduction kernels from one rocprofv3 --kernel-trace --stats run of the timed region per build, and of a run with
          one MSM at a time in its timed region (its host-scalar legs still call from six threads)
  alone   tools/sweep_plans.py 15 16 17 18 20 on both release builds, alternated twice: the latency of one MSM on an otherwise idle device;
          then one 2^20-point MSM at a time with each form forced (experiment build): what a form costs a caller who waits

Every GPU step is a process of its own under `timeout`; the first step that fails ends the job.
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDUCE = ("k_reduce_rowcol", "k_reduce_weighted", "k_reduce_combine")


def emit(line, fh):
    print(line, flush=True)
    fh.write(line + "\n")
    fh.flush()


def step(cmd, env=None, limit=300, cwd=None):
    """One GPU step: its own process, its own time limit; anything but success ends the job."""
    e = dict(os.environ)
    e.update(env or {})
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, env=e, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(f"step failed with {p.returncode}: {' '.join(cmd)}\n{p.stderr[-2000:]}")
    return p.stdout


def bench(root, args, env=None, limit=300):
    out = step([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"] + args, env=env, limit=limit, cwd=root)
    return json.loads(out.strip().splitlines()[-1])


def exp_lib(root):
    return os.path.join(root, "reef_amd", "_lib", "libreef_msm_exp.so")


def spread(v):
    return max(v) - min(v)


def stage_bound(a, fh):
    emit("# upper bound (kill criterion), parent's experiment build: bench.py --allow-experiment --steps 4 --warmup 2 --msms-per-step 48 --no-cpu-baseline --no-replay, "
         "shipped against REEF_MSM_SKIP_REDUCE=2 (row / column sums NOT RUN, results garbage: --no-check), alternated; ms per MSM, three in flight", fh)
    args = ["--allow-experiment", "--steps", "4", "--warmup", "2", "--msms-per-step", "48", "--no-cpu-baseline", "--no-replay"]
    got = {"shipped": [], "free": []}
    for _ in range(3):
        for label, skip in (("shipped", "0"), ("free", "2")):
            d = bench(a.parent, args + (["--no-check"] if skip != "0" else []), env={"REEF_MSM_LIB": exp_lib(a.parent), "REEF_MSM_SKIP_REDUCE": skip})
            got[label].append(d["config"]["ms_per_msm"])
            emit(f"{'shipped' if skip == '0' else 'row/column sums free':22s} c={d['config']['window_bits']} tables={d['config']['tables']}  {d['config']['ms_per_msm']:.4f} ms/MSM in flight   {d['config']['check']}", fh)
    s, f = got["shipped"], got["free"]
    noise = max(spread(s), spread(f))
    wins = all(x - y > noise for x, y in zip(s, f))
    emit(f"bound: shipped {min(s):.4f}-{max(s):.4f} (spread {spread(s):.4f}), free {min(f):.4f}-{max(f):.4f} (spread {spread(f):.4f}); "
         f"free beats shipped in every pairing by more than either spread: {wins}"
         f"{'' if wins else ' -- NOTHING TO WIN, no kernel'}; at most {100 * (sum(s) / sum(f) - 1):.1f} % for a row / column kernel that costs nothing", fh)
    return wins


def headline(d):
    c = d["config"]
    return f"value {d['value']:.4g}  ms_per_msm {c['ms_per_msm']:.4f}  plain_key {(c.get('plain_key') or {}).get('pairs_per_s', float('nan')):.4g}"


def stage_ab(a, fh):
    emit("# headline: bench.py --gpus 1 --steps 20 --warmup 5 --no-cpu-baseline, parent's release build (old) and this tree's (new) alternated three times: value (pairs/s), ms_per_msm, plain key pairs/s", fh)
    args = ["--steps", "20", "--warmup", "5", "--no-cpu-baseline"]
    vals = {"old": [], "new": []}
    dumps = {}
    tmp = tempfile.mkdtemp(prefix="rowcol_ab_")
    for i in range(3):
        for label, root in (("old", a.parent), ("new", ROOT)):
            extra = []
            if i == 0:
                dumps[label] = os.path.join(tmp, label)
                extra = ["--dump-outputs", dumps[label]]
            d = bench(root, args + extra, limit=420)
            vals[label].append(d["value"])
            emit(f"{label}  {headline(d)}  library {d['config'].get('library', '?')}", fh)
    o, n = vals["old"], vals["new"]
    emit(f"ab: old {min(o):.4g}-{max(o):.4g} (spread {100 * spread(o) / min(o):.2f} %), new {min(n):.4g}-{max(n):.4g} (spread {100 * spread(n) / min(n):.2f} %); "
         f"every new line above every old line: {min(n) > max(o)}; medians {100 * (sorted(n)[1] / sorted(o)[1] - 1):+.2f} %", fh)
    import numpy as np
    ra, rb = (np.load(os.path.join(dumps[k], "msm_results.npy")) for k in ("old", "new"))
    emit(f"# bench.py --dump-outputs, first pair of runs: msm_results.npy (canonical affine) byte-identical between old and new:\nmsm_results identical: {ra.shape} {bool(ra.shape == rb.shape and ra.tobytes() == rb.tobytes())}", fh)
    shutil.rmtree(tmp, ignore_errors=True)


FORMS = (("four waves per sum", "0"), ("64 lanes per sum", "64"), ("32 lanes per sum", "32"), ("16 lanes per sum", "16"))


def stage_lps(a, fh):
    emit("# each form forced (this tree's experiment build, REEF_MSM_ROWCOL): bench.py --allow-experiment --steps 8 --warmup 3 --no-cpu-baseline --no-replay, alternated three times", fh)
    args = ["--allow-experiment", "--steps", "8", "--warmup", "3", "--no-cpu-baseline", "--no-replay"]
    vals = defaultdict(list)
    for _ in range(3):
        for label, v in FORMS:
            d = bench(ROOT, args, env={"REEF_MSM_LIB": exp_lib(ROOT), "REEF_MSM_ROWCOL": v})
            vals[label].append(d["value"])
            emit(f"{label:20s} value {d['value']:.4g}  ms_per_msm {d['config']['ms_per_msm']:.4f}", fh)
    for label, _ in FORMS:
        v = vals[label]
        emit(f"lps: {label:20s} {min(v):.4g}-{max(v):.4g}  median {sorted(v)[1]:.4g}", fh)


def rocprof(root, mode, env, bench_args, limit=420):
    """bench.py under rocprofv3; -> the rows of the CSV the mode writes"""
    d = tempfile.mkdtemp(prefix="rowcol_prof_")
    flags = ["--pmc", "SQ_INSTS_VALU", "SQ_WAVES"] if mode == "pmc" else ["--kernel-trace", "--stats"]
    step(["rocprofv3"] + flags + ["--output-format", "csv", "-d", d, "--", sys.executable, os.path.join(root, "bench.py"), "--gpus", "1"] + bench_args,
         env=env, limit=limit, cwd=d)
    pat = "*counter_collection.csv" if mode == "pmc" else "*kernel_stats.csv"
    files = glob.glob(os.path.join(d, "**", pat), recursive=True)
    if not files:
        sys.exit(f"rocprofv3 wrote no {pat}")
    rows = list(csv.DictReader(open(files[0])))
    shutil.rmtree(d, ignore_errors=True)
    return rows


def short(name):
    return re.sub(r"^void ", "", name).replace("reef::", "").split("(")[0]


ONE_MSM = ["--steps", "4", "--warmup", "1", "--msms-per-step", "1", "--streams", "1", "--no-cpu-baseline", "--no-replay", "--no-check"]


def stage_pmc(a, fh):
    emit("# SQ_INSTS_VALU per launch of the reduction kernels: bench.py --steps 4 --warmup 1 --msms-per-step 1 --streams 1 --no-cpu-baseline --no-replay --no-check under "
         "rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES, a run of its own per line (this tree: experiment build, the form forced -- one MSM at a time takes the four-wave form by itself)", fh)
    runs = [("old (parent, release)", a.parent, {}, [])] + \
           [(f"new, {label}", ROOT, {"REEF_MSM_LIB": exp_lib(ROOT), "REEF_MSM_ROWCOL": v}, ["--allow-experiment"]) for label, v in FORMS]
    for label, root, env, extra in runs:
        per = defaultdict(lambda: defaultdict(float))
        for r in rocprof(root, "pmc", env, ONE_MSM + extra):
            if r["Counter_Name"] == "SQ_INSTS_VALU":
                per[short(r["Kernel_Name"])][r["Dispatch_Id"]] += float(r["Counter_Value"])
        parts = [f"{k} {sum(v.values()) / len(v):.4g} ({len(v)} launches)" for k, v in sorted(per.items()) if k.startswith(REDUCE)]
        emit(f"{label:28s} " + "   ".join(parts), fh)


def stage_trace(a, fh):
    emit("# durations of the reduction kernels, three MSMs in flight: bench.py --steps 2 --warmup 1 --msms-per-step 48 --no-cpu-baseline --no-replay under rocprofv3 --kernel-trace --stats, one run per build", fh)
    timed = ["--steps", "2", "--warmup", "1", "--msms-per-step", "48", "--no-cpu-baseline", "--no-replay"]
    for label, root in (("old", a.parent), ("new", ROOT)):
        for r in rocprof(root, "trace", {}, timed):
            if short(r["Name"]).startswith(REDUCE):
                emit(f"{label}  {short(r['Name']):32s} calls {r['Calls']:>5s}  average {float(r['AverageNs']) / 1e3:8.1f} us", fh)
    emit("# the kernels ONE MSM at a time launches (--msms-per-step 1 --streams 1, release builds): the reduction kernels' names and durations", fh)
    for label, root in (("old", a.parent), ("new", ROOT)):
        for r in rocprof(root, "trace", {}, ONE_MSM):
            if short(r["Name"]).startswith(REDUCE):
                emit(f"{label}  {short(r['Name']):32s} calls {r['Calls']:>5s}  average {float(r['AverageNs']) / 1e3:8.1f} us", fh)


def stage_alone(a, fh):
    emit("# one MSM on an idle device: tools/sweep_plans.py 15 16 17 18 20 (stream time per MSM, best plan per key size), release builds, alternated twice", fh)
    for _ in range(2):
        for label, root in (("old", a.parent), ("new", ROOT)):
            out = step([sys.executable, os.path.join(root, "tools", "sweep_plans.py"), "15", "16", "17", "18", "20"], limit=420, cwd=root)
            for line in out.splitlines():
                if line.startswith("## "):
                    emit(f"{label}  {line[3:]}", fh)
    emit("# for the record, what each form costs a caller who waits: bench.py --allow-experiment --steps 8 --warmup 2 --msms-per-step 1 --streams 1 --no-cpu-baseline --no-replay "
         "(one 2^20-point MSM at a time, ms per MSM), this tree's experiment build with the form forced, twice", fh)
    for _ in range(2):
        for label, v in FORMS:
            d = bench(ROOT, ["--allow-experiment", "--steps", "8", "--warmup", "2", "--msms-per-step", "1", "--streams", "1", "--no-cpu-baseline", "--no-replay"],
                      env={"REEF_MSM_LIB": exp_lib(ROOT), "REEF_MSM_ROWCOL": v})
            emit(f"{label:20s} one MSM at a time {d['config']['ms_per_msm']:.4f} ms", fh)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--parent", required=True, help="a checkout of the parent commit with its libraries built")
    p.add_argument("--stages", default="bound,ab,lps,pmc,trace,alone")
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17_rowcol_forms.txt"))
    a = p.parse_args()
    a.parent = os.path.abspath(a.parent)
    stages = a.stages.split(",")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as fh:
        for s in stages:
            fn = {"bound": stage_bound, "ab": stage_ab, "lps": stage_lps, "pmc": stage_pmc, "trace": stage_trace, "alone": stage_alone}[s]
            if fn(a, fh) is False:
                break                                    # the bound says there is nothing to win: the job ends with its verdict


if __name__ == "__main__":
    main()
