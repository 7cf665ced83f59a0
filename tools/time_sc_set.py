#!/usr/bin/env python3
"""Time the set-up of the sum-check table (row N2), from the host: reef_sc_set_table on the table written out as 32-byte integers against
reef_sc_set_table_parts on what the table is made of.

    python tools/time_sc_set.py PARENT_LIB [OUT]     the whole comparison; OUT defaults to profiles/r12_sc_set_parts_timing.txt
    python tools/time_sc_set.py --one LIB ROUTE SHAPE MEM [SUB]     one measurement in this process, one JSON line (what the first form
                                                                      starts, also under rocprofv3 --kernel-trace for the kernel times)

PARENT_LIB is a release build of the commit before reef_sc_set_table_parts (the old call as it was: tools/ab_libs.sh keeps such builds under
reef_amd/_lib/variants/); the new call runs on the tree's build.  ROUTE: old | new.  SHAPE: cfg3 ("nldoc": 2^21 one-byte symbols) |
cfg4 ("nlhybrid": 2^26 entries -- 2^12 field elements, calc_fill up to 2^25, 2^25 one-byte DNA symbols).  MEM: pageable | pinned.
SUB (experiment build only): REEF_SC_SET_SUB, the most 128-entry tiles a wave of k_sc_set_parts takes.
Every figure is call entry to return (the call waits for its stream), five runs after one that allocates; before a time is printed the
round-one coefficients of a folding step after the call are compared between the routes."""
import csv
import ctypes
import glob
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE_LIB = os.path.join(ROOT, "reef_amd", "_lib", "libreef_msm.so")
EXP_LIB = os.path.join(ROOT, "reef_amd", "_lib", "libreef_msm_exp.so")
HBM_PEAK = 8.0e12                     # the README's HBM figure
RUNS = 5
SHAPES = {"cfg3": 21, "cfg4": 26}
vp, sz = ctypes.c_void_p, ctypes.c_size_t


class Part(ctypes.Structure):        # reef_sc_part
    _fields_ = [("kind", ctypes.c_uint32), ("elem_bytes", ctypes.c_uint32), ("data", vp), ("count", sz), ("loc", ctypes.c_int)]


def bind(path):
    """The few entries this tool calls, bound by hand: the parent build has no reef_sc_set_table_parts, so reef_amd._ffi would refuse it."""
    lib = ctypes.CDLL(path)
    for name, args in (("reef_sc_create", [ctypes.POINTER(vp), ctypes.c_int, sz]), ("reef_sc_set_table", [vp, ctypes.c_int, vp, sz, ctypes.c_int]),
                       ("reef_sc_gen_eq_table", [vp, vp, vp, sz, vp, sz]), ("reef_sc_round_coeffs", [vp, sz, vp]), ("reef_device_count", [])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = ctypes.c_int, args
    lib.reef_sc_destroy.restype, lib.reef_sc_destroy.argtypes = None, [vp]
    lib.reef_last_error.restype = ctypes.c_char_p
    if hasattr(lib, "reef_sc_set_table_parts"):
        lib.reef_sc_set_table_parts.restype, lib.reef_sc_set_table_parts.argtypes = ctypes.c_int, [vp, ctypes.POINTER(Part), sz]
    return lib


def ok(lib, status):
    if status != 0:
        sys.exit("status %d: %s" % (status, lib.reef_last_error().decode(errors="replace")))


class HostMem:
    """Host arrays in pageable (numpy's own) or pinned (hipHostMalloc) memory."""

    def __init__(self, pinned):
        self.hip = ctypes.CDLL("libamdhip64.so") if pinned else None
        self.held = []

    def empty(self, shape, dtype):
        nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if not self.hip or nbytes == 0:
            return np.empty(shape, dtype=dtype)
        p = vp()
        if self.hip.hipHostMalloc(ctypes.byref(p), sz(nbytes), ctypes.c_uint(0)) != 0:
            sys.exit("hipHostMalloc of %d bytes failed" % nbytes)
        self.held.append(p)
        return np.frombuffer((ctypes.c_uint8 * nbytes).from_address(p.value), dtype=dtype).reshape(shape)

    def free(self):
        for p in self.held:
            self.hip.hipHostFree(p)
        self.held = []


def shape_inputs(shape):
    """-> (ell, public table as (k, 4) uint64, fill as (4,) uint64, its repetitions, symbols as uint8): seeded, the same in every process."""
    ell = SHAPES[shape]
    n = 1 << ell
    rng = np.random.default_rng(0x5C00 + ell)
    if shape == "cfg3":
        return ell, np.zeros((0, 4), dtype=np.uint64), np.zeros(4, dtype=np.uint64), 0, rng.integers(0, 128, size=n, dtype=np.uint8)
    table = rng.integers(0, 1 << 62, size=(1 << 12, 4), dtype=np.uint64)                 # below 2^254: canonical
    fill = rng.integers(0, 1 << 62, size=4, dtype=np.uint64)
    return ell, table, fill, n // 2 - len(table), rng.integers(0, 4, size=n // 2, dtype=np.uint8)


def one(lib_path, route, shape, mem, sub=None):
    if sub:
        os.environ["REEF_SC_SET_SUB"] = str(sub)
    lib = bind(lib_path)
    if lib.reef_device_count() <= 0:
        sys.exit("no HIP device: nothing is measured without one")
    ell, table, fill, nfill, syms = shape_inputs(shape)
    n = 1 << ell
    host = HostMem(mem == "pinned")
    res = {"lib": os.path.relpath(lib_path, ROOT), "route": route, "shape": shape, "ell": ell, "mem": mem, "sub": sub}
    h = vp()
    ok(lib, lib.reef_sc_create(ctypes.byref(h), 0, n))
    if route == "old":
        t0 = time.perf_counter()                                   # what a caller of the old call pays first: the table as 32-byte integers
        whole = host.empty((n, 4), np.uint64)
        whole[:len(table)] = table
        whole[len(table):len(table) + nfill] = fill
        at = len(table) + nfill
        whole[at:at + len(syms), 1:] = 0
        whole[at:at + len(syms), 0] = syms
        whole[at + len(syms):] = 0
        res["widen_host_ms"] = (time.perf_counter() - t0) * 1e3
        res["bytes_to_device"] = whole.nbytes

        def call():
            ok(lib, lib.reef_sc_set_table(h, 0, whole.ctypes.data, n, 0))
    else:
        tab, sy = host.empty(table.shape, np.uint64), host.empty(syms.shape, np.uint8)
        tab[...] = table
        sy[...] = syms
        fl = np.ascontiguousarray(fill)
        parts = (Part * 3)(Part(0, 0, tab.ctypes.data if len(tab) else None, len(tab), 0), Part(2, 0, fl.ctypes.data, nfill, 0),
                           Part(1, 1, sy.ctypes.data, len(sy), 0))
        res["bytes_to_device"] = tab.nbytes + sy.nbytes + (64 if nfill else 0)

        def call():
            ok(lib, lib.reef_sc_set_table_parts(h, parts, 3))
    t0 = time.perf_counter()
    call()
    res["first_call_ms"] = (time.perf_counter() - t0) * 1e3        # allocates the staging buffer and the structure's buffers
    times = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    res["call_ms"] = times
    # a folding step's first round on the table just set: the routes must agree on it
    rng = np.random.default_rng(99)
    nq = 33
    rs = rng.integers(0, 1 << 62, size=(nq + 1, 4), dtype=np.uint64)
    qs = rng.integers(0, n, size=nq + 1, dtype=np.uint32)
    last_q = rng.integers(0, 1 << 62, size=(ell, 4), dtype=np.uint64)
    out = np.zeros((3, 4), dtype=np.uint64)
    ok(lib, lib.reef_sc_gen_eq_table(h, rs.ctypes.data, qs.ctypes.data, nq, last_q.ctypes.data, ell))
    ok(lib, lib.reef_sc_round_coeffs(h, n // 2, out.ctypes.data))
    res["round_one"] = out.tobytes().hex()
    lib.reef_sc_destroy(h)
    host.free()
    print(json.dumps(res), flush=True)


def child(args, env=None):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"] + [str(a) for a in args], capture_output=True, text=True,
                       env=dict(os.environ, **(env or {})), timeout=600)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode != 0 or not lines:
        sys.exit("measurement %s failed (exit %d): %s" % (args, p.returncode, (p.stderr or p.stdout)[-600:]))
    print("measured", *args, file=sys.stderr, flush=True)
    return json.loads(lines[-1])


def kernel_times(args, tmp):
    """Per-kernel durations (us) of one --one run under rocprofv3 --kernel-trace --stats, a run of its own: {kernel name: [durations]}."""
    shutil.rmtree(tmp, ignore_errors=True)
    p = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--one"] +
                       [str(a) for a in args], capture_output=True, text=True, timeout=900)
    traces = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
    if p.returncode != 0 or not traces:
        sys.exit("rocprofv3 run %s failed (exit %d): %s" % (args, p.returncode, p.stderr[-600:]))
    out = {}
    with open(traces[0]) as f:
        for row in csv.DictReader(f):
            out.setdefault(row["Kernel_Name"], []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    print("traced", *args, file=sys.stderr, flush=True)
    return out


def med_min(xs):
    return "median %.3f min %.3f" % (float(np.median(xs)), min(xs))


def main(parent_lib, out_path):
    parent_lib = os.path.abspath(parent_lib)
    lines = ["# tools/time_sc_set.py: the sum-check table set from the host, one MI355X.  old = reef_sc_set_table on 32-byte integers, on the parent build",
             "# (%s) and on this build; new = reef_sc_set_table_parts on this build.  Times in ms, call entry to return," % os.path.relpath(parent_lib, ROOT),
             "# %d runs after one that allocates.  The round-one coefficients of a step after each call were compared before a time was printed." % RUNS]
    for shape in ("cfg3", "cfg4"):
        rows = []
        for mem in ("pageable", "pinned"):
            rows += [("old, parent build", child([parent_lib, "old", shape, mem])), ("old, this build", child([TREE_LIB, "old", shape, mem])),
                     ("new, this build", child([TREE_LIB, "new", shape, mem]))]
        if len({r["round_one"] for _, r in rows}) != 1:
            sys.exit("%s: the round-one coefficients differ between the routes: %s" % (shape, [(w, r["round_one"][:16]) for w, r in rows]))
        lines.append("")
        lines.append("## %s: 2^%d entries; round-one coefficients equal on every route" % (shape, SHAPES[shape]))
        for what, r in rows:
            extra = ", widening the symbols on the host first: %.1f ms" % r["widen_host_ms"] if "widen_host_ms" in r else ""
            lines.append("%-18s %-8s %11d bytes to the device   %s   first call %.3f%s" %
                         (what, r["mem"], r["bytes_to_device"], med_min(r["call_ms"]), r["first_call_ms"], extra))
        for mem in ("pageable", "pinned"):
            o = [r for w, r in rows if w == "old, parent build" and r["mem"] == mem][0]
            nw = [r for w, r in rows if w.startswith("new") and r["mem"] == mem][0]
            lines.append("%s: new / old (parent) = %.3f on the medians" % (mem, np.median(nw["call_ms"]) / np.median(o["call_ms"])))
    # entries per lane: the experiment build reads REEF_SC_SET_SUB (2 entries per lane and tile)
    lines += ["", "## 128-entry tiles per wave of k_sc_set_parts (experiment build, REEF_SC_SET_SUB), cfg4, pinned: call ms, and the kernel alone below"]
    for sub in (1, 2, 4, 8, 16):
        r = child([EXP_LIB, "new", "cfg4", "pinned", sub])
        lines.append("sub %d (%2d entries per lane): %s" % (sub, 2 * sub, med_min(r["call_ms"])))
    # kernel times: a rocprofv3 run of its own per route
    lines += ["", "## kernel time, us, from rocprofv3 --kernel-trace (every dispatch of the run: %d timed calls and the first)" % RUNS]
    tmp = os.path.join(os.environ.get("TMPDIR", "/tmp"), "time_sc_set_trace")
    for shape in ("cfg3", "cfg4"):
        n = 1 << SHAPES[shape]
        old = kernel_times([parent_lib, "old", shape, "pinned"], tmp)
        new = kernel_times([TREE_LIB, "new", shape, "pinned"], tmp)
        pick = lambda d, key: [v for k, v in d.items() if key in k]
        imp, cls, fills = pick(old, "k_fe_import"), pick(old, "k_sc_classify"), pick(old, "fillBuffer")
        sp = pick(new, "k_sc_set_parts")
        if not imp or not sp:
            sys.exit("%s: kernels missing from the trace: %s / %s" % (shape, sorted(old), sorted(new)))
        imp, cls, sp = imp[0], cls[0] if cls else [0.0], sp[0]       # a table below the rank-one gate (cfg3) has no row structure: nothing is classified
        lines.append("%s old: k_fe_import %s (%d)   k_sc_classify %s (%d)   sum of the medians %.3f; runtime fill kernels (the accumulators' and, if any, the tail's memset): %s" %
                     (shape, med_min(imp), len(imp), med_min(cls), len(cls), np.median(imp) + np.median(cls),
                      "; ".join("%d x median %.3f" % (len(v), np.median(v)) for v in fills) or "none traced"))
        lines.append("%s new: k_sc_set_parts %s max %.3f (%d)   = %.3f of the old sum" % (shape, med_min(sp), max(sp), len(sp), np.median(sp) / (np.median(imp) + np.median(cls))))
        wrote = n * (36 if cls[0] else 32)                               # no 4-byte copy without the row structure
        lines.append("%s new: %d bytes written (32 per entry to T0, 4 to the 4-byte copy where there is one) in the median time: %.0f GB/s = %.3f of the HBM peak of %.0f GB/s" %
                     (shape, wrote, wrote / (np.median(sp) * 1e-6) / 1e9, wrote / (np.median(sp) * 1e-6) / HBM_PEAK, HBM_PEAK / 1e9))
        if shape == "cfg4":
            for sub in (1, 2, 4, 8, 16):
                k = pick(kernel_times([EXP_LIB, "new", shape, "pinned", sub], tmp), "k_sc_set_parts")[0]
                lines.append("cfg4 new, experiment build, sub %d: k_sc_set_parts %s" % (sub, med_min(k)))
    shutil.rmtree(tmp, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    if len(sys.argv) >= 6 and sys.argv[1] == "--one":
        one(sys.argv[2], sys.argv[3], sys.argv[4], sys.argv[5], int(sys.argv[6]) if len(sys.argv) > 6 else None)
    elif len(sys.argv) >= 2 and not sys.argv[1].startswith("-"):
        main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r12_sc_set_parts_timing.txt"))
    else:
        sys.exit(__doc__)
