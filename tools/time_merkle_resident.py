#!/usr/bin/env python3
"""Time the resident Poseidon Merkle tree (reef_merkle_create / _open / _check_paths) against the route it replaces, from the host.

    python tools/time_merkle_resident.py PARENT_LIB [OUT] [LOGS]    the whole comparison; OUT defaults to profiles/r13_merkle_resident_timing.txt,
                                                                    LOGS to 20,24,27 (document lengths 2^LOG; a size that fails ends the run there)
    python tools/time_merkle_resident.py --step NAME LOG PARENT_LIB  one step in this process, JSON lines (what the first form starts, each
                                                                    under its own `timeout`; NAME: create | open | check | kernels)

PARENT_LIB is a release build of the commit before reef_merkle_create: its reef_merkle_commit is the comparison (root only for `create`, the
whole tree to the host plus MerkleCommitment.make_wits for `open`).  Every figure is call entry to return -- each call waits for its stream
-- over five runs after one warm call: median, minimum, maximum.  Device bytes are differences of hipMemGetInfo's free figure around the
calls (what stays allocated afterwards: the ctx's buffers, or the stateless call's grow-only scratch buffers); host bytes are the arrays the
route leaves the caller holding.  Before a time is printed the two routes' roots and openings are compared."""
import csv
import ctypes
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
RUNS = 5
STEP_LIMIT = {20: 120, 24: 240, 27: 600}      # seconds a step may take, by size
vp, sz = ctypes.c_void_p, ctypes.c_size_t


def bind_parent(path):
    """reef_merkle_commit of another build, bound by hand (reef_amd._ffi refuses a build without the new symbols)."""
    lib = ctypes.CDLL(path)
    lib.reef_merkle_commit.restype, lib.reef_merkle_commit.argtypes = ctypes.c_int, [ctypes.c_int, vp, vp, sz, ctypes.c_int, ctypes.c_bool, vp, ctypes.c_int, vp]
    lib.reef_last_error.restype = ctypes.c_char_p
    lib.reef_version.restype = ctypes.c_char_p
    return lib


def free_bytes():
    hip = ctypes.CDLL("libamdhip64.so")
    free, total = sz(0), sz(0)
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def timed(fn, runs=RUNS):
    fn()                                       # the warm call: allocations, the sparse constants
    out = []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t) * 1e3)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out)}


def setup(log):
    from oracle import merkle_oracle as M
    from reef_amd import merkle
    from reef_amd.sumcheck import ints_to_array
    p = M.standin_params()
    rc, mds = ints_to_array(p.rc), ints_to_array([x for row in p.mds for x in row])
    lim = lambda v: (ctypes.c_uint64 * 4)(*[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)])   # noqa: E731
    pp = merkle.PoseidonParams(p.t, p.rf, p.rp, 0, rc.ctypes.data, mds.ctypes.data, lim(p.tag_leaf), lim(p.tag_node))
    doc = np.random.default_rng(log).integers(0, 131, size=1 << log, dtype=np.uint32)
    return p, pp, (rc, mds), doc


def say(**kw):
    print(json.dumps(kw), flush=True)


def step_create(log, parent_path):
    from reef_amd import _ffi
    p, pp, keep, doc = setup(log)
    n = doc.shape[0]
    lib, par = _ffi.load(), bind_parent(parent_path)
    root_new, root_par = np.zeros((1, 4), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64)
    h = vp()

    def create():
        _ffi.check(lib.reef_merkle_create(ctypes.byref(h), 0, ctypes.byref(pp), doc.ctypes.data, n, 0, False, 0))

    def destroy():
        lib.reef_merkle_destroy(h)
    times = []
    create(); destroy()
    for _ in range(RUNS):
        t = time.perf_counter()
        create()
        times.append((time.perf_counter() - t) * 1e3)
        _ffi.check(lib.reef_merkle_info(h, None, None, None, root_new.ctypes.data))
        destroy()
    say(step="create", log=log, route="new: reef_merkle_create (destroyed outside the timing)", median_ms=statistics.median(times), min_ms=min(times), max_ms=max(times))

    def commit():
        st = par.reef_merkle_commit(0, ctypes.byref(pp), doc.ctypes.data, n, 0, False, None, 0, root_par.ctypes.data)
        assert st == 0, par.reef_last_error()
    say(step="create", log=log, route="parent: reef_merkle_commit, tree_out = NULL", **timed(commit))
    assert (root_new == root_par).all(), "the two builds disagree on the root"
    # where a difference goes: the ctx allocates its document and tree anew in every create; the stateless call keeps its scratch buffers
    hip = ctypes.CDLL("libamdhip64.so")
    nodes = lib.reef_merkle_nodes(n)

    def alloc():
        a, b = vp(), vp()
        assert hip.hipMalloc(ctypes.byref(a), sz(n * 4)) == 0 and hip.hipMalloc(ctypes.byref(b), sz(nodes * 32)) == 0
        hip.hipFree(a); hip.hipFree(b)
    say(step="create", log=log, route="hipMalloc + hipFree of the ctx's two large buffers alone (%d + %d bytes)" % (n * 4, nodes * 32), **timed(alloc))


def step_open(log, parent_path):
    from reef_amd import _ffi, merkle
    p, pp, keep, doc = setup(log)
    n = doc.shape[0]
    lib, par = _ffi.load(), bind_parent(parent_path)
    rng = np.random.default_rng(1000 + log)
    lookups = {k: [int(x) for x in rng.integers(0, n, size=k)] for k in (32, 1024)}
    merkle.ResidentMerkleCommitment.new("pallas", doc[:64], p.t, p.rf, p.rp, p.rc, p.mds, p.tag_leaf, p.tag_node).close()   # the runtime's own first allocations
    free0 = free_bytes()
    t = time.perf_counter()
    rm = merkle.ResidentMerkleCommitment.new("pallas", doc, p.t, p.rf, p.rp, p.rc, p.mds, p.tag_leaf, p.tag_node)
    create_ms = (time.perf_counter() - t) * 1e3
    L = rm.levels
    held_dev = free0 - free_bytes()
    got = {}
    for k, idx in lookups.items():
        arr = np.asarray(idx, dtype=np.uint64)
        oidx, opp = np.zeros(k, dtype=np.uint64), np.zeros((k * L, 4), dtype=np.uint64)

        def op():
            _ffi.check(lib.reef_merkle_open(rm._h, arr.ctypes.data, k, None, oidx.ctypes.data, opp.ctypes.data, None))
        say(step="open", log=log, k=k, route="new: reef_merkle_open, host to host (opposite_idx and opposite)", **timed(op))
        got[k] = rm.make_wits(idx)
    say(step="open", log=log, route="new: bytes held", device_bytes=held_dev, device_bytes_by_design=n * 4 + rm.nodes * 32,
        host_bytes=1024 * L * 32 + 1024 * 12, note="device: free memory before create minus after (document + tree + constants, in the allocator's granules); host: the ctx's "
        "staging vector for k = 1024; create took %.1f ms" % create_ms)
    rm.close()
    nodes = lib.reef_merkle_nodes(n)
    tree = np.empty((nodes, 4), dtype=np.uint64)
    root = np.zeros((1, 4), dtype=np.uint64)
    assert par.reef_merkle_commit(0, ctypes.byref(pp), doc.ctypes.data, 64, 0, False, None, 0, root.ctypes.data) == 0      # the same for the other build
    free1 = free_bytes()

    def commit():
        st = par.reef_merkle_commit(0, ctypes.byref(pp), doc.ctypes.data, n, 0, False, tree.ctypes.data, 0, root.ctypes.data)
        assert st == 0, par.reef_last_error()
    say(step="open", log=log, route="parent: reef_merkle_commit, tree_out on the host", **timed(commit, runs=RUNS if log < 27 else 2))
    held_par = free1 - free_bytes()
    levels, m, off = [], (n + 1) // 2, 0
    while True:
        levels.append(tree[off:off + m])
        off += m
        if m <= 1:
            break
        m = (m + 1) // 2
    mc = merkle.MerkleCommitment(doc, 0, levels)
    for k, idx in lookups.items():
        say(step="open", log=log, k=k, route="parent: MerkleCommitment.make_wits on the host tree (Python look-ups)", **timed(lambda: mc.make_wits(idx)))
        assert [[tuple(w) for w in ws] for ws in mc.make_wits(idx)] == [[tuple(w) for w in ws] for ws in got[k]], "the routes disagree on an opening"
    say(step="open", log=log, route="parent: bytes held", device_bytes=held_par, device_bytes_by_design=n * 4 + 2 * nodes * 32, host_bytes=int(tree.nbytes),
        note="device: what the stateless call's grow-only scratch buffers keep after it (document + tree + exported tree, each with its 1/8 head-room); host: the tree" +
        ("; two timed runs at this size" if log >= 27 else ""))


def step_check(log, parent_path):
    from reef_amd import _ffi, merkle
    p, pp, keep, doc = setup(log)
    lib = _ffi.load()
    rm = merkle.ResidentMerkleCommitment.new("pallas", doc, p.t, p.rf, p.rp, p.rc, p.mds, p.tag_leaf, p.tag_node)
    rng = np.random.default_rng(2000 + log)
    for k in (1, 32, 1024):
        idx = np.asarray(rng.integers(0, doc.shape[0], size=k), dtype=np.uint64)
        sym, oidx, opp, _ = rm.open_arrays(idx)
        sym, oidx, opp = np.ascontiguousarray(sym), np.ascontiguousarray(oidx), np.ascontiguousarray(opp)
        accept = np.zeros(k, dtype=np.uint32)

        def chk():
            _ffi.check(lib.reef_merkle_check_paths(rm._h, idx.ctypes.data, sym.ctypes.data, oidx.ctypes.data, opp.ctypes.data, k, accept.ctypes.data))
        r = timed(chk)
        assert accept.all(), "an honest opening was refused"
        say(step="check", log=log, k=k, depth=rm.levels, route="reef_merkle_check_paths, host to host", **r)
    rm.close()


def step_kernels(log, parent_path):
    """What the rocprofv3 pass runs: three opens of 1024 lookups, three checks each of 1, 32 and 1024 paths."""
    from reef_amd import merkle
    p, pp, keep, doc = setup(log)
    rm = merkle.ResidentMerkleCommitment.new("pallas", doc, p.t, p.rf, p.rp, p.rc, p.mds, p.tag_leaf, p.tag_node)
    rng = np.random.default_rng(3000 + log)
    for k in (1, 32, 1024):
        idx = [int(x) for x in rng.integers(0, doc.shape[0], size=k)]
        for _ in range(3):
            wits = rm.make_wits(idx)
            assert all(rm.check(idx, wits))
    rm.close()
    say(step="kernels", log=log, done=True)


STEPS = {"create": step_create, "open": step_open, "check": step_check, "kernels": step_kernels}


def run_step(name, log, parent, prefix=()):
    cmd = ["timeout", "-k", "10", str(STEP_LIMIT.get(log, 600))] + list(prefix) + [sys.executable, os.path.abspath(__file__), "--step", name, str(log), parent]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
    rows = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    return r.returncode, rows, r.stderr[-1500:]


def kernel_stats(log, parent):
    """A rocprofv3 --kernel-trace --stats pass of its own over step `kernels`: the rows of the two new kernels."""
    d = tempfile.mkdtemp(prefix="merkle_prof_")
    try:
        rc, rows, err = run_step("kernels", log, parent, prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"])
        if rc != 0:
            return rc, ["rocprofv3 pass failed with %d: %s" % (rc, err.strip().splitlines()[-1] if err.strip() else "")]
        out = []
        for f in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
            for row in csv.DictReader(open(f)):
                name = row.get("Name", "")
                if "k_pos_paths" in name or "k_merkle_open" in name:
                    short = name.split("(")[0].replace("void reef::", "")
                    out.append("%-40s calls %s  average %s ns  min %s ns  max %s ns" % (short, row.get("Calls"), row.get("AverageNs"), row.get("MinNs"), row.get("MaxNs")))
        return 0, out or ["no kernel_stats.csv row names k_pos_paths or k_merkle_open"]
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    if len(sys.argv) >= 5 and sys.argv[1] == "--step":
        STEPS[sys.argv[2]](int(sys.argv[3]), sys.argv[4])
        return
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    parent = os.path.abspath(sys.argv[1])
    out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "r13_merkle_resident_timing.txt")
    logs = [int(x) for x in (sys.argv[3] if len(sys.argv) > 3 else "20,24,27").split(",")]
    from reef_amd import _ffi
    lines = ["# tools/time_merkle_resident.py: %d runs after one warm call, call entry to return, median [min .. max] in ms; library sources %s; parent build %s"
             % (RUNS, _ffi.library_sources_sha16(), bind_parent(parent).reef_version().decode()),
             "# Pallas scalar field, stand-in Poseidon constants (8 full, 56 partial rounds), random symbols below 131, host buffers pageable (numpy)"]
    failed = False
    for log in logs:
        lines.append("")
        lines.append("## 2^%d symbols" % log)
        for name in ("create", "open", "check"):
            if name == "check" and log not in (20, 27):
                continue
            rc, rows, err = run_step(name, log, parent)
            print("step %s at 2^%d: exit %d" % (name, log, rc), file=sys.stderr, flush=True)
            for r in rows:
                if "median_ms" in r:
                    k = "k = %-5d" % r["k"] if "k" in r else "         "
                    depth = " depth %d" % r["depth"] if "depth" in r else ""
                    lines.append("%-7s %s %10.3f [%10.3f .. %10.3f]  %s%s" % (r["step"], k, r["median_ms"], r["min_ms"], r["max_ms"], r["route"], depth))
                elif "device_bytes" in r:
                    lines.append("%-7s           %s: device %d (by design %d), host %d -- %s" % (r["step"], r["route"], r["device_bytes"], r["device_bytes_by_design"], r["host_bytes"], r["note"]))
            if rc != 0:
                lines.append("%-7s FAILED with %d (124: the step's time limit): %s" % (name, rc, err.strip().splitlines()[-1] if err.strip() else ""))
                failed = True
                break
        if failed:
            break
    if not failed:
        lines.append("")
        lines.append("## reef_merkle_check_paths on the host: no figure -- reef_provider.hpp has no host Poseidon (the sponge stays with the caller)")
        lines.append("")
        lines.append("## rocprofv3 --kernel-trace --stats, a pass of its own at 2^20 symbols (three opens and three checks each of 1, 32 and 1024 paths, depth 20)")
        rc, rows = kernel_stats(20, parent)
        lines += rows
        failed = rc != 0
    text = "\n".join(lines) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    print(text)
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
