#!/usr/bin/env python3
"""The row commitments of a resident Hyrax document from its own ctx (reef_hyrax_commit, reef_hyrax_eval_comm_own) against the route a
prover took before them, host to host, one process, Pallas, every shape with row blinds.

    python tools/time_hyrax_commit.py [--reps N] [--out FILE] [--resources FILE]      (output: profiles/r14_hyrax_commit_timing.txt)

The route before (every step timed from call entry to return, the sum is the route):
  (1) reef_msm_rows_symbols[_wide]  host symbols, host blinds and h -> host Jacobian rows
  (2) reef_normalize                those rows -> host 32-byte rows (PolyCommit.comm)
  (3) reef_hyrax_create             the same document and blinds again
  (4) reef_hyrax_eval_comm_compressed  the 32-byte rows back up, decoded, comm_LZ     (after an eval_begin, which both routes run untimed)
The route now:
  (3) reef_hyrax_create   (5) reef_hyrax_commit -> host 32-byte rows   (6) reef_hyrax_eval_comm_own
A warm pass of both routes comes first (code objects, workspaces, the key's symbol tables and h's table); then --reps passes, the two
routes in turn.  The symbol tables of the key ctx are cached across calls in both routes alike.  The 32-byte rows and comm_LZ of the two
routes are compared in every pass.  Host buffers are numpy arrays: PAGEABLE memory.  PCIe bytes are counted from the shapes.
--resources FILE: the compiler's report on the new kernel (hipcc -Rpass-analysis=kernel-resource-usage), appended as it is."""
import argparse
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from reef_amd import _ffi, msm  # noqa: E402
from reef_amd.hyrax import HyraxEval  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_hyrax_commit_timing.txt"))
ap.add_argument("--resources", default=None)
args = ap.parse_args()
K0, D = 1234567, 89
P = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001      # Pallas' scalar field
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def fmt(ts):
    return "median %8.3f ms, min %8.3f ms" % (statistics.median(ts) * 1e3, min(ts) * 1e3)


def clock(fn):
    t0 = time.perf_counter()
    out = fn()                                            # every call here returns after the device has finished
    return out, time.perf_counter() - t0


def shape_case(name, num_vars, left, doc, bits):
    rows, cols = 1 << left, 1 << (num_vars - left)
    eb = doc.dtype.itemsize
    rng = random.Random(num_vars + bits)
    blinds = [rng.randrange(P) for _ in range(rows)]
    blinds_arr = np.frombuffer(b"".join(v.to_bytes(32, "little") for v in blinds), dtype=np.uint64).reshape(-1, 4).copy()
    point = [rng.randrange(P) for _ in range(num_vars)]
    h = msm.gen_bases("pallas", 0xB11D, 1, 1)[0].copy()
    bases = msm.gen_bases("pallas", K0, D, cols, device=True)
    steps = {k: [] for k in ("rows", "normalize", "create_old", "eval_comm_compressed", "create_new", "commit", "eval_comm_own")}
    same = True
    with msm.MsmContext("pallas", bases, cols, bucket_groups=1) as key:
        rows_call = (lambda: key.msm_rows_symbols(doc, rows, cols, bits, blinds=blinds_arr, h=h, blinds_are_mont=False)) if eb == 1 else \
            (lambda: key.msm_rows_symbols_wide(doc, rows, cols, bits, blinds=blinds_arr, h=h, blinds_are_mont=False))
        for rep in range(args.reps + 1):
            # the route before
            jac, t1 = clock(rows_call)
            (_, comp), t2 = clock(lambda: msm.normalize("pallas", jac, affine=False, compressed=True))
            hx, t3 = clock(lambda: HyraxEval("pallas", doc, num_vars, left, row_blinds=blinds))
            hx.eval_begin(key, point)
            lz_old, t4 = clock(lambda: hx.eval_comm_compressed(comp.reshape(-1)))
            hx.close()
            # the route now
            hx, t5 = clock(lambda: HyraxEval("pallas", doc, num_vars, left, row_blinds=blinds))
            enc, t6 = clock(lambda: hx.commit(key, h))
            hx.eval_begin(key, point)
            lz_new, t7 = clock(hx.eval_comm_own)
            hx.close()
            same = same and enc == comp.tobytes() and msm.compress("pallas", lz_new) == msm.compress("pallas", lz_old)
            if rep:                                       # pass 0 is the warm one
                for k, t in zip(steps, (t1, t2, t3, t4, t5, t6, t7)):
                    steps[k].append(t)
    old = [sum(x) for x in zip(steps["rows"], steps["normalize"], steps["create_old"], steps["eval_comm_compressed"])]
    new = [sum(x) for x in zip(steps["create_new"], steps["commit"], steps["eval_comm_own"])]
    docb = doc.nbytes
    up_old, down_old = 2 * docb + 2 * 32 * rows + 64 + 96 * rows + 32 * rows, 96 * rows + 32 * rows + 96
    up_new, down_new = docb + 32 * rows + 64, 32 * rows + 96
    say(f"{name}: {rows} x {cols}, {eb}-byte symbols below 2^{bits}, row blinds; rows and comm_LZ of the two routes {'equal' if same else 'DIFFER'}")
    say(f"  before  (1) rows from host symbols         {fmt(steps['rows'])}")
    say(f"          (2) reef_normalize                  {fmt(steps['normalize'])}")
    say(f"          (3) reef_hyrax_create               {fmt(steps['create_old'])}")
    say(f"          (4) eval_comm_compressed            {fmt(steps['eval_comm_compressed'])}")
    say(f"          route (1) + (2) + (3) + (4)         {fmt(old)}     PCIe: {up_old} B up, {down_old} B down")
    say(f"  now     (3) reef_hyrax_create               {fmt(steps['create_new'])}")
    say(f"          (5) reef_hyrax_commit               {fmt(steps['commit'])}")
    say(f"          (6) reef_hyrax_eval_comm_own        {fmt(steps['eval_comm_own'])}")
    say(f"          route (3) + (5) + (6)               {fmt(new)}     PCIe: {up_new} B up, {down_new} B down")
    say(f"  (5) against (1): median {statistics.median(steps['commit']) * 1e3 - statistics.median(steps['rows']) * 1e3:+.3f} ms; "
        f"(1)'s own spread over the passes: {(max(steps['rows']) - min(steps['rows'])) * 1e3:.3f} ms")
    return same


assert msm.device_count() > 0, "no HIP device: nothing is measured without one"
say(f"# tools/time_hyrax_commit.py, {_ffi.load().reef_version().decode()}, library sources {_ffi.library_sources_sha16()}, host buffers pageable (numpy), "
    f"{args.reps} passes after a warm one, the two routes in turn")
gen = np.random.default_rng(0xD0C)
ok = True
ok &= shape_case("cfg4, DNA", 25, 12, gen.integers(0, 5, size=1 << 25, dtype=np.uint8), 3)
ok &= shape_case("cfg4 shape, 9-bit symbols", 25, 12, gen.integers(0, 1 << 9, size=1 << 25, dtype=np.uint16), 9)
ok &= shape_case("cfg4 shape, 16-bit symbols", 25, 12, gen.integers(0, 1 << 16, size=1 << 25, dtype=np.uint16), 16)
ok &= shape_case("cfg3, ASCII", 21, 10, gen.integers(0, 128, size=1 << 21, dtype=np.uint8), 7)
if args.resources:
    say("# the new kernel as the compiler reports it (hipcc --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage):")
    for line in open(args.resources).read().splitlines():
        say("#   " + line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(LINES) + "\n")
sys.exit(0 if ok else 1)
