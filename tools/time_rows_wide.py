#!/usr/bin/env python3
"""Hyrax row commitments from 16-bit document symbols (reef_msm_rows_symbols_wide) against the only way such a document could be committed
before: reef_msm_rows on the same values as 32-byte field elements.  One process, Pallas, uniform symbols below 2^b.

    python tools/time_rows_wide.py [--reps N] [--fe-only | --no-fe]       (output: profiles/r09_rows_wide_timing.txt)

Per shape and width:
  (a) the new entry, tables cold  : host symbols -> host results; another (b, row_len) was committed on the context just before, so the
                                    plane tables are rebuilt inside the timed call (the workspace is already allocated)
  (b) the new entry, tables cached: host symbols -> host results
  (c) its kernels alone           : HIP events of the context (k_sym_entries_wide .. k_final), symbols and results on the device, tables cached
  (d) reef_msm_rows, max_scalar_bits = b, host field elements (canonical) -> host results
and, as the yardstick for the kernels, reef_msm_rows_symbols at b = 8 on the same shape, (a) to (c).
Host buffers are numpy arrays: PAGEABLE memory.  --fe-only runs (d) alone and uses nothing a checkout from before the wide entry lacks, so
that (d) can be taken from a build of that commit; --no-fe leaves (d) out.  Every timed configuration is checked on three rows against the
discrete logarithm of the key (B_j = (k0 + j d) G)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
from oracle.pasta_oracle import CURVES  # noqa: E402
from reef_amd import _ffi, msm  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--fe-only", action="store_true")
ap.add_argument("--no-fe", action="store_true")
args = ap.parse_args()
K0, D = 1234567, 89
C = CURVES["pallas"]


def spread(ts):
    return "median %.3f ms (min %.3f max %.3f, %d runs)" % (statistics.median(ts) * 1e3, min(ts) * 1e3, max(ts) * 1e3, len(ts))


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()                                              # host results: the call returns after the device has finished
        ts.append(time.perf_counter() - t0)
    return ts


def check(doc, rows, row_len, res):
    comp = msm.compress("pallas", res)
    w = K0 + np.arange(row_len, dtype=object) * D
    for r in (0, rows // 2, rows - 1):
        acc = int((doc[r * row_len:(r + 1) * row_len].astype(object) * w).sum()) % C.order
        if comp[32 * r:32 * r + 32] != C.compress(C.mul(acc, C.gen)):
            return "MISMATCH at row %d" % r
    return "ok"


def symbols_case(ctx, doc, rows, row_len, b, wide):
    call = (lambda s, **kw: ctx.msm_rows_symbols_wide(s, rows, row_len, b, **kw)) if wide else (lambda s, **kw: ctx.msm_rows_symbols(s, rows, row_len, b, **kw))
    evict_doc = np.zeros(8, dtype=doc.dtype)
    evict = (lambda: ctx.msm_rows_symbols_wide(evict_doc, 1, 8, b)) if wide else (lambda: ctx.msm_rows_symbols(evict_doc, 1, 8, b))
    res = call(doc)                                       # allocates the workspace, loads the code
    ok = check(doc, rows, row_len, res)
    cold = []
    for _ in range(args.reps):
        evict()                                           # tables for (b, 8): the next call rebuilds those for (b, row_len)
        cold += timed(lambda: call(doc), 1)
    cached = timed(lambda: call(doc), args.reps)
    d_doc, d_out = msm.DeviceBuffer.from_host(doc), msm.DeviceBuffer(96 * rows)
    kw = dict(elem_bytes=doc.dtype.itemsize) if wide else {}
    call(d_doc, out=d_out, **kw)
    ctx.sync()
    ctx.enable_timing(True)
    kern, acc = [], []
    for _ in range(args.reps):
        call(d_doc, out=d_out, **kw)
        ctx.sync()
        t, a = ctx.last_timing()
        kern.append(t * 1e-3)
        acc.append(a * 1e-3)
    ctx.enable_timing(False)
    ok2 = check(doc, rows, row_len, d_out.to_host((rows, 12)))
    name = "reef_msm_rows_symbols_wide uint16" if wide else "reef_msm_rows_symbols uint8 (yardstick)"
    print(f"{rows} x {row_len}, b = {b}, {name}: check {ok}, {ok2}")
    print(f"  (a) tables cold,   host to host: {spread(cold)}")
    print(f"  (b) tables cached, host to host: {spread(cached)}")
    print(f"  (c) kernels alone (events):      {spread(kern)}; k_accum0 alone {spread(acc)}", flush=True)


def fe_case(ctx, doc, rows, row_len, b):
    sc = np.zeros((rows * row_len, 4), dtype=np.uint64)
    sc[:, 0] = doc
    res = ctx.msm_rows(sc, rows, row_len, is_mont=False, max_scalar_bits=b)
    ok = check(doc, rows, row_len, res)
    ts = timed(lambda: ctx.msm_rows(sc, rows, row_len, is_mont=False, max_scalar_bits=b), args.reps)
    print(f"{rows} x {row_len}, b = {b}, reef_msm_rows on {sc.nbytes >> 20} MiB of field elements: check {ok}")
    print(f"  (d) host to host: {spread(ts)}", flush=True)


print(f"# tools/time_rows_wide.py, {_ffi.load().reef_version().decode()}, library sources {_ffi.library_sources_sha16()}, host buffers pageable (numpy), "
      f"{args.reps} runs a figure" + (", (d) only" if args.fe_only else ""))
for rows, row_len, widths in ((4096, 8192, (9, 12, 16)), (1024, 1024, (12,))):
    bases = msm.gen_bases("pallas", K0, D, row_len, device=True)
    with msm.MsmContext("pallas", bases, row_len, bucket_groups=1) as ctx:
        ctx.msm(msm.gen_scalars("pallas", 1, min(row_len, 1024)))          # first-launch costs out of the way
        rng = np.random.default_rng(0xD0C)
        for b in widths:
            doc = rng.integers(0, 1 << b, size=rows * row_len, dtype=np.uint16)
            if not args.fe_only:
                symbols_case(ctx, doc, rows, row_len, b, True)
            if not args.no_fe:
                fe_case(ctx, doc, rows, row_len, b)
        if not args.fe_only:
            symbols_case(ctx, rng.integers(0, 256, size=rows * row_len, dtype=np.uint8), rows, row_len, 8, False)
