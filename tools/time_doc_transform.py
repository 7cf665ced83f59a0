#!/usr/bin/env python3
"""Time a document's way from the file's bytes to symbols in device memory (include/reef_msm.h 3l: reef_doc_transform).

    python tools/time_doc_transform.py [OUT]          the whole comparison; OUT defaults to profiles/r15_doc_transform_timing.txt
    python tools/time_doc_transform.py --one ROUTE SHAPE     one measurement in this process, one JSON line (what the first form starts,
                                                             also under rocprofv3 --kernel-trace for the kernel times)

ROUTE:  a   today's route: the transform on the host as a numpy table lookup (for UTF-8: Python's decoder, then the lookup), the padded
            symbols copied up from pageable memory with reef_memcpy.  A STAND-IN for Reef's loop (framework.rs:978-1011: one hash-map lookup
            per character into a Vec<usize>), which cannot be built here and is slower than a table lookup by a factor nobody has measured
        b   reef_doc_transform, pageable host bytes in, device symbols out
        c   reef_doc_transform, device bytes in, device symbols out
SHAPE:  cfg3  1 MiB of printable ASCII, AsciiParser's own alphabet, 1-byte symbols
        cfg4  16 MiB of DNA, the map A, C, G, T -> 0..3, 1-byte symbols
        cfg5  64 MiB of UTF-8 from a seeded mix of 1- to 4-byte characters, Utf8Parser's own alphabet, 4-byte symbols
Every figure is call entry to return (the call waits for its stream), five runs after a warm one; before a time is printed the symbols in
device memory are read back and compared with route a's."""
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
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12                     # the README's HBM figure
RUNS = 5
POOL = [0x41, 0xE9, 0x20AC, 0x1F600, 0xD7FF, 0xE000, 0x10FFFF]
SHAPES = {"cfg3": (1 << 20, "1 MiB ASCII -> 1 byte"), "cfg4": (1 << 24, "16 MiB DNA -> 1 byte"), "cfg5": (1 << 26, "64 MiB UTF-8 -> 4 bytes")}


def make(shape):
    """-> (text bytes, encoding, map or None, alphabet_len, elem_bytes)"""
    n = SHAPES[shape][0]
    rng = np.random.default_rng(15)
    if shape == "cfg3":
        return rng.integers(0x20, 0x7F, n, dtype=np.uint8).tobytes(), 0, None, 128, 1
    if shape == "cfg4":
        m = np.full(256, 0xFFFFFFFF, dtype=np.uint32)
        m[[ord(c) for c in "ACGT"]] = np.arange(4)
        return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, n)].tobytes(), 0, m, 4, 1
    body = np.array(POOL, dtype="<u4")[rng.integers(0, len(POOL), n // 2)].tobytes().decode("utf-32-le").encode("utf-8")
    cut = n
    while (body[cut] & 0xC0) == 0x80:
        cut -= 1
    return body[:cut], 1, None, 0x10F800, 4


def host_transform(text, encoding, map_, alphabet_len, elem_bytes, table):
    """route a's host half: characters -> symbols through a table, EOF, EPSILON, zeros up to a power of two"""
    if encoding == 0:
        c = np.frombuffer(text, dtype=np.uint8)
    else:
        c = np.frombuffer(text.decode("utf-8").encode("utf-32-le"), dtype=np.uint32)
    sym = table[c]
    padded = 2
    while padded < sym.size + 2:
        padded <<= 1
    out = np.zeros(padded, dtype={1: np.uint8, 4: np.uint32}[elem_bytes])
    out[:sym.size] = sym
    out[sym.size], out[sym.size + 1] = alphabet_len + 2, alphabet_len + 1
    return out


def one(route, shape):
    from reef_amd import _ffi
    from reef_amd.msm import DeviceBuffer
    lib = _ffi.load()
    text, encoding, map_, ab_len, eb = make(shape)
    n = len(text)
    # the table of route a: the caller's map, or the encoding's own alphabet written out
    if map_ is not None:
        table = map_.astype({1: np.uint8, 4: np.uint32}[eb])
    elif encoding == 0:
        table = np.arange(256, dtype=np.uint8)
        table[0x1A] = ab_len + 2
    else:
        table = np.arange(0x110000, dtype=np.uint32)
        table[0xE000:] -= 0x800
        table[0x1A] = ab_len + 2
    want = host_transform(text, encoding, map_, ab_len, eb, table)
    src = np.frombuffer(text, dtype=np.uint8)
    d_out = DeviceBuffer(want.nbytes)
    d_text = DeviceBuffer.from_host(src) if route == "c" else None
    info = _ffi.DocInfo()
    m_ptr, m_len = (None, 0) if map_ is None else (map_.ctypes.data, map_.size)
    times, parts = [], []
    for _ in range(RUNS + 1):
        t0 = time.perf_counter()
        if route == "a":
            sym = host_transform(text, encoding, map_, ab_len, eb, table)
            t1 = time.perf_counter()
            _ffi.check(lib.reef_memcpy(d_out.ptr, sym.ctypes.data, sym.nbytes, 1, 0))
            parts.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
        else:
            _ffi.check(lib.reef_doc_transform(d_text.ptr if route == "c" else src.ctypes.data, n, 1 if route == "c" else 0, encoding, m_ptr, m_len,
                                              ab_len + 2, ab_len + 1, d_out.ptr, eb, want.size, 1, ctypes.byref(info)))
        times.append((time.perf_counter() - t0) * 1e3)
    got = d_out.to_host(want.shape, dtype=want.dtype)
    if not np.array_equal(got, want):
        sys.exit("%s %s: the symbols in device memory differ from the host transform's" % (route, shape))
    if route != "a" and (info.kept + 2 > info.padded or info.padded != want.size or info.bad or info.malformed_at != n):
        sys.exit("%s %s: info %s" % (route, shape, [(k, getattr(info, k)) for k, _ in _ffi.DocInfo._fields_]))
    res = {"route": route, "shape": shape, "nbytes": n, "padded": int(want.size), "elem_bytes": eb, "first_call_ms": times[0], "call_ms": times[1:]}
    if parts:
        res["host_ms"], res["copy_ms"] = [p[0] for p in parts[1:]], [p[1] for p in parts[1:]]
    print(json.dumps(res), flush=True)


def child(args):
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--one"] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    if p.returncode != 0 or not lines:
        sys.exit("measurement %s failed (exit %d): %s" % (args, p.returncode, (p.stderr or p.stdout)[-600:]))
    print("measured", *args, file=sys.stderr, flush=True)
    return json.loads(lines[-1])


def kernel_times(args, tmp):
    """Per-kernel durations (us) of one --one run under rocprofv3 --kernel-trace, a run of its own: {kernel name: [durations]}."""
    shutil.rmtree(tmp, ignore_errors=True)
    p = subprocess.run(["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--one"] +
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


def main(out_path):
    from reef_amd import _ffi
    lines = ["# tools/time_doc_transform.py: a document from the file's bytes to symbols in device memory, one MI355X, all routes in one job; library sources %s" % _ffi.library_sources_sha16(),
             "# a = the transform on the host (a numpy table lookup; for UTF-8 Python's decoder first) + reef_memcpy of the padded symbols from pageable memory:",
             "#     a stand-in for Reef's hash-map loop (framework.rs:978-1011), which cannot be built here and is slower than a table lookup by an unknown factor",
             "# b = reef_doc_transform, pageable host bytes -> device symbols;  c = reef_doc_transform, device bytes -> device symbols",
             "# Times in ms, call entry to return, %d calls after a warm one.  The symbols in device memory were compared with route a's before a time was printed." % RUNS]
    results = {}
    for shape in SHAPES:
        lines += ["", "## %s: %s" % (shape, SHAPES[shape][1])]
        for route in "abc":
            r = results[(route, shape)] = child([route, shape])
            extra = "   (host transform %s, copy of %d bytes %s)" % (med_min(r["host_ms"]), r["padded"] * r["elem_bytes"], med_min(r["copy_ms"])) if route == "a" else ""
            lines.append("%s  %9d bytes of text, %9d symbols of %d byte(s)   %s   first call %.3f%s" %
                         (route, r["nbytes"], r["padded"], r["elem_bytes"], med_min(r["call_ms"]), r["first_call_ms"], extra))
        a, b, c = (float(np.median(results[(k, shape)]["call_ms"])) for k in "abc")
        lines.append("b / a = %.3f, c / a = %.3f on the medians" % (b / a, c / a))
    lines += ["", "## route c, kernel time in us from rocprofv3 --kernel-trace, a run of its own per shape (every dispatch: %d timed calls and the warm one)" % RUNS]
    tmp = os.path.join(os.environ.get("TMPDIR", "/tmp"), "time_doc_transform_trace")
    for shape in SHAPES:
        k = kernel_times(["c", shape], tmp)
        pick = lambda key: [v for name, v in k.items() if key in name]
        total = 0.0
        for key in ("k_doc_count", "k_doc_scan", "k_doc_write", "k_doc_tail"):
            v = pick(key)
            if not v:
                sys.exit("%s: %s missing from the trace: %s" % (shape, key, sorted(k)))
            total += float(np.median(v[0]))
            lines.append("%s %-12s %s (%d)" % (shape, key, med_min(v[0]), len(v[0])))
        r = results[("c", shape)]
        moved = 2 * r["nbytes"] + r["padded"] * r["elem_bytes"]
        lines.append("%s sum of the medians %.3f us (call, median: %.3f ms); %d bytes read (the text twice) and written (the symbols): %.0f GB/s = %.3f of the HBM peak of %.0f GB/s" %
                     (shape, total, float(np.median(r["call_ms"])), moved, moved / (total * 1e-6) / 1e9, moved / (total * 1e-6) / HBM_PEAK, HBM_PEAK / 1e9))
    shutil.rmtree(tmp, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    with open(out_path, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        one(sys.argv[2], sys.argv[3])
    elif len(sys.argv) <= 2 and not (len(sys.argv) == 2 and sys.argv[1].startswith("-")):
        main(sys.argv[1] if len(sys.argv) == 2 else os.path.join(ROOT, "profiles", "r15_doc_transform_timing.txt"))
    else:
        sys.exit(__doc__)
