"""Times the Hyrax consistency arguments of m proofs over one resident document in lock-step (include/reef_msm.h 3p) against m single
arguments (3i) run one after another on the same inputs.
Usage: python tools/time_hyrax_batch.py batch            -> the batch, per phase, on this checkout's build
       python tools/time_hyrax_batch.py singles [TREE]   -> the looped singles; TREE: another built checkout (the parent commit's)
                                                            whose reef_amd package and library are used instead of this one's
       python tools/time_hyrax_batch.py split            -> one warm batch argument at m = 64 on the pre-shifted key and nothing else,
                                                            to be run under a kernel trace for the per-kernel split of a round
Text lines (profiles/r22_hyrax_batch_timing.txt holds the three outputs one after the other, with the ratios worked out from them).

Pallas, 1-byte symbols, R = 2^13 (num_vars = 25, left = 12), the h term on, on a pre-shifted key and on the library's default key;
m in {1, 2, 8, 32, 64}.  Host to host: C calls on arguments marshalled beforehand, seeded points, q, blinds and challenges (the
device work does not depend on their values).  Every cell is warmed once, then REPEATS whole arguments; ms: median min [p10..p90].
batch: eval_begin, ipa_begin, one round (the median of the argument's 12 ipa_round calls), finish, and the whole argument.
singles: m x (eval_begin, ipa_begin, 12 x ipa_round, finish), the whole loop."""
import ctypes
import os
import statistics
import sys
import time

MODE = sys.argv[1] if len(sys.argv) > 1 else "batch"
TREE = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, TREE)
import numpy as np  # noqa: E402

from reef_amd import _ffi, msm  # noqa: E402
from reef_amd._fe import _arr  # noqa: E402
from reef_amd.hyrax import HyraxEval  # noqa: E402

NUM_VARS, LEFT = 25, 12
RIGHT = NUM_VARS - LEFT
MS = (64,) if MODE == "split" else (1, 2, 8, 32, 64)
REPEATS = 1 if MODE == "split" else 7
CURVE = msm.curve_id("pallas")
P = msm.SCALAR_MODULUS[CURVE]
KEYS = (("pre-shifted key", dict(bucket_groups=1, byte_tables=2)), ("default key", {}))
if MODE == "split":
    KEYS = KEYS[:1]
lib = _ffi.load()
vp = ctypes.c_void_p


def scalars(rng, n):
    return [1 + int.from_bytes(rng.bytes(40), "little") % (P - 1) for _ in range(n)]


def stats(ts):
    ts = sorted(ts)
    return statistics.median(ts), ts[0], ts[len(ts) // 10], ts[(9 * len(ts)) // 10]


def fmt(s):
    return f"{s[0]:9.3f} {s[1]:9.3f} [{s[2]:9.3f}..{s[3]:9.3f}]"


def ms_of(fn):
    t0 = time.perf_counter()
    _ffi.check(fn())
    return (time.perf_counter() - t0) * 1e3


rng = np.random.default_rng(22)
z = rng.integers(0, 256, size=(1 << NUM_VARS) - 1000, dtype=np.uint64).astype(np.uint8)
gens = msm.gen_bases(CURVE, 7, 3, 1 << RIGHT)
M = max(MS)
qs = np.ascontiguousarray(msm.gen_bases(CURVE, 100003, 5, M))
h = np.ascontiguousarray(msm.gen_bases(CURVE, 5003, 1, 1)[0])
points = _arr(scalars(rng, M * NUM_VARS))                      # m x num_vars, row-major
blinds = [_arr(scalars(rng, 2 * M)) for _ in range(RIGHT)]      # per round: (bl, br) of proof 0, of proof 1, ...
rs = [_arr(scalars(rng, M)) for _ in range(RIGHT)]              # per round: one challenge per proof
row_blinds = scalars(rng, 1 << LEFT)

print(f"# {lib.reef_version().decode()}, library sources {_ffi.library_sources_sha16()}, mode {MODE}: pallas, 1-byte symbols, num_vars = {NUM_VARS}, "
      f"left = {LEFT} (R = 2^{RIGHT}), row blinds and the h term; host to host, C calls on arguments marshalled beforehand; one warm-up argument "
      f"per cell, then {REPEATS}; ms: median min [p10..p90]", flush=True)
with HyraxEval(CURVE, z, NUM_VARS, LEFT, row_blinds=row_blinds) as hx:
    for kname, kw in KEYS:
        with msm.MsmContext(CURVE, gens, **kw) as key:
            if MODE == "singles":
                ev, L, R = np.zeros((2, 4), np.uint64), np.zeros(12, np.uint64), np.zeros(12, np.uint64)

                def single(i):
                    _ffi.check(lib.reef_hyrax_eval_begin(hx._h, key._h, points[i * NUM_VARS:].ctypes.data, False, ev[0].ctypes.data, ev[1].ctypes.data))
                    _ffi.check(lib.reef_hyrax_ipa_begin(hx._h, qs[i].ctypes.data, h.ctypes.data, blinds[0][2 * i:].ctypes.data, False, L.ctypes.data, R.ctypes.data))
                    for k in range(RIGHT - 1):
                        _ffi.check(lib.reef_hyrax_ipa_round(hx._h, rs[k][i:].ctypes.data, blinds[k + 1][2 * i:].ctypes.data, False, L.ctypes.data, R.ctypes.data))
                    _ffi.check(lib.reef_hyrax_finish(hx._h, rs[RIGHT - 1][i:].ctypes.data, False, ev[0].ctypes.data, ev[1].ctypes.data))
                for m in MS:
                    ts = []
                    for rep in range(REPEATS + 1):
                        t0 = time.perf_counter()
                        for i in range(m):
                            single(i)
                        ts.append((time.perf_counter() - t0) * 1e3)
                    s = stats(ts[1:])
                    print(f"singles {kname:15s} m={m:2d} loop of m arguments {fmt(s)} per proof {s[0] / m:8.3f}", flush=True)
                continue
            from reef_amd.hyrax import HyraxBatch  # noqa: E402
            with HyraxBatch(hx, M) as hb:
                ev, lb = np.zeros((M, 4), np.uint64), np.zeros((M, 4), np.uint64)
                L, R = np.zeros((M, 12), np.uint64), np.zeros((M, 12), np.uint64)
                for m in MS:
                    cols = {"eval_begin": [], "ipa_begin": [], "one round": [], "finish": [], "whole argument": []}
                    for rep in range(REPEATS + 1):
                        t0 = time.perf_counter()
                        a = ms_of(lambda: lib.reef_hyrax_batch_eval_begin(hb._h, key._h, points.ctypes.data, m, False, ev.ctypes.data, lb.ctypes.data))
                        b = ms_of(lambda: lib.reef_hyrax_batch_ipa_begin(hb._h, qs.ctypes.data, h.ctypes.data, blinds[0].ctypes.data, False, L.ctypes.data, R.ctypes.data))
                        rounds = [ms_of(lambda: lib.reef_hyrax_batch_ipa_round(hb._h, rs[k].ctypes.data, blinds[k + 1].ctypes.data, False, L.ctypes.data, R.ctypes.data))
                                  for k in range(RIGHT - 1)]
                        f = ms_of(lambda: lib.reef_hyrax_batch_finish(hb._h, rs[RIGHT - 1].ctypes.data, False, ev.ctypes.data, lb.ctypes.data))
                        whole = (time.perf_counter() - t0) * 1e3
                        if rep or REPEATS == 1:
                            for name, v in zip(cols, (a, b, statistics.median(rounds), f, whole)):
                                cols[name].append(v)
                    for name, ts in cols.items():
                        s = stats(ts)
                        print(f"batch   {kname:15s} m={m:2d} {name:15s} {fmt(s)} per proof {s[0] / m:8.3f}", flush=True)
