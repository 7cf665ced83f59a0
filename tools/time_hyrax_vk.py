"""Times comm_LZ for m proofs over one document's rows (include/reef_msm.h 3n): ONE reef_hyrax_vk_comm_lz call, encodings included, on a
vk made beforehand -- against the code that existed, m x (reef_amd.verify.comm_lz + compress): per proof an upload and a decode of the
same rows, a fresh context keyed with them, the weights built in Python, one reef_msm, one reef_normalize.
Usage: python tools/time_hyrax_vk.py [left ...]   -> text lines (profiles/r20_hyrax_vk_timing.txt)

Pallas, host to host.  The rows are 2^left seeded points in reef_normalize's encoding; the points are seeded scalars.  The new route
is timed as a C call on arguments marshalled beforehand, on a vk with the library's default key and on one with a pre-shifted key;
the loop is the Python the parent commit shipped, unchanged (its Python is part of what a caller paid).  reef_hyrax_vk_create is
timed apart, host rows to a usable vk.  Before anything is timed the tool asserts that both vks and the loop give the same encodings.
All routes alternate inside one job after a warm-up of every shape: REPEATS repeats; median, minimum and p10..p90 of each.
The condition, per cell and per key: the new route's median is no slower than the loop's p10 -- the loop's own spread and nothing
else; the loop repeats decode, keying and upload that the new route does once, so anything slower would mean the batch dispatch is
wrong rather than unlucky.  A cell that misses it is marked FAILS."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from reef_amd import _ffi, msm, verify  # noqa: E402
from reef_amd._fe import _arr  # noqa: E402

LEFTS = [int(a) for a in sys.argv[1:] if a.isdigit()] or [10, 12, 13]
MS = (1, 4, 16, 64)
REPEATS, WARM, CREATES = 15, 2, 7
CURVE = msm.curve_id("pallas")
P = msm.SCALAR_MODULUS[CURVE]
KEYS = (("default key", {}), ("pre-shifted key", dict(bucket_groups=1, byte_tables=2)))
lib = _ffi.load()


def rows_of(left, seed):
    """2^left seeded points as the 32-byte rows of a .cmt file"""
    n = 1 << left
    aff = msm.gen_bases(CURVE, 1000 + seed, 7, n)
    one = np.frombuffer(((1 << 256) % msm.PALLAS_BASE_P).to_bytes(32, "little"), dtype=np.uint64)
    jac = np.ascontiguousarray(np.concatenate([aff, np.tile(one, (n, 1))], axis=1))
    return msm.normalize(CURVE, jac, affine=False, compressed=True)[1].tobytes()


def vk_call(vk, points):
    """one reef_hyrax_vk_comm_lz call, Jacobian points and encodings, on arguments marshalled once: () -> the encodings"""
    m = len(points)
    pa = _arr([x for pt in points for x in pt])
    jac, enc = np.zeros((m, 12), np.uint64), np.zeros((m, 32), np.uint8)

    def run(_keep=(pa, jac, enc)):
        _ffi.check(lib.reef_hyrax_vk_comm_lz(vk._h, pa.ctypes.data, m, False, jac.ctypes.data, enc.ctypes.data))
        return enc.tobytes()
    return run


def loop_call(rows32, points):
    """the parent commit's route: per proof verify.comm_lz and compress"""
    def run():
        return b"".join(msm.compress(CURVE, verify.comm_lz(CURVE, rows32, pt, P)) for pt in points)
    return run


def stats(ts):
    ts = sorted(ts)
    return statistics.median(ts), ts[0], ts[len(ts) // 10], ts[(9 * len(ts)) // 10]


def fmt(s):
    return f"{s[0]:8.3f} {s[1]:8.3f} [{s[2]:8.3f}..{s[3]:8.3f}]"


print(f"# {lib.reef_version().decode()}, library sources {_ffi.library_sources_sha16()}: comm_LZ of m proofs over one document's 2^left rows, "
      f"pallas, host to host.  new: one reef_hyrax_vk_comm_lz call (Jacobian points and encodings; a C call on arguments marshalled "
      f"beforehand; the vk made outside the timed region) on the default key and on a pre-shifted one; loop: m x (verify.comm_lz + "
      f"compress), the parent commit's code.  {WARM} warm-up calls of every shape, then {REPEATS} repeats, the routes alternately; ms: "
      f"median min [p10..p90].  Condition per cell and key: median(new) <= p10(loop).")
failed = []
for left in LEFTS:
    rows32 = rows_of(left, left)
    rng = np.random.default_rng(left)
    points = [[int.from_bytes(rng.bytes(40), "little") % P for _ in range(left)] for _ in range(max(MS))]
    for name, kw in KEYS:                                            # reef_hyrax_vk_create, host rows to a usable vk
        ts = []
        for _ in range(CREATES):
            t0 = time.perf_counter()
            vk = verify.HyraxVk(CURVE, rows32, left, **kw)
            ts.append((time.perf_counter() - t0) * 1e3)
            vk.close()
        print(f"pallas left={left:2d} reef_hyrax_vk_create, {name:15s}: {fmt(stats(ts[1:]))}  (first call of the job: {ts[0]:.3f})", flush=True)
    vks = [verify.HyraxVk(CURVE, rows32, left, **kw) for _, kw in KEYS]
    try:
        for m in MS:
            news = [vk_call(vk, points[:m]) for vk in vks]
            loop = loop_call(rows32, points[:m])
            for _ in range(WARM):
                want = loop()
                assert all(n() == want for n in news), f"left = {left}, m = {m}: the routes disagree"
            tn, tl = [[] for _ in news], []
            for _ in range(REPEATS):
                for k, n in enumerate(news):
                    t0 = time.perf_counter()
                    n()
                    tn[k].append((time.perf_counter() - t0) * 1e3)
                t0 = time.perf_counter()
                loop()
                tl.append((time.perf_counter() - t0) * 1e3)
            ls = stats(tl)
            for k, (name, _) in enumerate(KEYS):
                ns = stats(tn[k])
                ok = ns[0] <= ls[2]
                print(f"pallas left={left:2d} m={m:2d} {name:15s} new {fmt(ns)} per proof {ns[0] / m:7.3f} | loop {fmt(ls)} per proof {ls[0] / m:7.3f} "
                      f"| loop/new {ls[0] / ns[0]:7.2f} | {'ok' if ok else 'FAILS the condition'}", flush=True)
                if not ok:
                    failed.append(f"left={left} m={m} {name}")
    finally:
        for vk in vks:
            vk.close()
print("# every cell meets the condition: the new route's median is no slower than the loop's p10" if not failed else
      "# cells that FAIL the condition (median(new) > p10(loop)): " + ", ".join(failed))
