"""Times reef_ipa_check_batch (include/reef_msm.h 3m) host to host against the code that existed: a loop of m reef_ipa_check_eq calls
on the same inputs.  Usage: python tools/time_ipa_check_batch.py [log2 n ...]   -> text lines (profiles/r19_ipa_check_batch_timing.txt)

Pallas, a pre-shifted key, m honest Hyrax-shaped proofs per cell generated from a seed (one eq point over all k variables, every
fourth proof blinded): random rs, L, R, a_hat, c, and comm set so that the proof verifies -- comm = a_hat G_hat + a_hat b_hat q
(+ blind h) - c q - sum r^2 L - sum r^-2 R, with G_hat and P_hat taken from one reef_ipa_check_eq call on a stand-in comm.  Before
anything is timed the tool asserts that the batch accepts and that every call of the loop accepts.

Both sides are timed as C calls on arguments marshalled beforehand (no Python per proof inside the timed region), alternately, after
a warm-up of every shape: REPEATS repeats; median, minimum and the spread p10..p90 of each.  The condition: the batch is no slower
than the loop -- median(batch) <= median(loop) + (p90 - p10)(loop) -- in every cell; a cell that misses it is marked FAILS.  The
breakdown (the tables and the S pass; the MSM over the key; the one-off points on the second stream) is read from
reef_ipa_check_batch_last_timing in separate runs with the key's timing on (device milliseconds; the two streams overlap)."""
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from reef_amd import _ffi, msm, verify  # noqa: E402
from reef_amd._fe import _arr  # noqa: E402

LOGS = [int(a) for a in sys.argv[1:] if a.isdigit()] or [13, 15, 17]
MS = (1, 4, 16, 64)
REPEATS, WARM, TIMED_RUNS = 21, 3, 5
CURVE = msm.curve_id("pallas")
P = msm.SCALAR_MODULUS[CURVE]
lib = _ffi.load()


def honest_proofs(key, n, count, seed):
    lg = n.bit_length() - 1
    rng = np.random.default_rng(seed)
    rand = lambda: int.from_bytes(rng.bytes(40), "little") % P
    few = msm.gen_bases(CURVE, 900 + seed, 11, 2 * lg + 3)
    q, h = few[2 * lg + 1], few[2 * lg + 2]
    proofs = []
    with msm.MsmContext(CURVE, few[:1].copy(), byte_tables=2) as one:
        for i in range(count):
            jac = np.zeros((2 * lg + 1, 12), dtype=np.uint64)                # random multiples of a few points, lifted to Jacobian
            for j in range(2 * lg + 1):
                one.set_bases(few[j:j + 1].copy())
                jac[j] = one.msm(_arr([rand()]), is_mont=False)
            L, R, stand_in = list(jac[:lg]), list(jac[lg:2 * lg]), jac[2 * lg]
            rs, c, a_hat, point = [rand() or 1 for _ in range(lg)], rand(), rand(), [rand() for _ in range(lg)]
            blind = rand() if i % 4 == 3 else None
            got = verify.ipa_check_eq(key, n, stand_in, c, q, L, R, rs, a_hat, [point], [1], intermediates=True)
            pts, ks = [stand_in, got["g_hat"], q, got["p_hat"]], [1, a_hat, a_hat * got["b_hat"] % P, P - 1]
            if blind is not None:
                pts, ks = pts + [h], ks + [blind]
            comm = verify._lincomb(CURVE, pts, ks)
            proofs.append(dict(comm=comm, c=c, q=q, L=L, R=R, rs=rs, a_hat=a_hat, points=[point], weights=[1], h=None if blind is None else h, blind=blind))
    return proofs


def single_call(key, n, pr):
    """one reef_ipa_check_eq call on arguments marshalled once: () -> accept"""
    ca, qa, La, Ra = verify._jac([pr["comm"]], 1), verify._aff(pr["q"]), verify._jac(pr["L"]), verify._jac(pr["R"])
    cs, rsa, aa, pt, wa = _arr([pr["c"]]), _arr(pr["rs"]), _arr([pr["a_hat"]]), _arr(pr["points"][0]), _arr(pr["weights"])
    ptrs, nvars = (ctypes.c_void_p * 1)(pt.ctypes.data), (ctypes.c_size_t * 1)(len(pr["points"][0]))
    ha = None if pr["h"] is None else verify._aff(pr["h"])
    ba = None if pr["blind"] is None else _arr([pr["blind"]])
    acc = ctypes.c_uint32(0)
    keep = (ca, qa, La, Ra, cs, rsa, aa, pt, wa, ptrs, nvars, ha, ba)
    args = (key._h, n, ca.ctypes.data, cs.ctypes.data, qa.ctypes.data, La.ctypes.data, Ra.ctypes.data, rsa.ctypes.data, aa.ctypes.data,
            ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(nvars, ctypes.c_void_p), wa.ctypes.data, 1, None if ha is None else ha.ctypes.data,
            None if ba is None else ba.ctypes.data, False, ctypes.byref(acc), None, None, None)

    def run(_keep=keep):
        _ffi.check(lib.reef_ipa_check_eq(*args))
        return acc.value
    return run


def batch_call(key, n, proofs, rho):
    structs, ra, keep = verify._marshal_batch(n, proofs, rho)
    acc = ctypes.c_uint32(0)

    def run(_keep=keep):
        _ffi.check(lib.reef_ipa_check_batch(key._h, n, structs, len(proofs), ra.ctypes.data, False, ctypes.byref(acc), None, None, None, 0, None, None))
        return acc.value
    return run


def stats(ts):
    ts = sorted(ts)
    return statistics.median(ts), ts[0], ts[len(ts) // 10], ts[(9 * len(ts)) // 10]


print(f"# {lib.reef_version().decode()}, library sources {_ffi.library_sources_sha16()}: reef_ipa_check_batch against a loop of reef_ipa_check_eq, pallas, "
      f"pre-shifted key, host to host (C calls, arguments marshalled beforehand); {WARM} warm-up calls of every shape, then {REPEATS} repeats, "
      f"batch and loop alternately; ms: median min [p10..p90]")
failed = []
for lg in LOGS:
    n = 1 << lg
    bases = msm.gen_bases(CURVE, 7, 3, n)
    with msm.MsmContext(CURVE, bases, bucket_groups=1, byte_tables=2) as key:
        proofs = honest_proofs(key, n, max(MS), 19 + lg)
        rng = np.random.default_rng(lg)
        rho = [int.from_bytes(rng.bytes(40), "little") % P or 1 for _ in proofs]
        singles = [single_call(key, n, pr) for pr in proofs]
        cells = {m: batch_call(key, n, proofs[:m], rho[:m]) for m in MS}
        for m in MS:                                             # the same answer, and the warm-up of every shape
            for _ in range(WARM):
                assert cells[m]() == 1, f"the batch of {m} honest proofs at n = 2^{lg} does not accept"
                assert all(s() == 1 for s in singles[:m]), f"a single check of an honest proof at n = 2^{lg} does not accept"
        for m in MS:
            tb, tl = [], []
            for _ in range(REPEATS):
                t0 = time.perf_counter()
                cells[m]()
                t1 = time.perf_counter()
                for s in singles[:m]:
                    s()
                t2 = time.perf_counter()
                tb.append((t1 - t0) * 1e3)
                tl.append((t2 - t1) * 1e3)
            (bm, bmin, b10, b90), (lm, lmin, l10, l90) = stats(tb), stats(tl)
            key.enable_timing(True)
            parts = []
            for _ in range(TIMED_RUNS):
                cells[m]()
                parts.append(verify.ipa_check_batch_timing(key))
            key.enable_timing(False)
            sp, km, sd = (statistics.median(x[f] for x in parts) for f in ("s_pass_ms", "key_msm_ms", "side_ms"))
            ok = bm <= lm + (l90 - l10)
            line = (f"pallas n=2^{lg} m={m:2d} batch {bm:8.3f} {bmin:8.3f} [{b10:8.3f}..{b90:8.3f}] per proof {bm / m:7.3f} | loop {lm:8.3f} {lmin:8.3f} "
                    f"[{l10:8.3f}..{l90:8.3f}] per proof {lm / m:7.3f} | loop/batch {lm / bm:6.2f} | timed: S pass {sp:6.3f}, key MSM {km:6.3f}, "
                    f"one-off points {sd:6.3f} | {'ok' if ok else 'FAILS the condition'}")
            print(line, flush=True)
            if not ok:
                failed.append(f"n=2^{lg} m={m}")
print("# every cell meets the condition: the batch is no slower than the loop within the loop's spread" if not failed else
      "# cells that FAIL the condition (batch median > loop median + loop spread): " + ", ".join(failed))
