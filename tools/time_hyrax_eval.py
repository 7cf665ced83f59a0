"""The Hyrax consistency argument on the device, host to host (reef_amd.hyrax.HyraxEval; include/reef_msm.h 3i), against the host-a
route: reef_mle_bound_rows with LZ back to the host, then reef_ipa_cross_terms with a uploaded every round.

    python tools/time_hyrax_eval.py [reps]
    python tools/time_hyrax_eval.py --one          (ONE argument, Pallas at R = 2^13, pre-shifted key, no baseline: for rocprofv3)

Pallas, R = 2^11 (num_vars 22, cfg3) and 2^13 (num_vars 25, cfg4), a document of random 1-byte symbols filling 2^num_vars, left =
num_vars / 2; the gens_v key with default options and pre-shifted (bucket_groups = 1).  Reported, median over `reps` arguments with
random challenges and the per-round h term off: eval_begin (LZ, eval, b), ipa_begin (c_L, c_R, round 0's L, R), the mean round
(fold + next L, R), finish, and the whole argument.  Baseline, in the same process on the same key: reef_mle_bound_rows with LZ to
the host, and reef_ipa_cross_terms of every round k >= 1 with a (R / 2^k random scalars) uploaded from the host, the mean over k."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from reef_amd import mle, msm                          # noqa: E402
from reef_amd.hyrax import HyraxEval, factored_lens    # noqa: E402

P = 0x40000000000000000000000000000000224698fc0994a8dd8c46eb2100000001   # Pallas scalars (Fq)


def rand_fe(rng):
    return int(rng.integers(1, 1 << 62)) << 188 | int(rng.integers(0, 1 << 62))


def one_argument(hx, key, point, q, rng):
    t = {"eval_begin": [], "ipa_begin": [], "round": [], "finish": []}

    def call(name, fn, *a):
        t0 = time.perf_counter()
        fn(*a)
        t[name].append((time.perf_counter() - t0) * 1e3)
    call("eval_begin", hx.eval_begin, key, point)
    call("ipa_begin", hx.ipa_begin, q)
    for _ in range(hx.right - 1):
        call("round", hx.ipa_round, rand_fe(rng))
    call("finish", hx.finish, rand_fe(rng))
    return {k: statistics.mean(v) for k, v in t.items()}, sum(sum(v) for v in t.values())


def baseline(key, z, point, left, n, rng):
    """(reef_mle_bound_rows with LZ to the host, the mean reef_ipa_cross_terms of rounds 1 .. log2(n) - 1 with a from the host), ms"""
    pa = mle.ints_to_array(point)
    t0 = time.perf_counter()
    mle.bound_rows_raw(0, z, pa, left, is_mont=False)
    bound = (time.perf_counter() - t0) * 1e3
    ts, w1s, w2s = [], [], []
    for k in range(1, n.bit_length() - 1):
        w1s.append(rand_fe(rng))
        w2s.append(rand_fe(rng))
        a = rng.integers(0, 1 << 62, size=(n >> k, 4), dtype=np.uint64)
        t0 = time.perf_counter()
        key.ipa_cross_terms(a, w1s, w2s, is_mont=False)
        ts.append((time.perf_counter() - t0) * 1e3)
    return bound, statistics.mean(ts)


def main():
    one = "--one" in sys.argv
    reps = 1 if one else int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
    print(f"# tools/time_hyrax_eval.py: the Hyrax consistency argument on Pallas, a document of 2^num_vars random 1-byte symbols, "
          f"left = num_vars / 2, R = 2^right, median over {reps} arguments, host to host, ms; round = the mean IPA round (fold + L, R); "
          f"baseline = reef_mle_bound_rows with LZ to the host, and reef_ipa_cross_terms with a from the host, mean over rounds "
          f"1 .. right - 1, same key, same process")
    rng = np.random.default_rng(3)
    for num_vars in ((25,) if one else (22, 25)):
        left, right = factored_lens(num_vars)
        n = 1 << right
        z = rng.integers(0, 256, size=1 << num_vars, dtype=np.uint64).astype(np.uint8)
        point = [rand_fe(rng) % P for _ in range(num_vars)]
        bases = msm.gen_bases(0, 42, 5, n)
        q = msm.gen_bases(0, 1000003, 1, 1)[0]
        for groups in ((1,) if one else (0, 1)):
            with HyraxEval(0, z, num_vars) as hx, msm.MsmContext(0, bases, bucket_groups=groups) as key:
                if not one:
                    one_argument(hx, key, point, q, rng)          # warm: the workspace, q's nibble table
                    baseline(key, z, point, left, n, rng)
                runs = [one_argument(hx, key, point, q, rng) for _ in range(reps)]
                bases_ = [baseline(key, z, point, left, n, rng) for _ in range(0 if one else reps)]
                kind = "byte tables" if key.has_byte_tables() else ("pre-shifted" if key.plan()["bucket_groups"] == 1 else "plain")
            med = {k: statistics.median(r[0][k] for r in runs) for k in runs[0][0]}
            total = statistics.median(r[1] for r in runs)
            bb = statistics.median(b[0] for b in bases_) if bases_ else float("nan")
            br = statistics.median(b[1] for b in bases_) if bases_ else float("nan")
            print(f"pallas R 2^{right:2d} (num_vars {num_vars})  key {kind:11s}  eval_begin {med['eval_begin']:6.3f}  ipa_begin {med['ipa_begin']:6.3f}  "
                  f"round {med['round']:6.3f} x {right - 1:2d}  finish {med['finish']:6.3f}  total {total:7.3f} ms  |  baseline bound_rows {bb:6.3f}  "
                  f"round {br:6.3f} ms  round / baseline {med['round'] / br:5.3f}")


if __name__ == "__main__":
    main()
