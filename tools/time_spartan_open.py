"""The batched IPA opening of the final SNARK on the device, host to host (reef_amd.spartan.Opening; include/reef_msm.h 3h), against
reef_ipa_cross_terms with a uploaded from the host as the baseline round.

    python tools/time_spartan_open.py [reps] [--quick]
    python tools/time_spartan_open.py --one          (one prove and ONE opening, Pallas at 2^16, no baseline: for rocprofv3)

Per curve and padded size (num_cons_pad = num_vars_pad = 2^14, 2^15, 2^16, 2^20): a NIFS ctx with SYNTHETIC matrices (the
generator of tools/_synthetic.py; num_cons = num_vars = the padded size minus 3, num_io = 2), a random running instance, one prove of
both sum-checks (3g), then `reps` openings on it, each with random challenges.  The key is gens_v with default options (reported:
its kind).  Reported: begin (eq tables, cross term), fold, the mean IPA round (fold + next L, R), ipa_begin, finish and the whole
opening, each the median over the openings, host to host.  Baseline, in the same process on the same key: reef_ipa_cross_terms
of every round k >= 1 with a (n / 2^k random scalars) uploaded from the host, the mean over k, median over `reps` sweeps."""
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from reef_amd import msm                               # noqa: E402
from reef_amd.nifs import Nifs                         # noqa: E402
from reef_amd.spartan import Opening, Spartan          # noqa: E402
from _synthetic import synthetic_matrix                # noqa: E402
from time_spartan import one_prove                     # noqa: E402

SIZES = [14, 15, 16, 20]


def rand_fe(rng):
    return int(rng.integers(1, 1 << 62)) << 188 | int(rng.integers(0, 1 << 62))


def one_opening(op, key, n, q, rng):
    t = {"begin": [], "fold": [], "ipa_begin": [], "round": [], "finish": []}

    def call(name, fn, *a):
        t0 = time.perf_counter()
        fn(*a)
        t[name].append((time.perf_counter() - t0) * 1e3)
    call("begin", op.begin, key)
    call("fold", op.fold, rand_fe(rng))
    call("ipa_begin", op.ipa_begin, q)
    for _ in range(n.bit_length() - 2):
        call("round", op.ipa_round, rand_fe(rng))
    call("finish", op.finish, rand_fe(rng))
    return {k: statistics.mean(v) for k, v in t.items()}, sum(sum(v) for v in t.values())


def baseline_sweep(key, n, rng):
    """reef_ipa_cross_terms of rounds 1 .. log2(n) - 1, a from the host: the mean call, ms"""
    ts = []
    w1s, w2s = [], []
    for k in range(1, n.bit_length() - 1):
        w1s.append(rand_fe(rng))
        w2s.append(rand_fe(rng))
        a = rng.integers(0, 1 << 62, size=(n >> k, 4), dtype=np.uint64)
        t0 = time.perf_counter()
        key.ipa_cross_terms(a, w1s, w2s, is_mont=False)
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.mean(ts)


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 10
    one = "--one" in sys.argv
    sizes = [16] if one else SIZES[:2] if "--quick" in sys.argv else SIZES
    reps = 1 if one else reps
    print(f"# tools/time_spartan_open.py: the batched IPA opening per curve and padded size after one prove of the sum-checks, SYNTHETIC "
          f"matrices, num_cons = num_vars = pad - 3, n = pad, median over {reps} openings, host to host, ms; round = the mean IPA round "
          f"(fold + L, R); baseline = reef_ipa_cross_terms with a from the host, mean over rounds 1 .. log2(n) - 1, same key, same process")
    rng = np.random.default_rng(2)
    for curve in (0,) if one else (0, 1):
        for lg in sizes:
            pad = 1 << lg
            n, nio = pad - 3, 2
            nz = n + 1 + nio
            long_rows = rng.choice(n, size=4, replace=False)
            bases = msm.gen_bases(curve, 42, 5, pad)
            q = msm.gen_bases(curve, 1000003, 1, 1)[0]
            with Nifs(curve, n, n, nio) as nf, msm.MsmContext(curve, bases) as key:
                for k in range(3):
                    r, c, v, _ = synthetic_matrix(rng, n, nz, long_rows)
                    nf.set_matrix(k, r, c, v)
                w = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
                e = rng.integers(0, 1 << 62, size=(n, 4), dtype=np.uint64)
                x = rng.integers(0, 1 << 62, size=(nio, 4), dtype=np.uint64)
                nf.set_running(w, e, np.array([[7, 0, 0, 0]], dtype=np.uint64), x)
                one_prove(Spartan(nf), pad, pad, rng)
                op = Opening(nf)
                if not one:
                    one_opening(op, key, pad, q, rng)             # warm: the workspace, q's nibble table
                    baseline_sweep(key, pad, rng)
                runs = [one_opening(op, key, pad, q, rng) for _ in range(reps)]
                base = float("nan") if one else statistics.median(baseline_sweep(key, pad, rng) for _ in range(reps))
                kind = "byte tables" if key.has_byte_tables() else ("pre-shifted" if key.plan()["bucket_groups"] == 1 else "plain")
            med = {k: statistics.median(r[0][k] for r in runs) for k in runs[0][0]}
            total = statistics.median(r[1] for r in runs)
            print(f"{'pallas' if curve == 0 else 'vesta ':6s} n 2^{lg:2d}  key {kind:11s}  begin {med['begin']:6.3f}  fold {med['fold']:6.3f}  "
                  f"ipa_begin {med['ipa_begin']:6.3f}  round {med['round']:6.3f} x {lg - 1:2d}  finish {med['finish']:6.3f}  total {total:7.3f} ms  "
                  f"|  baseline round {base:6.3f} ms  round / baseline {med['round'] / base:5.3f}")


if __name__ == "__main__":
    main()
