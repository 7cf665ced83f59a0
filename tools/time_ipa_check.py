"""Times the verifier's IPA check (reef_ipa_check_eq, include/reef_msm.h 3j) host to host against what the public ABI allowed before it.
Usage: python tools/time_ipa_check.py [exp | one-stream | lanes] [log2 n ...]   -> text lines (profiles/r10_ipa_check_timing.txt)
  exp         the +experiment build of the same sources (the A/B partner of the next two)
  one-stream  the +experiment build with REEF_IPA_CHECK_ONE_STREAM=1: the one-off points on the key ctx's stream, ahead of the MSM
  lanes       the +experiment build with REEF_IPA_CHECK_ROUTE=lanes: the one-off points one lane each by double-and-add, the route
              measured against the re-keyed plain key that ships
Run under `rocprofv3 --kernel-trace --stats` for the kernels' own durations (k_ic_s: the s-and-b_hat pass).

The baseline is the same verdict from the calls that existed: s and b built on the host (here: Python big integers, timed apart and
not counted), s uploaded to reef_msm, L and R made affine with reef_normalize and the one-off points summed through mult_pippenger,
b_hat on the host (with s), reef_normalize to compare.  The inputs are random points: nothing verifies, the work is the same."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
mode = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].isdigit() else "release"
if mode in ("exp", "one-stream", "lanes"):
    os.environ["REEF_MSM_LIB"] = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reef_amd", "_lib", "libreef_msm_exp.so")
    if mode == "one-stream":
        os.environ["REEF_IPA_CHECK_ONE_STREAM"] = "1"
    if mode == "lanes":
        os.environ["REEF_IPA_CHECK_ROUTE"] = "lanes"
import numpy as np  # noqa: E402

from reef_amd import _ffi, msm, verify  # noqa: E402
from reef_amd._fe import _arr  # noqa: E402

logs = [int(a) for a in sys.argv[1:] if a.isdigit()] or [13, 15, 16, 17]
RUNS, WARM = 7, 2
lib = _ffi.load()
print(f"# {lib.reef_version().decode()}, library sources {_ffi.library_sources_sha16()}, mode {mode}: reef_ipa_check_eq host to host, "
      f"{WARM} warm-up calls then {RUNS} runs; ms")


def timed(fn):
    for _ in range(WARM):
        fn()
    ts = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts)


for cname in ("pallas", "vesta"):
    cid = msm.curve_id(cname)
    p = msm.SCALAR_MODULUS[cid]
    rng = np.random.default_rng(5 + cid)
    rand = lambda: int.from_bytes(rng.bytes(40), "little") % p
    for lg in logs:
        n = 1 << lg
        bases = msm.gen_bases(cid, 7, 3, n)
        few = msm.gen_bases(cid, 900, 11, 2 * lg + 3)                       # comm, L, R as affine points ...
        jac = np.zeros((2 * lg + 1, 12), dtype=np.uint64)                    # ... lifted to Jacobian by a one-point MSM each
        with msm.MsmContext(cid, few[:1].copy(), byte_tables=2) as one:
            for i in range(2 * lg + 1):
                one.set_bases(few[i:i + 1].copy())
                jac[i] = one.msm(_arr([rand()]), is_mont=False)
        comm, L, R = jac[0], list(jac[1:1 + lg]), list(jac[1 + lg:])
        q, h = few[2 * lg + 1], few[2 * lg + 2]
        rs, c, a_hat, blind, r = [rand() for _ in range(lg)], rand(), rand(), rand(), rand()
        r_x, r_y = [rand() for _ in range(lg)], [rand() for _ in range(lg - 1)]
        for kind, kw in (("plain", dict(bucket_groups=0, byte_tables=2)), ("pre-shifted", dict(bucket_groups=1, byte_tables=2))):
            with msm.MsmContext(cid, bases, **kw) as key:
                med, best = timed(lambda: verify.ipa_check_eq(key, n, comm, c, q, L, R, rs, a_hat, [r_x, r_y], [1, r], h=h, blind=blind))
                line = f"{cname} n=2^{lg} {kind:11s} reef_ipa_check_eq median {med:8.3f} min {best:8.3f}"
                if mode == "release":
                    # ---- the baseline: host s and b (not counted), then the device calls that existed
                    t0 = time.perf_counter()
                    s = [1]
                    for x in rs:
                        xi = pow(x, -1, p)
                        s = [v for e in s for v in (e * xi % p, e * x % p)]
                    sa = _arr(s)
                    host_ms = (time.perf_counter() - t0) * 1e3
                    ks = _arr([c] + [x * x % p for x in rs] + [pow(x, -2, p) for x in rs] + [1])
                    ks2 = _arr([a_hat, a_hat * 3 % p, blind])

                    def baseline():
                        g_hat = key.msm(sa, is_mont=False)
                        aff = msm.normalize(cid, np.vstack([np.stack(L + R), comm[None], g_hat[None]]))[0]
                        lhs = msm.mult_pippenger(cid, np.vstack([q[None], aff[:2 * lg + 1]]), ks, is_mont=False)
                        rhs = msm.mult_pippenger(cid, np.vstack([aff[2 * lg + 1:], q[None], h[None]]), ks2, is_mont=False)
                        both = msm.normalize(cid, np.stack([lhs, rhs]), affine=False, compressed=True)[1]
                        return both[0].tobytes() == both[1].tobytes()
                    bmed, bbest = timed(baseline)
                    line += f" | baseline device calls median {bmed:8.3f} min {bbest:8.3f} (+ host s, Python big integers: {host_ms:8.1f})"
                print(line, flush=True)
