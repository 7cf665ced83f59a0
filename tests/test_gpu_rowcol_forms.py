"""The row / column sums of the bucket reduction have two forms (engine.inc: rowcol_lanes): one four-wave workgroup per sum
(k_reduce_rowcol_coop, the shortest chain) and LPS lanes per sum, 64 / LPS sums per wave (k_reduce_rowcol<C, LPS>, the fewest
instructions).  Every case here is checked two ways: the point must be the oracle's (oracle.pasta_oracle: bases with known discrete
logarithms, compressed encoding), and the forced four-wave form and every forced LPS must agree with one another.  The matrix is
chosen through window_bits on 1536-4096 points, so that it is sparse and a run is short; pre-shifted keys have more than 1024 points,
because smaller ones are served from nibble tables and have no bucket matrix.  The last test is about the rule that picks the form."""
import threading

import numpy as np
import pytest

from oracle.pasta_oracle import CURVES, SplitMix64, msm_via_dlog, uniform_scalar

pytestmark = pytest.mark.gpu
CID = {"pallas": 0, "vesta": 1}
FORMS = ("0", "64", "32", "16")          # REEF_MSM_ROWCOL: four waves per sum, then the lanes per sum
K0, D = 0x5EED, 7                        # bases B_i = (K0 + i * D) * G


def limbs(v):
    return [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def as_array(ints):
    return np.array([limbs(v) for v in ints], dtype=np.uint64).reshape(len(ints), 4)


def expected(name, ints):
    C = CURVES[name]
    return C.compress(msm_via_dlog(C, ints, K0, D))


def from_windows(c, vals):
    """The canonical scalar whose c-bit windows are vals (each in 1 .. 2^(c-1): such a window is its own signed digit, no carry)."""
    return sum(v << (c * w) for w, v in enumerate(vals))


def patterns(name, c, n, seed):
    """name of the pattern -> n canonical scalars.  Bucket b = i * cols + j of the 2^c1 x 2^c2 matrix holds the entries of digit b + 1."""
    order = CURVES[name].order
    rng = SplitMix64(seed)
    used = 250 // c                                       # windows that stay below the group order
    half = 1 << (c - 1)
    c2 = c // 2
    rows, cols = half >> c2, 1 << c2
    out = {"uniform": [uniform_scalar(rng, order) for _ in range(n)]}
    out["all equal"] = [uniform_scalar(rng, order)] * n   # one bucket per window is non-empty, every other row and column sum is empty
    out["first and last bucket"] = [from_windows(c, [1 if i % 2 == 0 else half] * used) for i in range(n)]
    r0, j0 = rows - 1, cols - 1                           # row r0 stays empty; column j0 gets an entry in every other row
    sc = []
    for p in range(n):
        vals = []
        for w in range(used):
            i, j = divmod(rng.next() % half, cols)
            if w == 0 and p < rows:
                i, j = p, j0
            if i == r0:
                i = (i + 1) % rows
            vals.append(i * cols + j + 1)
        sc.append(from_windows(c, vals))
    out["one row empty, one column full"] = sc
    return out


def every_form(monkeypatch, name, bases, window_bits, groups, cases):
    """cases: label -> (ints, call(ctx, scalars) -> Jacobian points).  Runs them under every forced form, each on a context of its own (the
    switch is read when a context is made); -> form -> label -> compressed bytes, after checking which form the context counted."""
    from reef_amd import msm
    got = {}
    for form in FORMS:
        monkeypatch.setenv("REEF_MSM_ROWCOL", form)
        with msm.MsmContext(name, bases, window_bits=window_bits, bucket_groups=groups) as ctx:
            assert ctx.plan()["window_bits"] == window_bits
            got[form] = {label: msm.compress(name, call(ctx, as_array(ints))) for label, (ints, call) in cases.items()}
            n = ctx.rowcol_forms()
            assert (n["latency"] > 0, n["throughput"] > 0) == (form == "0", form != "0"), (form, n)   # the switch took hold
    return got


def one_msm(ctx, sc):
    return ctx.msm(sc, is_mont=False)


@pytest.mark.parametrize("c,n", [(3, 1536), (6, 1536), (13, 4096), (17, 4096)])   # 2 x 2, 4 x 8, 64 x 64, 256 x 256 buckets
def test_matrix_shapes_and_scalar_patterns(c, n, gpu_lib, cref, experiment_build, monkeypatch):
    name = "pallas"
    bases = cref.gen_bases_ap(CID[name], K0, D, n)
    cases = {label: (ints, one_msm) for label, ints in patterns(name, c, n, 100 + c).items()}
    cases["n = 1"] = ([uniform_scalar(SplitMix64(c), CURVES[name].order)], one_msm)
    want = {label: expected(name, ints) for label, (ints, _) in cases.items()}
    got = every_form(monkeypatch, name, bases, c, 1, cases)
    for label in cases:
        assert len({got[f][label] for f in FORMS}) == 1, (label, "the forms disagree")
        for f in FORMS:
            assert got[f][label] == want[label], (label, f)


@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_both_curves_and_the_other_paths_through_the_pipeline(name, gpu_lib, cref, experiment_build, monkeypatch):
    """64 x 64 buckets: a pre-shifted key (one bucket group per result), plain keys with 20 and with 4 groups per result (their sums share
    waves across group borders at LPS < 64), and one msm_rows call with two rows."""
    c, n = 13, 2048
    bases = cref.gen_bases_ap(CID[name], K0, D, n)
    pats = patterns(name, c, n, 7 + CID[name])
    two_rows = pats["uniform"][:1024] + pats["one row empty, one column full"][:1024]

    def rows_call(ctx, sc):
        return ctx.msm_rows(sc, 2, 1024, is_mont=False)
    want_rows = expected(name, two_rows[:1024]) + expected(name, two_rows[1024:])
    for groups in (1, 0, 4):
        cases = {"uniform": (pats["uniform"], one_msm), "all equal": (pats["all equal"], one_msm), "two rows": (two_rows, rows_call)}
        got = every_form(monkeypatch, name, bases, c, groups, cases)
        for f in FORMS:
            assert got[f]["uniform"] == expected(name, pats["uniform"]), (groups, f)
            assert got[f]["all equal"] == expected(name, pats["all equal"]), (groups, f)
            assert got[f]["two rows"] == want_rows, (groups, f)


def test_a_shared_device_takes_the_throughput_form_and_a_lone_caller_does_not(gpu_lib, cref):
    """The rule itself, on the release build: 256 x 256 buckets (c = 17).  Three clones of one key called from three threads, a few calls
    each without waiting, find one another at work on the device; afterwards one context that calls and waits is alone.  No timing."""
    from reef_amd import msm
    name, c, n, calls = "pallas", 17, 4096, 4
    bases = cref.gen_bases_ap(CID[name], K0, D, n)
    ints = patterns(name, c, n, 17)["uniform"]
    want = expected(name, ints)
    sc = msm.DeviceBuffer.from_host(as_array(ints))
    with msm.MsmContext(name, bases, window_bits=c, bucket_groups=1) as ctx0:
        ctxs = [ctx0, ctx0.clone(), ctx0.clone()]
        outs = [[msm.DeviceBuffer(96) for _ in range(calls)] for _ in ctxs]
        gate = threading.Barrier(len(ctxs))
        errors = []

        def work(j):
            try:
                gate.wait()
                for k in range(calls):
                    ctxs[j].msm(sc, n, is_mont=False, out=outs[j][k])      # device result: the call returns with its work in flight
            except Exception as e:                                           # noqa: BLE001 -- reported by the main thread
                errors.append(e)
        th = [threading.Thread(target=work, args=(j,)) for j in range(len(ctxs))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors
        for cx in ctxs:
            cx.sync()
        for j in range(len(ctxs)):
            for k in range(calls):
                assert msm.compress(name, outs[j][k].to_host((1, 12))) == want, (j, k)
        shared = [cx.rowcol_forms() for cx in ctxs]
        assert sum(s["latency"] + s["throughput"] for s in shared) == calls * len(ctxs), shared
        assert sum(s["throughput"] for s in shared) >= 1, shared            # callers that found another at work took the throughput form
        for _ in range(2):                                                   # every context is idle now: one caller, who waits for the result
            assert msm.compress(name, ctx0.msm(sc, n, is_mont=False)) == want
        assert ctx0.rowcol_forms() == {"latency": 2, "throughput": 0}
        for cx in ctxs[1:]:
            cx.close()
