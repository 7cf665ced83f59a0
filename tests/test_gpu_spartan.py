"""Row N5 on the GPU: the sum-checks of the final SNARK (reef_amd.spartan over include/reef_msm.h 3g) against the big-integer
reference of oracle/spartan_oracle.py, bit-exact: every round's evaluations, every challenge and every claim, both curves, both
input forms, on shapes that reach each path (renumbered columns, empty rows, duplicates, a long row, a long column, cfg4's size);
a running instance folded on the device; a 2^20-row shape checked by the verifier's identities; the NIFS state left as it was;
the order and argument errors."""
import random

import pytest

from gpu_drivers import PROOF_KEYS, SPARTAN_SHAPES, ap_key, pads_of, prove_dev, set_running, spartan_shape, upload_shape
from oracle.r1cs_oracle import cross_term, fold, fresh_instance, layered_shape, matvec, relaxed_instance, running_from_fresh
from oracle.spartan_oracle import Challenger, next_pow2, prove_ref, verify
from reef_amd._fe import _arr, _ints

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("name", list(SPARTAN_SHAPES))
def test_prove_bit_exact_against_the_reference(gpu_lib, curve, name):
    from reef_amd.nifs import E, U, W, X, Nifs
    shape, pads = spartan_shape(curve, name)
    p = shape["p"]
    inst = relaxed_instance(shape, 1, 11 + curve)                   # u != 1, E != 0 (reference folds)
    ref = prove_ref(shape, inst, pads[0], pads[1], Challenger(p, curve))
    for is_mont in (False, True):
        with Nifs(curve, shape["num_cons"], shape["num_vars"], shape["num_io"]) as nf:
            upload_shape(nf, shape, is_mont)
            set_running(nf, inst, p, is_mont)
            got = prove_dev(nf, shape, pads, is_mont, curve)
            for k in PROOF_KEYS:
                assert got[k] == ref[k], f"{k} ({'Montgomery' if is_mont else 'canonical'} form)"
            assert _ints(nf.read(W)) == inst["W"] and _ints(nf.read(E)) == inst["E"]      # the running instance is untouched
            assert _ints(nf.read(U)) == [inst["u"]] and _ints(nf.read(X)) == inst["X"]
            assert nf.check_relaxed() == (0, None)


@pytest.mark.parametrize("curve", [0, 1])
def test_device_folded_instance_then_fold_after_the_prove(gpu_lib, curve):
    """Three device commit_T + fold steps make the running instance; the prove matches the reference on reference folds, leaves
    W, E, u, X as they were, and a NIFS step after it is still bit-exact."""
    from reef_amd.nifs import E, T, U, W, X, Nifs
    shape = layered_shape(curve, 3000, num_io=3, extra_vars=17, empty_every=23, dup_every=7, long_row=700, seed=60 + curve)
    p, n = shape["p"], shape["num_cons"]
    pads = pads_of(shape, None)
    rng = random.Random(curve)
    run = running_from_fresh(fresh_instance(shape, 0), n)
    _, key = ap_key(curve, n)
    with key, Nifs(curve, n, shape["num_vars"], shape["num_io"]) as nf:
        upload_shape(nf, shape, False)
        set_running(nf, run, p, False, zero_e=True)
        for step in range(1, 4):
            fresh = fresh_instance(shape, step)
            nf.commit_t(key, _arr(fresh["W"]), _arr(fresh["X"]))
            r = rng.randrange(p)
            nf.fold(r)
            run = fold(run, fresh, cross_term(shape, run, fresh, p), r, p)
        assert run["u"] != 1 and any(run["E"])
        ref = prove_ref(shape, run, pads[0], pads[1], Challenger(p, 7))
        got = prove_dev(nf, shape, pads, False, 7)
        for k in PROOF_KEYS:
            assert got[k] == ref[k], k
        got = {"W": _ints(nf.read(W)), "E": _ints(nf.read(E)), "u": _ints(nf.read(U))[0], "X": _ints(nf.read(X))}
        assert got == run
        fresh = fresh_instance(shape, 9)
        nf.commit_t(key, _arr(fresh["W"]), _arr(fresh["X"]))
        t = cross_term(shape, run, fresh, p)
        assert _ints(nf.read(T)) == t
        nf.fold(12345)
        run = fold(run, fresh, t, 12345, p)
        assert _ints(nf.read(W)) == run["W"] and _ints(nf.read(E)) == run["E"]
        assert nf.check_relaxed() == (0, None)
        # a second prove on the new running instance (the workspace is reused)
        assert prove_dev(nf, shape, pads, False, 8)["claims_inner"] == prove_ref(shape, run, pads[0], pads[1], Challenger(p, 8))["claims_inner"]


def test_2_20_rows_by_the_verifier_identities(gpu_lib):
    """cfg5's size (2^20 padded constraints): too slow for the reference prover in Python, so the verifier checks the transcript --
    chained round sums, claims evaluated straight from the shape, both final identities."""
    from reef_amd.nifs import Nifs
    curve = 0
    shape = layered_shape(curve, (1 << 20) - 3, num_inputs=64, num_io=2, extra_vars=3, long_row=20000, shuffle=False, seed=77)
    p, n = shape["p"], shape["num_cons"]
    inst = running_from_fresh(fresh_instance(shape, 1), n)
    inst["u"] = 5                                                     # relaxed: E makes up the difference row by row
    z = inst["W"] + [5] + inst["X"]
    az, bz, cz = (matvec(shape[m], z, n, p) for m in "ABC")
    inst["E"] = [(a * b - 5 * c) % p for a, b, c in zip(az, bz, cz)]
    pads = (1 << 20, next_pow2(shape["num_vars"]))
    with Nifs(curve, n, shape["num_vars"], shape["num_io"]) as nf:
        upload_shape(nf, shape, False)
        set_running(nf, inst, p, False)
        got = prove_dev(nf, shape, pads, False, 3)
    verify(shape, inst, pads[0], pads[1], got, Challenger(p, 3))


@pytest.mark.parametrize("curve", [0, 1])
def test_order_and_argument_errors(gpu_lib, curve):
    from reef_amd._ffi import ReefError
    from reef_amd.nifs import Nifs
    from reef_amd.spartan import Spartan
    shape = layered_shape(curve, 20, num_io=2, seed=5)
    p, n, nv, nio = shape["p"], shape["num_cons"], shape["num_vars"], shape["num_io"]
    inst = running_from_fresh(fresh_instance(shape, 1), n)
    ncp, nvp = pads_of(shape, None)
    ell_x, ell_y = ncp.bit_length() - 1, (2 * nvp).bit_length() - 1
    tau = list(range(3, 3 + ell_x))

    def arg_error(fn, *a, expect=None):
        with pytest.raises(ReefError) as e:
            fn(*a)
        assert e.value.status == 1, str(e.value)           # REEF_ERR_ARG
        if expect:
            assert expect in str(e.value), str(e.value)

    with Nifs(curve, n, nv, nio) as nf:
        sp = Spartan(nf)
        upload_shape(nf, shape, False)
        arg_error(sp.begin, ncp, nvp, tau)                                     # no running instance yet
        set_running(nf, inst, p, False)
        arg_error(sp.outer_round, 7, expect="reef_spartan_begin")              # a round before begin
        arg_error(sp.begin, ncp // 2, nvp, tau[:-1])                           # num_cons_pad < num_cons
        arg_error(sp.begin, ncp + 2, nvp, tau)                                 # not a power of two
        arg_error(sp.begin, ncp, nvp // 2, tau)                                # num_vars_pad < num_vars
        arg_error(sp.begin, 1 << 25, nvp, list(range(25)))                     # over 2^24
        arg_error(sp.begin, ncp, nvp, [p] + tau[1:])                           # tau not below the modulus
        with Nifs(curve, 4, 1, 2) as small:                                    # num_io >= num_vars_pad
            arg_error(Spartan(small).begin, 4, 2, [1, 2])
        sp.begin(ncp, nvp, tau)
        arg_error(sp.outer_claims, 5, expect="reef_spartan_outer_round")       # too few rounds
        arg_error(sp.inner_begin, 5, expect="reef_spartan_outer_round")
        for k in range(ell_x - 1):
            sp.outer_round(11 + k)
        arg_error(sp.outer_round, 5, expect="reef_spartan_outer_claims")       # one round too many
        sp.outer_claims(9)
        arg_error(sp.outer_claims, 9, expect="reef_spartan_inner_begin")
        sp.inner_begin(4)
        for k in range(ell_y - 1):
            sp.inner_round(20 + k)
        arg_error(sp.inner_round, 5, expect="reef_spartan_inner_claims")
        sp.inner_claims(3)
        arg_error(sp.inner_round, 5, expect="reef_spartan_begin")              # nothing after the claims
        # the NIFS calls void a prove in progress
        sp.begin(ncp, nvp, tau)
        set_running(nf, inst, p, False)
        arg_error(sp.outer_round, 5, expect="reef_spartan_begin")
        arg_error(sp.outer_round, 5, expect="reef_spartan_begin")
        _, key = ap_key(curve, n)
        with key:
            for undo in ("commit", "fold"):
                sp.begin(ncp, nvp, tau)
                fresh = fresh_instance(shape, 2)
                nf.commit_t(key, _arr(fresh["W"]), _arr(fresh["X"]))
                if undo == "fold":
                    sp.begin(ncp, nvp, tau)
                    nf.fold(3)
                    inst = fold(inst, fresh, cross_term(shape, inst, fresh, p), 3, p)
                arg_error(sp.outer_round, 5, expect="reef_spartan_begin")
        sp.begin(ncp, nvp, tau)
        r = list(range(40, 40 + ell_x))
        arg_error(sp.outer_round, p)                                           # a challenge not below the modulus, refused ...
        for k in range(ell_x - 1):
            sp.outer_round(r[k])                                               # ... and the prove goes on
        # the ctx is still usable: a whole prove matches the reference
        pads = (ncp, nvp)
        ref = prove_ref(shape, inst, ncp, nvp, Challenger(p, 1))
        got = prove_dev(nf, shape, pads, False, 1)
        for k in PROOF_KEYS:
            assert got[k] == ref[k], k
