"""The batched IPA opening of the final SNARK on the GPU (reef_amd.spartan.Opening over include/reef_msm.h 3h) against the
big-integer reference of oracle/ipa_oracle.py, bit-exact: the cross term, c, every L and R (compressed), a_hat and a, b
after every round, both curves, both input forms, on the Spartan shapes of tests/gpu_drivers.py that reach each padding direction; the
three key kinds; a device-folded instance end to end through the verifier; a 2^20 shape by the verifier alone; the NIFS state
afterwards; the order and argument errors."""
import random

import numpy as np
import pytest

from gpu_drivers import key_of_kind, open_shape, opening_instances, pads_of, run_opening, set_running, upload_shape
from oracle import pasta_ref
from oracle.ipa_oracle import affine, compress, gens_of, msm, open_ref, verify_open
from oracle.r1cs_oracle import cross_term, fold, fresh_instance, layered_shape, matvec, relaxed_instance, running_from_fresh
from oracle.spartan_oracle import Challenger, check_pads, eq_evals, next_pow2, prove_ref
from reef_amd._fe import _arr, _ints

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("name", ["smallest", "cons_gt_vars", "vars_gt_cons", "dup_empty", "cfg4"])
def test_opening_bit_exact_against_the_reference(gpu_lib, curve, name):
    from reef_amd.nifs import Nifs
    from reef_amd.spartan import prove
    shape, pads = open_shape(curve, name)
    p, n = shape["p"], max(pads)
    inst = relaxed_instance(shape, 1, 11 + curve)
    gens, gens_s = gens_of(curve, n)
    ch = Challenger(p, curve)
    pf = prove_ref(shape, inst, pads[0], pads[1], ch)
    i1, i2 = opening_instances(curve, shape, inst, pf, gens)
    ref = open_ref(curve, gens, gens_s, i1, i2, ch)
    assert len(ref["L"]) == n.bit_length() - 1
    with key_of_kind(curve, gens, "pre") as key:
        for is_mont in (False, True):
            with Nifs(curve, shape["num_cons"], shape["num_vars"], shape["num_io"]) as nf:
                upload_shape(nf, shape, is_mont)
                set_running(nf, inst, p, is_mont)
                prove(nf, pads[0], pads[1], Challenger(p, curve), p, is_mont=is_mont)
                run_opening(nf, key, ref, curve, p, is_mont, trace=n <= 4096 or not is_mont)


def test_padding_directions_are_both_covered():
    for name, want in (("cons_gt_vars", "cons"), ("vars_gt_cons", "vars")):
        for curve in (0, 1):
            shape, (ncp, nvp) = open_shape(curve, name)
            assert check_pads(shape, ncp, nvp)
            assert {"vars": nvp > ncp, "cons": ncp > nvp}[want] and shape["num_cons"] < ncp and shape["num_vars"] < nvp, (name, ncp, nvp)


@pytest.mark.parametrize("curve", [0, 1])
def test_key_kinds_give_the_same_proof(gpu_lib, curve):
    """The pre-shifted bucket key, byte tables and a plain key (host window combine): the blind term c q enters each route."""
    from reef_amd.nifs import Nifs
    from reef_amd.spartan import prove
    shape = layered_shape(curve, 1500, num_io=2, extra_vars=40, empty_every=7, seed=30 + curve)
    p = shape["p"]
    pads = pads_of(shape, None)
    n = max(pads)
    assert n == 2048
    inst = relaxed_instance(shape, 1, 4)
    gens, gens_s = gens_of(curve, n)
    ch = Challenger(p, 2)
    pf = prove_ref(shape, inst, pads[0], pads[1], ch)
    i1, i2 = opening_instances(curve, shape, inst, pf, gens)
    ref = open_ref(curve, gens, gens_s, i1, i2, ch)
    with Nifs(curve, shape["num_cons"], shape["num_vars"], shape["num_io"]) as nf:
        upload_shape(nf, shape, False)
        set_running(nf, inst, p, False)
        for kind in ("pre", "tables", "plain"):
            with key_of_kind(curve, gens, kind) as key:
                prove(nf, pads[0], pads[1], Challenger(p, 2), p)
                run_opening(nf, key, ref, curve, p, False, trace=False)


def _comm_ops(curve, comm_e, comm_w, gens_s):
    def comm_a(r):
        return compress(curve, msm(curve, np.stack([comm_e, comm_w]), [1, r]))

    def q_of(r):
        return affine(curve, pasta_ref.scalar_mul(curve, gens_s, r))
    return comm_a, q_of


@pytest.mark.parametrize("curve", [0, 1])
def test_device_folded_instance_end_to_end_and_state_afterwards(gpu_lib, curve):
    """Three device folding steps, then 3g and 3h through prove_with_opening; the verifier accepts against comm_E, comm_W taken from
    reef_nifs_read.  W, E, u, X are untouched, commit_T and fold still work, and a second prove gives the same bytes."""
    from reef_amd.msm import MsmContext
    from reef_amd.nifs import E, T, U, W, X, Nifs
    from reef_amd.spartan import prove_with_opening
    shape = layered_shape(curve, 3000, num_io=3, extra_vars=17, empty_every=23, dup_every=7, long_row=700, seed=60 + curve)
    p, nc = shape["p"], shape["num_cons"]
    pads = pads_of(shape, None)
    n = max(pads)
    gens, gens_s = gens_of(curve, n)
    rng = random.Random(curve)
    run = running_from_fresh(fresh_instance(shape, 0), nc)
    with MsmContext(curve, pasta_ref.gen_bases_ap(curve, 42, 5, nc)) as tkey, key_of_kind(curve, gens, "pre") as key, \
            Nifs(curve, nc, shape["num_vars"], shape["num_io"]) as nf:
        upload_shape(nf, shape, False)
        set_running(nf, run, p, False, zero_e=True)
        for step in range(1, 4):
            fresh = fresh_instance(shape, step)
            nf.commit_t(tkey, _arr(fresh["W"]), _arr(fresh["X"]))
            r = rng.randrange(p)
            nf.fold(r)
            run = fold(run, fresh, cross_term(shape, run, fresh, p), r, p)
        e_dev, w_dev = _ints(nf.read(E)), _ints(nf.read(W))
        assert e_dev == run["E"] and w_dev == run["W"] and any(e_dev)
        comm_e, comm_w = msm(curve, gens[:nc], e_dev), msm(curve, gens[:len(w_dev)], w_dev)
        comm_a, q_of = _comm_ops(curve, comm_e, comm_w, gens_s)
        got = prove_with_opening(nf, key, pads[0], pads[1], Challenger(p, 7), p, comm_a, q_of)
        eval_e, eval_w = got["claims_outer"][3], got["claims_inner"][2]
        verify_open(curve, gens, gens_s, comm_e, eq_evals(got["r_x"], p), eval_e, comm_w, eq_evals(got["r_y"][1:], p), eval_w, _proof(got),
                    _replayed(p, 7, got))
        state = {"W": _ints(nf.read(W)), "E": _ints(nf.read(E)), "u": _ints(nf.read(U))[0], "X": _ints(nf.read(X))}
        assert state == run
        again = prove_with_opening(nf, key, pads[0], pads[1], Challenger(p, 7), p, comm_a, q_of)
        assert [compress(curve, x) for x in again["L"] + again["R"]] == [compress(curve, x) for x in got["L"] + got["R"]]
        assert (again["a_hat"], again["c"], again["cross_term"]) == (got["a_hat"], got["c"], got["cross_term"])
        fresh = fresh_instance(shape, 9)
        nf.commit_t(tkey, _arr(fresh["W"]), _arr(fresh["X"]))
        t = cross_term(shape, run, fresh, p)
        assert _ints(nf.read(T)) == t
        nf.fold(12345)
        run = fold(run, fresh, t, 12345, p)
        assert _ints(nf.read(W)) == run["W"] and _ints(nf.read(E)) == run["E"]
        assert nf.check_relaxed() == (0, None)


def _proof(got):
    """what the verifier receives of prove_with_opening's result"""
    return {"cross": got["cross_term"], "L": got["L"], "R": got["R"], "a_hat": got["a_hat"]}


def _replayed(p, seed, got):
    """A Challenger in the state the verifier of the opening starts from: the sum-checks' challenges re-drawn in order"""
    ch = Challenger(p, seed)
    for _ in got["tau"]:
        ch("t", [])
    for ev in got["outer"]:
        ch("outer", ev)
    ch("r", got["claims_outer"])
    for ev in got["inner"]:
        ch("inner", ev)
    return ch


def test_2_20_shape_by_the_verifier(gpu_lib):
    """cfg5's size: the opening at n = 2^20 checked by the verifier alone (no reference prover)."""
    from reef_amd.nifs import Nifs
    from reef_amd.spartan import prove_with_opening
    curve = 0
    shape = layered_shape(curve, (1 << 20) - 3, num_inputs=64, num_io=2, extra_vars=3, long_row=20000, shuffle=False, seed=77)
    p, nc = shape["p"], shape["num_cons"]
    inst = running_from_fresh(fresh_instance(shape, 1), nc)
    inst["u"] = 5
    z = inst["W"] + [5] + inst["X"]
    az, bz, cz = (matvec(shape[m], z, nc, p) for m in "ABC")
    inst["E"] = [(a * b - 5 * c) % p for a, b, c in zip(az, bz, cz)]
    pads = (1 << 20, next_pow2(shape["num_vars"]))
    n = max(pads)
    gens, gens_s = gens_of(curve, n)
    comm_e, comm_w = msm(curve, gens[:nc], inst["E"]), msm(curve, gens[:len(inst["W"])], inst["W"])
    comm_a, q_of = _comm_ops(curve, comm_e, comm_w, gens_s)
    with key_of_kind(curve, gens, "pre") as key, Nifs(curve, nc, shape["num_vars"], shape["num_io"]) as nf:
        upload_shape(nf, shape, False)
        set_running(nf, inst, p, False)
        got = prove_with_opening(nf, key, pads[0], pads[1], Challenger(p, 3), p, comm_a, q_of)
    verify_open(curve, gens, gens_s, comm_e, eq_evals(got["r_x"], p), got["claims_outer"][3], comm_w, eq_evals(got["r_y"][1:], p),
                got["claims_inner"][2], _proof(got), _replayed(p, 3, got))


@pytest.mark.parametrize("curve", [0, 1])
def test_order_and_argument_errors(gpu_lib, curve):
    from reef_amd._ffi import ReefError
    from reef_amd.msm import MsmContext
    from reef_amd.nifs import W, Nifs
    from reef_amd.spartan import Opening, Spartan, prove
    shape = layered_shape(curve, 20, num_io=2, seed=5)
    p, nc, nv, nio = shape["p"], shape["num_cons"], shape["num_vars"], shape["num_io"]
    inst = running_from_fresh(fresh_instance(shape, 1), nc)
    ncp, nvp = pads_of(shape, None)
    n = max(ncp, nvp)
    gens, gens_s = gens_of(curve, n)
    q = affine(curve, pasta_ref.scalar_mul(curve, gens_s, 99))

    def arg_error(fn, *a, expect=None):
        with pytest.raises(ReefError) as e:
            fn(*a)
        assert e.value.status == 1, str(e.value)           # REEF_ERR_ARG
        if expect:
            assert expect in str(e.value), str(e.value)

    with Nifs(curve, nc, nv, nio) as nf, key_of_kind(curve, gens, "pre") as key, \
            MsmContext(curve, pasta_ref.gen_bases_ap(curve, 7, 3, 2 * n)) as long_key, \
            MsmContext(1 - curve, pasta_ref.gen_bases_ap(1 - curve, 7, 3, n)) as other_curve:
        op, sp = Opening(nf), Spartan(nf)
        upload_shape(nf, shape, False)
        set_running(nf, inst, p, False)
        arg_error(op.begin, key, expect="reef_spartan_begin")                              # before any prove
        sp.begin(ncp, nvp, list(range(3, 3 + ncp.bit_length() - 1)))
        arg_error(op.begin, key, expect="reef_spartan_outer_round")                        # before inner_claims
        prove(nf, ncp, nvp, Challenger(p, 1), p)
        arg_error(op.fold, 5, expect="reef_spartan_open_begin")
        arg_error(op.ipa_round, 5, expect="reef_spartan_open_begin")                      # a round before the fold
        arg_error(op.read, 0, 1, expect="reef_spartan_open_begin")
        arg_error(op.begin, long_key, expect=f"{2 * n}")                                   # wrong length: both sizes named
        with pytest.raises(ReefError, match=f"= {n}"):
            op.begin(long_key)
        arg_error(op.begin, other_curve, expect="curve")
        cross = op.begin(key)
        arg_error(op.ipa_begin, q, expect="reef_spartan_open_fold")
        arg_error(op.fold, p, expect="modulus")                                            # a challenge not below the modulus ...
        c = op.fold(5)                                                                     # ... refused, and the opening goes on
        arg_error(op.ipa_round, 5, expect="reef_spartan_open_ipa_begin")
        op.ipa_begin(q)
        arg_error(op.ipa_round, 0, expect="zero")
        for k in range(n.bit_length() - 2):
            op.ipa_round(11 + k)
        arg_error(op.ipa_round, 5, expect="reef_spartan_open_finish")                     # one round too many
        arg_error(op.read, 0, 3, expect="has 2")
        a_hat = op.finish(7)
        arg_error(op.finish, 7, expect="reef_spartan_begin")
        # the same opening again gives the same values; then a NIFS call voids an opening in progress
        assert op.begin(key) == cross and op.fold(5) == c
        op.ipa_begin(q)
        for k in range(n.bit_length() - 2):
            op.ipa_round(11 + k)
        assert op.finish(7) == a_hat
        op.begin(key)
        op.fold(5)
        w = _ints(nf.read(W))
        set_running(nf, inst, p, False)
        arg_error(op.ipa_begin, q, expect="reef_spartan_begin")
        arg_error(op.read, 0, 1, expect="reef_spartan_begin")
        assert _ints(nf.read(W)) == w == inst["W"]
        if gpu_lib.reef_device_count() > 1:                                                  # a key on another device
            with MsmContext(curve, gens, device=1, bucket_groups=1) as far:
                prove(nf, ncp, nvp, Challenger(p, 1), p)
                arg_error(op.begin, far, expect="device")
