"""The batched IPA opening of the final SNARK on the GPU (reef_amd.spartan.Opening over include/reef_msm.h 3h) against the
big-integer reference of tests/test_spartan_open_host.py, bit-exact: the cross term, c, every L and R (compressed), a_hat and a, b
after every round, both curves, both input forms, on the shapes of tests/test_gpu_spartan.py that reach each padding direction; the
three key kinds; a device-folded instance end to end through the verifier; a 2^20 shape by the verifier alone; the NIFS state
afterwards; the order and argument errors."""
import random

import numpy as np
import pytest

from test_gpu_nifs import _set_running, _upload_shape
from test_gpu_spartan import _pads, _shape
from test_nifs_host import cross_term, fold, fresh_instance, from_arr, layered_shape, running_from_fresh, to_arr
from test_spartan_host import Challenger, eq_evals, next_pow2, prove_ref, relaxed_instance
from test_spartan_open_host import affine, compress, gens_of, msm, open_ref, verify_open

from oracle import pasta_ref

pytestmark = pytest.mark.gpu


def _instances(curve, shape, inst, pf, gens):
    """[E, W] as 3h batches them, from the reference prove pf: {comm, a, b, eval}"""
    p = shape["p"]
    e1, e2 = eq_evals(pf["r_x"], p), eq_evals(pf["r_y"][1:], p)
    E, W = list(inst["E"]), list(inst["W"])
    out = []
    for a, b in ((E, e1), (W, e2)):
        out.append({"a": a, "b": b, "comm": msm(curve, gens[:len(a)], a) if a else np.zeros(12, np.uint64),
                    "eval": sum(x * y for x, y in zip(a, b)) % p})
    return out


def _key(curve, gens, kind):
    from reef_amd.msm import MsmContext
    kw = {"pre": dict(bucket_groups=1, byte_tables=2), "tables": dict(bucket_groups=1, byte_tables=1), "plain": dict(bucket_groups=4)}[kind]
    key = MsmContext(curve, gens, **kw)
    assert key.has_byte_tables() == (kind == "tables")
    return key


def _run_steps(nf, key, ref, curve, p, is_mont, trace=True):
    """The opening call by call with the reference's challenges: every output against the reference"""
    from reef_amd.spartan import Opening
    R = (1 << 256) % p
    to = (lambda v: v * R % p) if is_mont else (lambda v: v)
    frm = (lambda v: v * pow(R, -1, p) % p) if is_mont else (lambda v: v)
    op = Opening(nf)
    form = "Montgomery" if is_mont else "canonical"
    assert frm(op.begin(key, is_mont=is_mont)) == ref["cross"], f"cross term ({form})"
    assert frm(op.fold(to(ref["r"]), is_mont=is_mont)) == ref["c"], f"c ({form})"
    L, Rp = op.ipa_begin(ref["q"])
    assert (compress(curve, L), compress(curve, Rp)) == (compress(curve, ref["L"][0]), compress(curve, ref["R"][0])), f"L, R round 0 ({form})"
    for k, r in enumerate(ref["rs"][:-1]):
        L, Rp = op.ipa_round(to(r), is_mont=is_mont)
        assert compress(curve, L) == compress(curve, ref["L"][k + 1]), f"L round {k + 1} ({form})"
        assert compress(curve, Rp) == compress(curve, ref["R"][k + 1]), f"R round {k + 1} ({form})"
        if trace and (k < 3 or k == len(ref["rs"]) - 2):
            t = ref["trace"][k]
            assert [frm(v) for v in op.read(0, len(t["a"]), to_mont=is_mont)] == t["a"], f"a after round {k} ({form})"
            assert [frm(v) for v in op.read(1, len(t["b"]), to_mont=is_mont)] == t["b"], f"b after round {k} ({form})"
    assert frm(op.finish(to(ref["rs"][-1]), is_mont=is_mont)) == ref["a_hat"], f"a_hat ({form})"
    assert op.read(1, 1) == [ref["b_hat"]]
    return op


def _open_shape(curve, name):
    """the shapes of tests/test_gpu_spartan.py, and two with num_cons_pad and num_vars_pad apart (both padding directions)"""
    if name == "cons_gt_vars":
        shape = layered_shape(curve, 100, num_inputs=3, num_io=2, empty_every=9, seed=40 + curve)
        return shape, (512, _pads(shape, None)[1])
    if name == "vars_gt_cons":
        shape = layered_shape(curve, 40, num_inputs=4, num_io=3, extra_vars=300, dup_every=4, seed=50 + curve)
        return shape, (64, 4 * _pads(shape, None)[1])
    return _shape(curve, name)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("name", ["smallest", "cons_gt_vars", "vars_gt_cons", "dup_empty", "cfg4"])
def test_opening_bit_exact_against_the_reference(gpu_lib, curve, name):
    from reef_amd.nifs import Nifs
    from reef_amd.spartan import prove
    shape, pads = _open_shape(curve, name)
    p, n = shape["p"], max(pads)
    inst = relaxed_instance(shape, 1, 11 + curve)
    gens, gens_s = gens_of(curve, n)
    ch = Challenger(p, curve)
    pf = prove_ref(shape, inst, pads[0], pads[1], ch)
    i1, i2 = _instances(curve, shape, inst, pf, gens)
    ref = open_ref(curve, gens, gens_s, i1, i2, ch)
    assert len(ref["L"]) == n.bit_length() - 1
    with _key(curve, gens, "pre") as key:
        for is_mont in (False, True):
            with Nifs(curve, shape["num_cons"], shape["num_vars"], shape["num_io"]) as nf:
                _upload_shape(nf, shape, is_mont)
                _set_running(nf, inst, p, is_mont)
                prove(nf, pads[0], pads[1], Challenger(p, curve), p, is_mont=is_mont)
                _run_steps(nf, key, ref, curve, p, is_mont, trace=n <= 4096 or not is_mont)


def test_padding_directions_are_both_covered():
    from test_spartan_host import check_pads
    for name, want in (("cons_gt_vars", "cons"), ("vars_gt_cons", "vars")):
        for curve in (0, 1):
            shape, (ncp, nvp) = _open_shape(curve, name)
            assert check_pads(shape, ncp, nvp)
            assert {"vars": nvp > ncp, "cons": ncp > nvp}[want] and shape["num_cons"] < ncp and shape["num_vars"] < nvp, (name, ncp, nvp)


@pytest.mark.parametrize("curve", [0, 1])
def test_key_kinds_give_the_same_proof(gpu_lib, curve):
    """The pre-shifted bucket key, byte tables and a plain key (host window combine): the blind term c q enters each route."""
    from reef_amd.nifs import Nifs
    from reef_amd.spartan import prove
    shape = layered_shape(curve, 1500, num_io=2, extra_vars=40, empty_every=7, seed=30 + curve)
    p = shape["p"]
    pads = _pads(shape, None)
    n = max(pads)
    assert n == 2048
    inst = relaxed_instance(shape, 1, 4)
    gens, gens_s = gens_of(curve, n)
    ch = Challenger(p, 2)
    pf = prove_ref(shape, inst, pads[0], pads[1], ch)
    i1, i2 = _instances(curve, shape, inst, pf, gens)
    ref = open_ref(curve, gens, gens_s, i1, i2, ch)
    with Nifs(curve, shape["num_cons"], shape["num_vars"], shape["num_io"]) as nf:
        _upload_shape(nf, shape, False)
        _set_running(nf, inst, p, False)
        for kind in ("pre", "tables", "plain"):
            with _key(curve, gens, kind) as key:
                prove(nf, pads[0], pads[1], Challenger(p, 2), p)
                _run_steps(nf, key, ref, curve, p, False, trace=False)


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
    pads = _pads(shape, None)
    n = max(pads)
    gens, gens_s = gens_of(curve, n)
    rng = random.Random(curve)
    run = running_from_fresh(fresh_instance(shape, 0), nc)
    with MsmContext(curve, pasta_ref.gen_bases_ap(curve, 42, 5, nc)) as tkey, _key(curve, gens, "pre") as key, \
            Nifs(curve, nc, shape["num_vars"], shape["num_io"]) as nf:
        _upload_shape(nf, shape, False)
        _set_running(nf, run, p, False, zero_e=True)
        for step in range(1, 4):
            fresh = fresh_instance(shape, step)
            nf.commit_t(tkey, to_arr(fresh["W"]), to_arr(fresh["X"]))
            r = rng.randrange(p)
            nf.fold(r)
            run = fold(run, fresh, cross_term(shape, run, fresh, p), r, p)
        e_dev, w_dev = from_arr(nf.read(E)), from_arr(nf.read(W))
        assert e_dev == run["E"] and w_dev == run["W"] and any(e_dev)
        comm_e, comm_w = msm(curve, gens[:nc], e_dev), msm(curve, gens[:len(w_dev)], w_dev)
        comm_a, q_of = _comm_ops(curve, comm_e, comm_w, gens_s)
        got = prove_with_opening(nf, key, pads[0], pads[1], Challenger(p, 7), p, comm_a, q_of)
        eval_e, eval_w = got["claims_outer"][3], got["claims_inner"][2]
        verify_open(curve, gens, gens_s, comm_e, eq_evals(got["r_x"], p), eval_e, comm_w, eq_evals(got["r_y"][1:], p), eval_w, _proof(got),
                    _replayed(p, 7, got))
        state = {"W": from_arr(nf.read(W)), "E": from_arr(nf.read(E)), "u": from_arr(nf.read(U))[0], "X": from_arr(nf.read(X))}
        assert state == run
        again = prove_with_opening(nf, key, pads[0], pads[1], Challenger(p, 7), p, comm_a, q_of)
        assert [compress(curve, x) for x in again["L"] + again["R"]] == [compress(curve, x) for x in got["L"] + got["R"]]
        assert (again["a_hat"], again["c"], again["cross_term"]) == (got["a_hat"], got["c"], got["cross_term"])
        fresh = fresh_instance(shape, 9)
        nf.commit_t(tkey, to_arr(fresh["W"]), to_arr(fresh["X"]))
        t = cross_term(shape, run, fresh, p)
        assert from_arr(nf.read(T)) == t
        nf.fold(12345)
        run = fold(run, fresh, t, 12345, p)
        assert from_arr(nf.read(W)) == run["W"] and from_arr(nf.read(E)) == run["E"]
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
    from test_nifs_host import matvec
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
    with _key(curve, gens, "pre") as key, Nifs(curve, nc, shape["num_vars"], shape["num_io"]) as nf:
        _upload_shape(nf, shape, False)
        _set_running(nf, inst, p, False)
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
    ncp, nvp = _pads(shape, None)
    n = max(ncp, nvp)
    gens, gens_s = gens_of(curve, n)
    q = affine(curve, pasta_ref.scalar_mul(curve, gens_s, 99))

    def arg_error(fn, *a, expect=None):
        with pytest.raises(ReefError) as e:
            fn(*a)
        assert e.value.status == 1, str(e.value)           # REEF_ERR_ARG
        if expect:
            assert expect in str(e.value), str(e.value)

    with Nifs(curve, nc, nv, nio) as nf, _key(curve, gens, "pre") as key, \
            MsmContext(curve, pasta_ref.gen_bases_ap(curve, 7, 3, 2 * n)) as long_key, \
            MsmContext(1 - curve, pasta_ref.gen_bases_ap(1 - curve, 7, 3, n)) as other_curve:
        op, sp = Opening(nf), Spartan(nf)
        _upload_shape(nf, shape, False)
        _set_running(nf, inst, p, False)
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
        w = from_arr(nf.read(W))
        _set_running(nf, inst, p, False)
        arg_error(op.ipa_begin, q, expect="reef_spartan_begin")
        arg_error(op.read, 0, 1, expect="reef_spartan_begin")
        assert from_arr(nf.read(W)) == w == inst["W"]
        if gpu_lib.reef_device_count() > 1:                                                  # a key on another device
            with MsmContext(curve, gens, device=1, bucket_groups=1) as far:
                prove(nf, ncp, nvp, Challenger(p, 1), p)
                arg_error(op.begin, far, expect="device")
