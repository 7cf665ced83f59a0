"""Row N5 on the GPU: the sum-checks of the final SNARK (reef_amd.spartan over include/reef_msm.h 3g) against the big-integer
reference of tests/test_spartan_host.py, bit-exact: every round's evaluations, every challenge and every claim, both curves, both
input forms, on shapes that reach each path (renumbered columns, empty rows, duplicates, a long row, a long column, cfg4's size);
a running instance folded on the device; a 2^20-row shape checked by the verifier's identities; the NIFS state left as it was;
the order and argument errors."""
import random

import pytest

from test_gpu_nifs import _key, _set_running, _upload_shape
from test_nifs_host import cross_term, fold, fresh_instance, from_arr, layered_shape, running_from_fresh, to_arr
from test_spartan_host import Challenger, next_pow2, prove_ref, relaxed_instance, verify

pytestmark = pytest.mark.gpu


def with_long_column(shape, col: int, seed: int) -> dict:
    """Adds to B, in every row, the pair (row, col, v), (row, col, -v): a column of 2 num_cons entries that sums to nothing."""
    p, rng = shape["p"], random.Random(seed)
    r, c, v = (list(x) for x in shape["B"])
    for i in range(shape["num_cons"]):
        x = rng.randrange(p)
        r += [i, i]
        c += [col, col]
        v += [x, (p - x) % p]
    return dict(shape, B=(r, c, v))


def _pads(shape, pads):
    return pads or (next_pow2(shape["num_cons"]), next_pow2(max(shape["num_vars"], shape["num_io"] + 1)))


SHAPES = {   # name: (layered_shape keyword arguments, (num_cons_pad, num_vars_pad) or None: the smallest legal)
    "smallest": (dict(num_cons=1, num_inputs=1, num_io=1), (2, 2)),
    "dup_empty": (dict(num_cons=127, dup_every=3, empty_every=5, extra_vars=4), None),
    "long_row": (dict(num_cons=300, long_row=1500, num_io=2), None),
    "vars_lt_cons": (dict(num_cons=500, num_inputs=3, empty_every=2, num_io=3), (512, 512)),      # u moves; num_vars_pad > num_vars
    "io_close": (dict(num_cons=100, num_inputs=4, num_io=120), None),                            # num_io = num_vars_pad - 8
    "cfg4": (dict(num_cons=39484, long_row=1100, empty_every=101, dup_every=13), (1 << 16, None)),
}


def _shape(curve, name):
    kw, pads = SHAPES[name]
    shape = layered_shape(curve, seed=len(name) + curve, **kw)
    if name == "cfg4":
        shape = with_long_column(shape, shape["num_vars"], 3)        # the u column: 2 x 39484 entries more
        pads = (pads[0], next_pow2(shape["num_vars"]))
    return shape, _pads(shape, pads)


def _prove_dev(nf, shape, pads, is_mont, seed):
    from reef_amd.spartan import prove
    return prove(nf, pads[0], pads[1], Challenger(shape["p"], seed), shape["p"], is_mont=is_mont)


KEYS = ("tau", "outer", "r_x", "claims_outer", "r", "inner", "r_y", "claims_inner")


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_prove_bit_exact_against_the_reference(gpu_lib, curve, name):
    from reef_amd.nifs import E, U, W, X, Nifs
    shape, pads = _shape(curve, name)
    p = shape["p"]
    inst = relaxed_instance(shape, 1, 11 + curve)                   # u != 1, E != 0 (reference folds)
    ref = prove_ref(shape, inst, pads[0], pads[1], Challenger(p, curve))
    for is_mont in (False, True):
        with Nifs(curve, shape["num_cons"], shape["num_vars"], shape["num_io"]) as nf:
            _upload_shape(nf, shape, is_mont)
            _set_running(nf, inst, p, is_mont)
            got = _prove_dev(nf, shape, pads, is_mont, curve)
            for k in KEYS:
                assert got[k] == ref[k], f"{k} ({'Montgomery' if is_mont else 'canonical'} form)"
            assert from_arr(nf.read(W)) == inst["W"] and from_arr(nf.read(E)) == inst["E"]      # the running instance is untouched
            assert from_arr(nf.read(U)) == [inst["u"]] and from_arr(nf.read(X)) == inst["X"]
            assert nf.check_relaxed() == (0, None)


@pytest.mark.parametrize("curve", [0, 1])
def test_device_folded_instance_then_fold_after_the_prove(gpu_lib, curve):
    """Three device commit_T + fold steps make the running instance; the prove matches the reference on reference folds, leaves
    W, E, u, X as they were, and a NIFS step after it is still bit-exact."""
    from reef_amd.nifs import E, T, U, W, X, Nifs
    shape = layered_shape(curve, 3000, num_io=3, extra_vars=17, empty_every=23, dup_every=7, long_row=700, seed=60 + curve)
    p, n = shape["p"], shape["num_cons"]
    pads = _pads(shape, None)
    rng = random.Random(curve)
    run = running_from_fresh(fresh_instance(shape, 0), n)
    _, key = _key(curve, n)
    with key, Nifs(curve, n, shape["num_vars"], shape["num_io"]) as nf:
        _upload_shape(nf, shape, False)
        _set_running(nf, run, p, False, zero_e=True)
        for step in range(1, 4):
            fresh = fresh_instance(shape, step)
            nf.commit_t(key, to_arr(fresh["W"]), to_arr(fresh["X"]))
            r = rng.randrange(p)
            nf.fold(r)
            run = fold(run, fresh, cross_term(shape, run, fresh, p), r, p)
        assert run["u"] != 1 and any(run["E"])
        ref = prove_ref(shape, run, pads[0], pads[1], Challenger(p, 7))
        got = _prove_dev(nf, shape, pads, False, 7)
        for k in KEYS:
            assert got[k] == ref[k], k
        got = {"W": from_arr(nf.read(W)), "E": from_arr(nf.read(E)), "u": from_arr(nf.read(U))[0], "X": from_arr(nf.read(X))}
        assert got == run
        fresh = fresh_instance(shape, 9)
        nf.commit_t(key, to_arr(fresh["W"]), to_arr(fresh["X"]))
        t = cross_term(shape, run, fresh, p)
        assert from_arr(nf.read(T)) == t
        nf.fold(12345)
        run = fold(run, fresh, t, 12345, p)
        assert from_arr(nf.read(W)) == run["W"] and from_arr(nf.read(E)) == run["E"]
        assert nf.check_relaxed() == (0, None)
        # a second prove on the new running instance (the workspace is reused)
        assert _prove_dev(nf, shape, pads, False, 8)["claims_inner"] == prove_ref(shape, run, pads[0], pads[1], Challenger(p, 8))["claims_inner"]


def test_2_20_rows_by_the_verifier_identities(gpu_lib):
    """cfg5's size (2^20 padded constraints): too slow for the reference prover in Python, so the verifier checks the transcript --
    chained round sums, claims evaluated straight from the shape, both final identities."""
    from reef_amd.nifs import Nifs
    curve = 0
    shape = layered_shape(curve, (1 << 20) - 3, num_inputs=64, num_io=2, extra_vars=3, long_row=20000, shuffle=False, seed=77)
    p, n = shape["p"], shape["num_cons"]
    inst = running_from_fresh(fresh_instance(shape, 1), n)
    inst["u"] = 5                                                     # relaxed: E makes up the difference row by row
    from test_nifs_host import matvec
    z = inst["W"] + [5] + inst["X"]
    az, bz, cz = (matvec(shape[m], z, n, p) for m in "ABC")
    inst["E"] = [(a * b - 5 * c) % p for a, b, c in zip(az, bz, cz)]
    pads = (1 << 20, next_pow2(shape["num_vars"]))
    with Nifs(curve, n, shape["num_vars"], shape["num_io"]) as nf:
        _upload_shape(nf, shape, False)
        _set_running(nf, inst, p, False)
        got = _prove_dev(nf, shape, pads, False, 3)
    verify(shape, inst, pads[0], pads[1], got, Challenger(p, 3))


@pytest.mark.parametrize("curve", [0, 1])
def test_order_and_argument_errors(gpu_lib, curve):
    from reef_amd._ffi import ReefError
    from reef_amd.nifs import Nifs
    from reef_amd.spartan import Spartan
    shape = layered_shape(curve, 20, num_io=2, seed=5)
    p, n, nv, nio = shape["p"], shape["num_cons"], shape["num_vars"], shape["num_io"]
    inst = running_from_fresh(fresh_instance(shape, 1), n)
    ncp, nvp = _pads(shape, None)
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
        _upload_shape(nf, shape, False)
        arg_error(sp.begin, ncp, nvp, tau)                                     # no running instance yet
        _set_running(nf, inst, p, False)
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
        _set_running(nf, inst, p, False)
        arg_error(sp.outer_round, 5, expect="reef_spartan_begin")
        arg_error(sp.outer_round, 5, expect="reef_spartan_begin")
        _, key = _key(curve, n)
        with key:
            for undo in ("commit", "fold"):
                sp.begin(ncp, nvp, tau)
                fresh = fresh_instance(shape, 2)
                nf.commit_t(key, to_arr(fresh["W"]), to_arr(fresh["X"]))
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
        got = _prove_dev(nf, shape, pads, False, 1)
        for k in KEYS:
            assert got[k] == ref[k], k
