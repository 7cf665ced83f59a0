"""Row N6 on the GPU: the NIFS step (reef_amd.nifs over include/reef_msm.h 3f) against the big-integer reference of
oracle/r1cs_oracle.py, bit-exact: T for canonical and Montgomery inputs, comm_T against oracle/pasta_ref's MSM of the
reference T, the four folds, a chain of folding steps under the relaxed-R1CS check, a shape of cfg5's size, argument errors."""
import random
import time

import numpy as np
import pytest

from gpu_drivers import ap_key, arr, set_running, upload_shape
from oracle import pasta_ref as R
from oracle.r1cs_oracle import bad_rows, cross_term, fold, fresh_instance, layered_shape, running_from_fresh, to_mont
from reef_amd._fe import _arr, _ints

pytestmark = pytest.mark.gpu


def _relaxed_running(shape, seed):
    """A running instance with u != 1 and E != 0: one reference fold of two fresh instances."""
    p, n = shape["p"], shape["num_cons"]
    run = running_from_fresh(fresh_instance(shape, seed), n)
    fresh = fresh_instance(shape, seed + 1000)
    return fold(run, fresh, cross_term(shape, run, fresh, p), random.Random(seed).randrange(p), p)


SHAPES = {   # name: layered_shape keyword arguments
    "1": dict(num_cons=1, num_inputs=2, num_io=1),
    "127_dup": dict(num_cons=127, dup_every=3, extra_vars=4),
    "4096_empty_long": dict(num_cons=4096, empty_every=9, long_row=(1 << 14) + 3, dup_every=11),
    "11376": dict(num_cons=11376, extra_vars=1000, num_io=4),
    "39484_long": dict(num_cons=39484, long_row=(1 << 14) + 77, empty_every=101, dup_every=13),
}


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_cross_term_commitment_and_fold_bit_exact(gpu_lib, curve, name):
    from reef_amd.msm import compress
    from reef_amd.nifs import E, T, U, W, X, Nifs
    shape = layered_shape(curve, seed=len(name) + curve, **SHAPES[name])
    p, n = shape["p"], shape["num_cons"]
    run = _relaxed_running(shape, 7)
    fresh = fresh_instance(shape, 8)
    t_ref = cross_term(shape, run, fresh, p)
    r = random.Random(name).randrange(p)
    ref = fold(run, fresh, t_ref, r, p)
    bases, key = ap_key(curve, n)
    with key:
        for is_mont in (False, True):
            with Nifs(curve, n, shape["num_vars"], shape["num_io"]) as nf:
                upload_shape(nf, shape, is_mont)
                set_running(nf, run, p, is_mont)
                comm = nf.commit_t(key, arr(fresh["W"], p, is_mont), arr(fresh["X"], p, is_mont), is_mont=is_mont)
                assert _ints(nf.read(T)) == t_ref, f"T ({'Montgomery' if is_mont else 'canonical'} inputs)"
                if not is_mont:
                    exp = R.compress(curve, R.msm_pippenger(curve, bases, _arr(t_ref), mont=False, threads=4))
                    assert compress(curve, comm) == exp, "comm_T"
                nf.fold(to_mont([r], p)[0] if is_mont else r, is_mont=is_mont)
                assert _ints(nf.read(W)) == ref["W"]
                assert _ints(nf.read(E)) == ref["E"]
                assert _ints(nf.read(U)) == [ref["u"]]
                assert _ints(nf.read(X)) == ref["X"]
                assert _ints(nf.read(E, to_mont=True)) == to_mont(ref["E"], p)
                assert nf.check_relaxed() == (0, None)


@pytest.mark.parametrize("curve", [0, 1])
def test_chain_of_folding_steps_stays_satisfied_and_tampering_is_reported(gpu_lib, curve):
    from reef_amd.nifs import E, T, U, W, X, Nifs
    shape = layered_shape(curve, 3000, num_io=3, extra_vars=17, empty_every=23, dup_every=7, long_row=700, seed=40 + curve)
    p, n = shape["p"], shape["num_cons"]
    rng = random.Random(curve)
    run = running_from_fresh(fresh_instance(shape, 0), n)
    _, key = ap_key(curve, n)
    with key, Nifs(curve, n, shape["num_vars"], shape["num_io"]) as nf:
        upload_shape(nf, shape, False)
        set_running(nf, run, p, False, zero_e=True)                 # nova's first step: E = 0, u = 1
        assert nf.check_relaxed() == (0, None)
        for step in range(1, 10):
            fresh = fresh_instance(shape, step)
            nf.commit_t(key, _arr(fresh["W"]), _arr(fresh["X"]))
            t = cross_term(shape, run, fresh, p)
            assert _ints(nf.read(T)) == t, f"T of step {step}"
            r = rng.randrange(p)
            nf.fold(r)
            run = fold(run, fresh, t, r, p)
            assert nf.check_relaxed() == (0, None), f"step {step}"
        got = {"W": _ints(nf.read(W)), "E": _ints(nf.read(E)), "u": _ints(nf.read(U))[0], "X": _ints(nf.read(X))}
        assert got == run
        assert bad_rows(shape, got, p) == []                          # the Python check agrees
        rows = [i for i in range(n) if shape["plan"][i] is not None]
        for k in (rows[0], rows[len(rows) // 2], rows[-1]):
            bad = dict(run, E=list(run["E"]))
            bad["E"][k] = (bad["E"][k] + 1) % p
            set_running(nf, bad, p, False)
            assert nf.check_relaxed() == (1, k)
            assert bad_rows(shape, bad, p) == [k]
        bad = dict(run, E=list(run["E"]))
        for k in rows[5:12]:
            bad["E"][k] = (bad["E"][k] + 3) % p
        set_running(nf, bad, p, False)
        assert nf.check_relaxed() == (7, rows[5])


def _row_dot(terms, z, p):
    return sum(v * z[c] for c, v in terms) % p


@pytest.mark.parametrize("curve", [0, 1])
def test_cfg5_sized_shape_three_folds_and_sampled_rows(gpu_lib, curve):
    """A 2^20-row shape (cfg5: 1 032 421 constraints): the relaxed check after three folds on the device, and 256 sampled rows of
    each step's T against the reference row by row."""
    from reef_amd.nifs import T, Nifs
    t0 = time.time()
    n = 1 << 20
    shape = layered_shape(curve, n, num_inputs=64, num_io=2, extra_vars=3, long_row=20000, shuffle=False, seed=77 + curve)
    p = shape["p"]
    fresh = [fresh_instance(shape, s) for s in (1, 2)]
    assert time.time() - t0 < 90, "generation over budget"
    rng = random.Random(5)
    sample = sorted(rng.sample(range(n), 255) + [n // 2])             # the long row among them
    run = running_from_fresh(fresh[0], n)
    z1 = run["W"] + [1] + run["X"]
    _, key = ap_key(curve, n)
    with key, Nifs(curve, n, shape["num_vars"], shape["num_io"]) as nf:
        upload_shape(nf, shape, False)
        set_running(nf, run, p, False, zero_e=True)
        e_rows = {i: 0 for i in sample}
        for step in range(3):
            fr = fresh[1 - step % 2] if step < 2 else fresh[1]
            z2 = fr["W"] + [1] + fr["X"]
            nf.commit_t(key, _arr(fr["W"]), _arr(fr["X"]))
            t = _ints(nf.read(T))
            u1 = z1[shape["num_vars"]]
            for i in sample:
                ta, tb, tc, cinv, out = shape["plan"][i]
                tcc = tc + [(out, pow(cinv, -1, p))]
                a1, b1, c1 = (_row_dot(x, z1, p) for x in (ta, tb, tcc))
                a2, b2, c2 = (_row_dot(x, z2, p) for x in (ta, tb, tcc))
                assert t[i] == (a1 * b2 + a2 * b1 - u1 * c2 - c1) % p, f"T[{i}] of step {step}"
            r = rng.randrange(p)
            nf.fold(r)
            z1 = [(a + r * b) % p for a, b in zip(z1, z2)]
            assert nf.check_relaxed() == (0, None), f"after fold {step + 1}"


@pytest.mark.parametrize("curve", [0, 1])
def test_argument_errors(gpu_lib, curve):
    from reef_amd._ffi import ReefError
    from reef_amd.nifs import Nifs
    shape = layered_shape(curve, 64, seed=3)
    p, n, nv, nio = shape["p"], shape["num_cons"], shape["num_vars"], shape["num_io"]
    fresh = fresh_instance(shape, 1)
    with Nifs(curve, n, nv, nio) as nf:
        def arg_error(fn, *a, **k):
            with pytest.raises(ReefError) as e:
                fn(*a, **k)
            assert e.value.status == 1          # REEF_ERR_ARG
        one = _arr([1])
        arg_error(nf.set_matrix, 0, [0], [nv + 1 + nio], one)           # column out of range
        arg_error(nf.set_matrix, 0, [n], [0], one)                      # row out of range
        arg_error(nf.set_matrix, 3, [0], [0], one)                      # no matrix D
        upload_shape(nf, shape, False)
        set_running(nf, running_from_fresh(fresh, n), p, False, zero_e=True)
        arg_error(nf.fold, 5)                                           # fold before commit_T
        _, wrong = ap_key(1 - curve, n)
        with wrong:
            arg_error(nf.commit_t, wrong, _arr(fresh["W"]), _arr(fresh["X"]))
        _, short = ap_key(curve, n - 1)
        with short:
            arg_error(nf.commit_t, short, _arr(fresh["W"]), _arr(fresh["X"]))
        _, key = ap_key(curve, n)
        with key:
            nf.commit_t(key, _arr(fresh["W"]), _arr(fresh["X"]))
            nf.fold(5)
            arg_error(nf.fold, 5)                                       # a second fold needs the next commit_T
        arg_error(nf.read, 0, nv + 1)                                   # more than W holds
        assert nf.check_relaxed() == (0, None)
