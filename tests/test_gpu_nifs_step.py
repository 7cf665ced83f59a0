"""The step's two commitments from one upload (reef_nifs_commit_step), the running instance's commitments (reef_nifs_commit_running)
and the check of the fresh instance (reef_nifs_check_fresh) on the GPU, bit-exact against oracle/r1cs_oracle.py and oracle/pasta_ref's
MSM: both curves and forms, row tails on either side, the segment path, the row length at which wide rows change route, the key kinds,
a chain that alternates commit_T and commit_step, device inputs, and the argument errors with the ctx left as it was."""
import ctypes
import functools
import random

import numpy as np
import pytest

from gpu_drivers import ap_key, arr, key_of_kind, pads_of, set_running, upload_shape
from oracle import pasta_ref as R
from oracle.r1cs_oracle import bad_rows, cross_term, fold, fresh_instance, layered_shape, running_from_fresh, to_mont
from reef_amd._fe import _arr, _ints

pytestmark = pytest.mark.gpu

ZERO32 = bytes(32)


def _relaxed_running(shape, seed):
    """A running instance with u != 1 and E != 0: one reference fold of two fresh instances (as tests/test_gpu_nifs.py makes it)."""
    p, n = shape["p"], shape["num_cons"]
    run = running_from_fresh(fresh_instance(shape, seed), n)
    fresh = fresh_instance(shape, seed + 1000)
    return fold(run, fresh, cross_term(shape, run, fresh, p), random.Random(seed).randrange(p), p)


SHAPES = {   # name: layered_shape keyword arguments
    "1": dict(num_cons=1, num_inputs=2, num_io=1),
    "127_dup": dict(num_cons=127, dup_every=3, extra_vars=4),
    "vars_lt_cons": dict(num_cons=500, num_inputs=3, empty_every=2),                    # row 0 (W2) has a zero tail
    "vars_gt_cons": dict(num_cons=40, extra_vars=300),                                   # row 1 (T) has one; the key covers num_vars
    "4096_empty_long": dict(num_cons=4096, empty_every=9, long_row=(1 << 14) + 3, dup_every=11),   # the segment path writes into row 1
    "len_8191": dict(num_cons=8191, empty_every=2),                                      # max(num_vars, num_cons) = 8191 and 8192: where
    "len_8192": dict(num_cons=8192, empty_every=2),                                      # rows of a batch change route in v_msm_rows
    "11376": dict(num_cons=11376, extra_vars=1000, num_io=4),
    "39484_long": dict(num_cons=39484, long_row=(1 << 14) + 77, empty_every=101, dup_every=13),
}


def _msm_ref(curve, bases, ints):
    if not ints:
        return ZERO32
    return R.compress(curve, R.msm_pippenger(curve, np.ascontiguousarray(bases[:len(ints)]), _arr(ints), mont=False, threads=4))


@functools.lru_cache(maxsize=None)
def _case(curve, name):
    """The reference of one step on a shape, computed once and shared: never modified by a test."""
    shape = layered_shape(curve, seed=len(name) + curve, **SHAPES[name])
    p, n, nv = shape["p"], shape["num_cons"], shape["num_vars"]
    run = _relaxed_running(shape, 7)
    fresh = fresh_instance(shape, 8)
    t_ref = cross_term(shape, run, fresh, p)
    r = random.Random(name).randrange(p)
    bases = R.gen_bases_ap(curve, 42, 5, max(n, nv))
    return dict(shape=shape, p=p, n=n, nv=nv, run=run, fresh=fresh, t=t_ref, r=r, folded=fold(run, fresh, t_ref, r, p), bases=bases,
                comm_w=_msm_ref(curve, bases, fresh["W"]), comm_t=_msm_ref(curve, bases, t_ref))


def _new_ctx(curve, c, is_mont, zero_e=False, run=None):
    from reef_amd.nifs import Nifs
    nf = Nifs(curve, c["n"], c["nv"], c["shape"]["num_io"])
    upload_shape(nf, c["shape"], is_mont)
    set_running(nf, run or c["run"], c["p"], is_mont, zero_e=zero_e)
    return nf


def _assert_step(nf, key, curve, c, is_mont, w2=None, x2=None):
    """The assertions of one commit_step and the fold behind it against the case's reference."""
    from reef_amd.msm import compress
    from reef_amd.nifs import E, T, U, W, X
    p = c["p"]
    w2 = arr(c["fresh"]["W"], p, is_mont) if w2 is None else w2
    x2 = arr(c["fresh"]["X"], p, is_mont) if x2 is None else x2
    cw, ct = nf.commit_step(key, w2, x2, is_mont=is_mont)
    form = "Montgomery" if is_mont else "canonical"
    assert compress(curve, cw) == c["comm_w"], f"comm_W2 ({form} inputs)"
    assert compress(curve, ct) == c["comm_t"], f"comm_T ({form} inputs)"
    assert _ints(nf.read(T)) == c["t"], f"T ({form} inputs)"
    assert nf.check_fresh() == (0, None)
    nf.fold(to_mont([c["r"]], p)[0] if is_mont else c["r"], is_mont=is_mont)
    ref = c["folded"]
    assert _ints(nf.read(W)) == ref["W"]
    assert _ints(nf.read(E)) == ref["E"]
    assert _ints(nf.read(U)) == [ref["u"]]
    assert _ints(nf.read(X)) == ref["X"]
    assert nf.check_relaxed() == (0, None)


# ---------------------------------------------------------------------------------------------------------------- 1, 8: bit-exact pair
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("name", [s for s in SHAPES if s != "39484_long"])
def test_pair_is_bit_exact_on_both_forms(gpu_lib, curve, name):
    from reef_amd.msm import MsmContext
    c = _case(curve, name)
    with MsmContext(curve, c["bases"]) as key:
        for is_mont in (False, True):
            with _new_ctx(curve, c, is_mont) as nf:
                _assert_step(nf, key, curve, c, is_mont)


@pytest.mark.parametrize("curve", [0, 1])
def test_pair_at_cfg4_size(gpu_lib, curve):
    c = _case(curve, "39484_long")
    with key_of_kind(curve, c["bases"], "plain") as key, _new_ctx(curve, c, False) as nf:
        _assert_step(nf, key, curve, c, False)


# ---------------------------------------------------------------------------------------------------------------- 2: key kinds
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("kind", ["plain", "pre", "tables"])
def test_every_key_kind_gives_the_same_points(gpu_lib, curve, kind):
    from reef_amd.msm import compress
    c = _case(curve, "11376")
    with key_of_kind(curve, c["bases"], kind) as key, _new_ctx(curve, c, False) as nf:
        _assert_step(nf, key, curve, c, False)
        cw, ce = nf.commit_running(key)
        assert compress(curve, cw) == _msm_ref(curve, c["bases"], c["folded"]["W"])
        assert compress(curve, ce) == _msm_ref(curve, c["bases"], c["folded"]["E"])


# ---------------------------------------------------------------------------------------------------------------- 3: alternating chain
@pytest.mark.parametrize("curve", [0, 1])
def test_chain_alternating_commit_t_and_commit_step(gpu_lib, curve):
    """Eight steps on one ctx, commit_T and commit_step in turn: a stale row tail or a T that moved would show in a later step."""
    from reef_amd.msm import compress
    from reef_amd.nifs import E, T, U, W, X, Nifs
    shape = layered_shape(curve, 700, num_inputs=3, num_io=3, empty_every=3, dup_every=7, long_row=300, seed=60 + curve)
    p, n, nv = shape["p"], shape["num_cons"], shape["num_vars"]
    assert nv < n
    rng = random.Random(curve)
    run = running_from_fresh(fresh_instance(shape, 0), n)
    bases, key = ap_key(curve, n)
    with key, Nifs(curve, n, nv, shape["num_io"]) as nf:
        upload_shape(nf, shape, False)
        set_running(nf, run, p, False, zero_e=True)
        for step in range(1, 9):
            fresh = fresh_instance(shape, step)
            t = cross_term(shape, run, fresh, p)
            if step % 2:
                ct = nf.commit_t(key, _arr(fresh["W"]), _arr(fresh["X"]))
            else:
                cw, ct = nf.commit_step(key, _arr(fresh["W"]), _arr(fresh["X"]))
                assert compress(curve, cw) == _msm_ref(curve, bases, fresh["W"]), f"comm_W2 of step {step}"
            assert compress(curve, ct) == _msm_ref(curve, bases, t), f"comm_T of step {step}"
            assert _ints(nf.read(T)) == t, f"T of step {step}"
            assert nf.check_fresh() == (0, None)
            r = rng.randrange(p)
            nf.fold(r)
            run = fold(run, fresh, t, r, p)
        got = {"W": _ints(nf.read(W)), "E": _ints(nf.read(E)), "u": _ints(nf.read(U))[0], "X": _ints(nf.read(X))}
        assert got == run
        assert nf.check_relaxed() == (0, None)


# ---------------------------------------------------------------------------------------------------------------- 4: device inputs
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("is_mont", [False, True])
def test_device_inputs_give_the_same_and_stay_unchanged(gpu_lib, curve, is_mont):
    from reef_amd.msm import DeviceBuffer
    c = _case(curve, "vars_lt_cons")
    w_host, x_host = arr(c["fresh"]["W"], c["p"], is_mont), arr(c["fresh"]["X"], c["p"], is_mont)
    d_w, d_x = DeviceBuffer.from_host(w_host), DeviceBuffer.from_host(x_host)
    _, key = ap_key(curve, c["n"])
    with key, _new_ctx(curve, c, is_mont) as nf:
        _assert_step(nf, key, curve, c, is_mont, w2=d_w, x2=d_x)
    assert np.array_equal(d_w.to_host(w_host.shape), w_host)
    assert np.array_equal(d_x.to_host(x_host.shape), x_host)
    d_w.free()
    d_x.free()


# ---------------------------------------------------------------------------------------------------------------- 5: commit_running
@pytest.mark.parametrize("curve", [0, 1])
def test_commit_running(gpu_lib, curve):
    from reef_amd.msm import compress
    from reef_amd.nifs import E, U, W, X
    from reef_amd.spartan import Spartan
    c = _case(curve, "127_dup")
    shape, p, n = c["shape"], c["p"], c["n"]
    bases = c["bases"]
    rng = random.Random(90 + curve)
    first = running_from_fresh(fresh_instance(shape, 0), n)
    from reef_amd.msm import MsmContext
    with MsmContext(curve, bases) as key, _new_ctx(curve, c, False, zero_e=True, run=first) as nf:
        cw, ce = nf.commit_running(key)                              # the first instance: E = 0 is the identity
        assert compress(curve, cw) == _msm_ref(curve, bases, first["W"])
        assert compress(curve, ce) == ZERO32
        run = first
        for step in range(1, 4):
            fresh = fresh_instance(shape, step)
            t = cross_term(shape, run, fresh, p)
            nf.commit_step(key, _arr(fresh["W"]), _arr(fresh["X"]))
            if step == 2:                                             # between commit_step and fold: reads only
                cw, ce = nf.commit_running(key)
                assert compress(curve, cw) == _msm_ref(curve, bases, run["W"])
                assert compress(curve, ce) == _msm_ref(curve, bases, run["E"])
            r = rng.randrange(p)
            nf.fold(r)
            run = fold(run, fresh, t, r, p)
        got = {"W": _ints(nf.read(W)), "E": _ints(nf.read(E)), "u": _ints(nf.read(U))[0], "X": _ints(nf.read(X))}
        assert got == run
        cw, ce = nf.commit_running(key)
        assert compress(curve, cw) == _msm_ref(curve, bases, run["W"])
        assert compress(curve, ce) == _msm_ref(curve, bases, run["E"])
        # one output alone
        only = np.zeros(12, dtype=np.uint64)
        assert nf._lib.reef_nifs_commit_running(nf._h, key._h, None, only.ctypes.data) == 0
        assert compress(curve, only) == _msm_ref(curve, bases, run["E"])
        # between reef_spartan_begin and the first outer round: the round is accepted and returns what it returns without the call
        ncp, nvp = pads_of(shape, None)
        tau = [rng.randrange(p) for _ in range(ncp.bit_length() - 1)]
        r0 = rng.randrange(p)
        sp = Spartan(nf)
        e0 = sp.begin(ncp, nvp, tau)
        want = sp.outer_round(r0)
        assert sp.begin(ncp, nvp, tau) == e0
        nf.commit_running(key)
        assert nf.check_fresh() == (0, None)
        assert sp.outer_round(r0) == want


# ---------------------------------------------------------------------------------------------------------------- 6: check_fresh
@pytest.mark.parametrize("curve", [0, 1])
def test_check_fresh_reports_the_tampered_rows(gpu_lib, curve):
    from reef_amd._ffi import ReefError
    c = _case(curve, "4096_empty_long")
    shape, p, n = c["shape"], c["p"], c["n"]
    plan = shape["plan"]
    rows = [i for i in range(n) if plan[i] is not None]
    assert plan[n // 2] is not None
    _, key = ap_key(curve, max(n, c["nv"]))
    with key, _new_ctx(curve, c, False) as nf:
        with pytest.raises(ReefError) as e:                          # no fresh instance yet
            nf.check_fresh()
        assert e.value.status == 1

        def check(tampered_rows):
            w = list(c["fresh"]["W"])
            for k in tampered_rows:
                w[plan[k][4]] = (w[plan[k][4]] + 1) % p
            nf.commit_t(key, _arr(w), _arr(c["fresh"]["X"]))
            bad = bad_rows(shape, {"W": w, "E": [0] * n, "u": 1, "X": c["fresh"]["X"]}, p)
            assert nf.check_fresh() == (len(bad), bad[0] if bad else None)
            return bad
        assert check([]) == []
        for k in (rows[0], rows[len(rows) // 2], rows[-1], n // 2):
            assert k in check([k])
        # seven rows whose output no other row reads: exactly those fail
        used_by = {}
        for m in "ABC":
            for r_, col in zip(shape[m][0], shape[m][1]):
                used_by.setdefault(col, set()).add(r_)
        lone = [k for k in rows[5:] if used_by[plan[k][4]] == {k}][:7]
        assert len(lone) == 7
        assert check(lone) == lone
        assert nf.check_fresh() == (7, lone[0])


# ---------------------------------------------------------------------------------------------------------------- 7: argument errors
@pytest.mark.parametrize("curve", [0, 1])
def test_argument_errors_leave_the_ctx_as_it_was(gpu_lib, curve):
    from reef_amd._ffi import ReefError
    from reef_amd.msm import MsmContext, compress
    from reef_amd.nifs import T, Nifs
    from reef_amd.spartan import Spartan
    c = _case(curve, "vars_gt_cons")
    shape, p, n, nv = c["shape"], c["p"], c["n"], c["nv"]
    assert nv > n
    w2, x2 = _arr(c["fresh"]["W"]), _arr(c["fresh"]["X"])
    lib = None

    def arg_error(fn, *a, **k):
        with pytest.raises(ReefError) as e:
            fn(*a, **k)
        assert e.value.status == 1                                   # REEF_ERR_ARG
        return str(e.value)

    with MsmContext(curve, c["bases"]) as key, MsmContext(curve, c["bases"][:n]) as short, \
            MsmContext(1 - curve, R.gen_bases_ap(1 - curve, 42, 5, nv)) as wrong, Nifs(curve, n, nv, shape["num_io"]) as nf:
        lib = nf._lib
        upload_shape(nf, shape, False)
        arg_error(nf.commit_step, key, w2, x2)                       # before set_running
        arg_error(nf.commit_running, key)
        set_running(nf, c["run"], p, False)
        arg_error(nf.fold, 5)                                        # no cross term yet
        msg = arg_error(nf.commit_step, short, w2, x2)               # the key covers num_cons, not num_vars
        assert str(n) in msg and str(nv) in msg
        arg_error(nf.fold, 5)                                        # ... and the fold is refused as before
        arg_error(nf.read, T)                                        # ... and there is still no T
        msg = arg_error(nf.commit_running, short)
        assert str(n) in msg and str(nv) in msg
        # a committed step and a prove in flight: refused calls change neither
        nf.commit_step(key, w2, x2)
        ncp, nvp = pads_of(shape, None)
        rng = random.Random(curve)
        tau = [rng.randrange(p) for _ in range(ncp.bit_length() - 1)]
        sp = Spartan(nf)
        sp.begin(ncp, nvp, tau)
        other = _arr([(v + 1) % p for v in c["fresh"]["W"]])
        arg_error(nf.commit_step, short, other, x2)
        arg_error(nf.commit_step, wrong, other, x2)                  # a key of the other curve
        arg_error(nf.commit_running, wrong)
        out = np.zeros(12, dtype=np.uint64)
        assert lib.reef_nifs_commit_step(nf._h, key._h, other.ctypes.data, x2.ctypes.data, 0, False, None, out.ctypes.data) == 1
        assert lib.reef_nifs_commit_step(nf._h, key._h, other.ctypes.data, x2.ctypes.data, 0, False, out.ctypes.data, None) == 1
        assert lib.reef_nifs_commit_running(nf._h, key._h, None, None) == 1
        assert _ints(nf.read(T)) == c["t"]                           # T of the step before the refused calls
        assert nf.check_fresh() == (0, None)                         # and its z2
        sp.outer_round(rng.randrange(p))                             # the prove was not voided
        nf.fold(c["r"])                                              # the one fold of the committed step
        arg_error(nf.fold, c["r"])                                   # a second fold needs the next commit
        assert nf.check_relaxed() == (0, None)
        cw, ce = nf.commit_running(key)
        assert compress(curve, ce) == _msm_ref(curve, c["bases"], c["folded"]["E"])
        # a key with a window split is refused
        assert lib.reef_msm_ctx_set_window_split(key._h, 0, 2) == 0
        arg_error(nf.commit_step, key, w2, x2)
        arg_error(nf.commit_running, key)
        assert lib.reef_msm_ctx_set_window_split(key._h, 0, 1) == 0
