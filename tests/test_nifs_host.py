"""Row N6 on the host: the big-integer reference of one NIFS step and of is_sat_relaxed (oracle/r1cs_oracle.py) checked against
itself -- fresh instances of the layered generator satisfy the relation, folds keep it, tampering is caught; the library's new
symbols; the loud failure without a GPU."""
import random

import pytest

from oracle.pasta_oracle import Q
from oracle.r1cs_oracle import bad_rows, cross_term, fold, fresh_instance, layered_shape, running_from_fresh
from reef_amd._fe import _arr, _ints


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("curve", [0, 1])
def test_fresh_instances_of_the_generator_satisfy_the_relation(curve):
    shape = layered_shape(curve, 300, extra_vars=5, empty_every=17, dup_every=7, long_row=200, seed=curve + 3)
    for s in range(3):
        inst = running_from_fresh(fresh_instance(shape, s), shape["num_cons"])
        assert bad_rows(shape, inst, shape["p"]) == []


@pytest.mark.parametrize("curve", [0, 1])
def test_folding_keeps_instances_satisfiable_and_tampering_is_caught(curve):
    shape = layered_shape(curve, 200, num_io=3, extra_vars=9, empty_every=11, dup_every=5, seed=curve + 10)
    p, n = shape["p"], shape["num_cons"]
    rng = random.Random(99 + curve)
    run = running_from_fresh(fresh_instance(shape, 0), n)
    for step in range(1, 9):
        fresh = fresh_instance(shape, step)
        t = cross_term(shape, run, fresh, p)
        run = fold(run, fresh, t, rng.randrange(p), p)
        assert bad_rows(shape, run, p) == [], f"step {step}"
    assert run["u"] != 1 and any(run["E"])                       # a really relaxed instance by now
    k = next(i for i in range(n) if shape["plan"][i] is not None)
    bad = dict(run, E=list(run["E"]))
    bad["E"][k] = (bad["E"][k] + 1) % p
    assert bad_rows(shape, bad, p) == [k]
    bad = dict(run, W=list(run["W"]))
    out = shape["plan"][k][4]
    bad["W"][out] = (bad["W"][out] + 1) % p                      # an output variable: its own constraint breaks
    assert k in bad_rows(shape, bad, p)
    # a wrong T breaks the fold
    fresh = fresh_instance(shape, 50)
    t = cross_term(shape, run, fresh, p)
    t[k] = (t[k] + 1) % p
    assert bad_rows(shape, fold(run, fresh, t, 5, p), p) == [k]


def test_empty_rows_and_zero_coefficients_are_trivially_satisfied():
    shape = layered_shape(0, 40, empty_every=2, seed=5)
    inst = running_from_fresh(fresh_instance(shape, 1), 40)
    assert bad_rows(shape, inst, shape["p"]) == []
    assert all(shape["plan"][i] is None for i in range(1, 40, 2))


def test_array_round_trip():
    vals = [0, 1, Q - 1, 1 << 200, 0x1234567890ABCDEF << 64]
    assert _ints(_arr(vals)) == vals


def test_library_exports_the_nifs_symbols():
    from reef_amd import _ffi
    lib = _ffi.load()
    for name in ("reef_nifs_create", "reef_nifs_destroy", "reef_nifs_set_matrix", "reef_nifs_set_running", "reef_nifs_commit_T",
                 "reef_nifs_fold", "reef_nifs_read", "reef_nifs_check_relaxed"):
        assert hasattr(lib, name), name
        assert name in _ffi.declared_symbols()
    assert lib.reef_abi_version() == 7


def test_nifs_create_fails_loudly_without_gpu():
    from reef_amd import _ffi
    from reef_amd.nifs import Nifs
    if _ffi.load().reef_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(_ffi.ReefError) as e:
        Nifs("pallas", 16, 16, 1)
    assert e.value.status == 3           # REEF_ERR_NO_GPU: no silent CPU fallback
