"""The verifier's matrix evaluations (include/reef_msm.h 3k) and the sum-check verifier of reef_amd.verify without a GPU: the symbol
is declared, exported and bound on every side; the big-integer model the GPU tests compare with satisfies the two identities that
define it; and verify_sumchecks, with the model in place of the device call, accepts and rejects what the oracle's verifier does."""
import ctypes
import os
import random

import numpy as np
import pytest

from abi_text import ROOT, header_prototypes
from oracle.spartan_oracle import Challenger, verify
from reef_amd import _ffi
from spartan_verify_model import (bits, combine, ells, entry_sums, model_evals, model_fn, named_instance, named_prove, named_shape, replayable,
                                  straddle_shape, tamperings, STRADDLE_PADS)
from oracle.spartan_oracle import renumber

SMALL = ["smallest", "dup_empty", "long_row", "vars_lt_cons", "io_close"]
NAME = "reef_spartan_eval_matrices"


def test_symbol_is_exported_declared_and_bound():
    protos = header_prototypes()
    for path in (_ffi.LIB_PATH, _ffi.EXPERIMENT_LIB_PATH):
        assert hasattr(ctypes.CDLL(path), NAME)
    assert NAME in _ffi.declared_symbols()
    assert protos[NAME] == ("i32", ["ptr", "usize", "usize", "ptr", "ptr", "bool", "ptr"])
    fn = getattr(_ffi.load(), NAME)
    assert fn.restype is ctypes.c_int and fn.argtypes == [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p,
                                                          ctypes.c_bool, ctypes.c_void_p]
    assert f"fn {NAME}(" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hdr = open(_ffi.HEADER).read()
    assert "(3k)" in hdr and hdr.index("(3j)") < hdr.index("(3k)") < hdr.index("(4) Runtime plumbing")
    assert _ffi.load().reef_abi_version() == 7


def test_fails_loudly_without_a_ctx():
    lib = _ffi.load()
    out = np.full((3, 4), 7, dtype=np.uint64)
    z = np.zeros((8, 4), dtype=np.uint64)
    assert lib.reef_spartan_eval_matrices(None, 2, 2, z.ctypes.data, z.ctypes.data, False, out.ctypes.data) == 1
    assert b"null" in lib.reef_last_error() and (out == 7).all()


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("name", SMALL)
def test_model_ties_to_the_prover(curve, name):
    """identity 1: A~ + r B~ + r^2 C~ at prove_ref's (r_x, r_y) is that prove's claims_inner[0]"""
    shape, pads = named_shape(curve, name)
    pf = named_prove(curve, name, 5)
    assert combine(model_evals(shape, pads[1], pf["r_x"], pf["r_y"]), pf["r"], shape["p"]) == pf["claims_inner"][0]


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("name", SMALL + ["straddle"])
def test_model_selects_one_position_at_a_01_point(curve, name):
    """identity 2: at the bits of (row i, col' j) the value is the sum of the entries at (i, j)"""
    shape, pads = (straddle_shape(curve, False), STRADDLE_PADS) if name == "straddle" else named_shape(curve, name)
    ell_x, ell_y = ells(pads)
    rng = random.Random(curve)
    picks = [(shape[m][0][e], shape[m][1][e]) for m in "ABC" for e in [rng.randrange(len(shape[m][0]))] if shape[m][0]]
    picks += [(rng.randrange(shape["num_cons"]), rng.randrange(shape["num_vars"] + 1 + shape["num_io"])) for _ in range(2)]
    for row, col in picks:
        point = bits(row, ell_x), bits(renumber(col, shape["num_vars"], pads[1]), ell_y)
        assert model_evals(shape, pads[1], *point) == entry_sums(shape, row, col)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("name", ["smallest", "dup_empty", "io_close"])
def test_verify_sumchecks_agrees_with_the_oracle_verifier(curve, name):
    from reef_amd.verify import verify_sumchecks
    shape, pads = named_shape(curve, name)
    inst, p = named_instance(curve, name), shape["p"]
    pf = named_prove(curve, name, 5)
    fn = model_fn(shape)
    verify(shape, inst, pads[0], pads[1], pf, Challenger(p, 5))
    assert verify_sumchecks(None, pads[0], pads[1], inst["u"], inst["X"], pf, Challenger(p, 5), p, evals_fn=fn) is True
    assert verify_sumchecks(None, pads[0], pads[1], inst["u"], inst["X"], replayable(pf), Challenger(p, 5), p, evals_fn=fn) is True
    assert verify_sumchecks(None, pads[0], pads[1], inst["u"], inst["X"], pf, Challenger(p, 6), p, evals_fn=fn) is False   # another transcript
    for what, bad, u, X in tamperings(pf, inst["u"], inst["X"], p):
        with pytest.raises(AssertionError):
            verify(shape, dict(inst, u=u, X=list(X)), pads[0], pads[1], bad, Challenger(p, 5))
        assert verify_sumchecks(None, pads[0], pads[1], u, X, bad, Challenger(p, 5), p, evals_fn=fn) is False, what
        assert verify_sumchecks(None, pads[0], pads[1], u, X, replayable(bad), Challenger(p, 5), p, evals_fn=fn) is False, what
    wrong = lambda *a: [(v + 1) % p for v in fn(*a)]                     # and a wrong evaluation is caught by the final check
    assert verify_sumchecks(None, pads[0], pads[1], inst["u"], inst["X"], pf, Challenger(p, 5), p, evals_fn=wrong) is False


def test_matrix_evals_checks_the_point_lengths_on_the_host():
    from reef_amd.verify import matrix_evals
    with pytest.raises(ValueError):
        matrix_evals(None, 4, 4, [1], [1, 2, 3])
    with pytest.raises(ValueError):
        matrix_evals(None, 4, 4, [1, 2], [1, 2])
