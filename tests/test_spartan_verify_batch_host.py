"""The verifier's matrix evaluations at many points (include/reef_msm.h 3o) and verify_sumchecks_batch without a GPU: the three symbols
are declared, exported and bound on every side; a NULL ctx fails with nothing written; and verify_sumchecks_batch, with the model in
place of the device call, returns what verify_sumchecks returns proof by proof and makes at most one call, over the proofs whose host
checks passed."""
import ctypes
import os

import numpy as np
import pytest

from abi_text import ROOT, header_prototypes
from oracle.spartan_oracle import Challenger
from reef_amd import _ffi
from spartan_verify_model import model_evals, model_fn, named_instance, named_prove, named_shape, replayable, tamperings

SMALL = ["smallest", "dup_empty", "long_row", "vars_lt_cons", "io_close"]
BATCH, SETTER, INFO = "reef_spartan_eval_matrices_batch", "reef_nifs_set_eval_workspace", "reef_spartan_eval_matrices_batch_last_info"
SZ = ctypes.POINTER(ctypes.c_size_t)
WANT = {BATCH: (("i32", ["ptr", "usize", "usize", "ptr", "ptr", "usize", "bool", "ptr"]),
                [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_bool, ctypes.c_void_p]),
        SETTER: (("i32", ["ptr", "usize"]), [ctypes.c_void_p, ctypes.c_size_t]),
        INFO: (("i32", ["ptr", "ptr", "ptr", "ptr"]), [ctypes.c_void_p, SZ, SZ, SZ])}


def test_symbols_are_exported_declared_and_bound():
    protos = header_prototypes()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, (proto, argtypes) in WANT.items():
        for path in (_ffi.LIB_PATH, _ffi.EXPERIMENT_LIB_PATH):
            assert hasattr(ctypes.CDLL(path), name), (name, path)
        assert name in _ffi.declared_symbols()
        assert protos[name] == proto, name
        fn = getattr(_ffi.load(), name)
        assert fn.restype is ctypes.c_int and fn.argtypes == argtypes, name
        assert f"fn {name}(" in integration, name
    hdr = open(_ffi.HEADER).read()
    assert hdr.index("(3n)") < hdr.index("(3o)") < hdr.index("(4) Runtime plumbing")
    assert _ffi.load().reef_abi_version() == 7


def test_fails_loudly_without_a_ctx():
    lib = _ffi.load()
    out = np.full((6, 4), 7, dtype=np.uint64)
    z = np.zeros((8, 4), dtype=np.uint64)
    assert lib.reef_spartan_eval_matrices_batch(None, 2, 2, z.ctypes.data, z.ctypes.data, 2, False, out.ctypes.data) == 1
    assert b"null" in lib.reef_last_error() and (out == 7).all()
    assert lib.reef_spartan_eval_matrices_batch(None, 2, 2, z.ctypes.data, z.ctypes.data, 0, False, out.ctypes.data) == 1
    assert lib.reef_nifs_set_eval_workspace(None, 1 << 20) == 1
    g, k, b = (ctypes.c_size_t(7) for _ in range(3))
    assert lib.reef_spartan_eval_matrices_batch_last_info(None, ctypes.byref(g), ctypes.byref(k), ctypes.byref(b)) == 1
    assert (g.value, k.value, b.value) == (7, 7, 7)


class Stub:
    """the model as verify_sumchecks_batch's evals_fn, recording its calls"""
    def __init__(self, shape):
        self.shape, self.calls = shape, []

    def __call__(self, nifs, ncp, nvp, points):
        self.calls.append([(list(r_x), list(r_y)) for r_x, r_y in points])
        return [model_evals(self.shape, nvp, r_x, r_y) for r_x, r_y in points]


def _instance(inst, pf, p, seed, u=None, X=None):
    return {"u": inst["u"] if u is None else u, "X": inst["X"] if X is None else X, "proof": pf, "challenge": Challenger(p, seed)}


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("name", SMALL)
def test_batch_returns_what_the_single_verifier_returns(curve, name):
    from reef_amd.verify import verify_sumchecks, verify_sumchecks_batch
    shape, pads = named_shape(curve, name)
    inst, p = named_instance(curve, name), shape["p"]
    pfs = {seed: named_prove(curve, name, seed) for seed in (5, 6)}
    cases = [(5, pfs[5], None, None), (6, replayable(pfs[6]), None, None), (6, pfs[5], None, None)]      # the last: another transcript
    what, bad, u, X = tamperings(pfs[5], inst["u"], inst["X"], p)[3 + curve]
    cases.append((5, replayable(bad), u, X))
    single = [verify_sumchecks(None, pads[0], pads[1], inst["u"] if u is None else u, inst["X"] if X is None else X, pf, Challenger(p, seed), p,
                               evals_fn=model_fn(shape)) for seed, pf, u, X in cases]
    assert single == [True, True, False, False]
    stub = Stub(shape)
    got = verify_sumchecks_batch(None, pads[0], pads[1], [_instance(inst, pf, p, seed, u, X) for seed, pf, u, X in cases], p, evals_fn=stub)
    assert got == single
    assert len(stub.calls) == 1 and all(len(r_x) == len(pfs[5]["r_x"]) for r_x, _ in stub.calls[0])


@pytest.mark.parametrize("curve", [0, 1])
def test_one_tampered_proof_is_the_one_rejected(curve):
    from reef_amd.verify import verify_sumchecks_batch
    shape, pads = named_shape(curve, "dup_empty")
    inst, p = named_instance(curve, "dup_empty"), shape["p"]
    pf = named_prove(curve, "dup_empty", 5)
    for k, (what, bad, u, X) in enumerate(tamperings(pf, inst["u"], inst["X"], p)):
        at = k % 3
        batch = [_instance(inst, pf, p, 5) for _ in range(3)]
        batch[at] = _instance(inst, replayable(bad), p, 5, u, X)
        stub = Stub(shape)
        got = verify_sumchecks_batch(None, pads[0], pads[1], batch, p, evals_fn=stub)
        assert got == [i != at for i in range(3)], what
        # a tampering the host chain catches never reaches the device call; one only the final comparison catches does
        assert len(stub.calls) == 1 and len(stub.calls[0]) in (2, 3), what
        if what.startswith("claims_outer") or what == "outer round":
            assert stub.calls[0] == [(pf["r_x"], pf["r_y"])] * 2, what


@pytest.mark.parametrize("curve", [0, 1])
def test_the_call_covers_only_the_proofs_that_passed_and_is_not_made_for_none(curve):
    from reef_amd.verify import verify_sumchecks_batch
    shape, pads = named_shape(curve, "io_close")
    inst, p = named_instance(curve, "io_close"), shape["p"]
    good, other = named_prove(curve, "io_close", 5), named_prove(curve, "io_close", 6)
    short = dict(replayable(good), outer=good["outer"][:-1])
    stub = Stub(shape)
    batch = [_instance(inst, short, p, 5), _instance(inst, good, p, 5), _instance(inst, good, p, 6), _instance(inst, other, p, 6)]
    assert verify_sumchecks_batch(None, pads[0], pads[1], batch, p, evals_fn=stub) == [False, True, False, True]
    assert stub.calls == [[(good["r_x"], good["r_y"]), (other["r_x"], other["r_y"])]]
    stub = Stub(shape)
    assert verify_sumchecks_batch(None, pads[0], pads[1], [_instance(inst, short, p, 5), _instance(inst, good, p, 6)], p, evals_fn=stub) == [False, False]
    assert stub.calls == []
    assert verify_sumchecks_batch(None, pads[0], pads[1], [], p, evals_fn=stub) == [] and stub.calls == []
    wrong = lambda *a: [[(v + 1) % p for v in ev] for ev in Stub(shape)(*a)]           # a wrong evaluation is caught by the final check
    assert verify_sumchecks_batch(None, pads[0], pads[1], [_instance(inst, good, p, 5)], p, evals_fn=wrong) == [False]


def test_matrix_evals_batch_checks_the_point_lengths_on_the_host():
    from reef_amd.verify import matrix_evals_batch
    with pytest.raises(ValueError):
        matrix_evals_batch(None, 4, 4, [([1, 2], [1, 2, 3]), ([1], [1, 2, 3])])          # ragged r_x
    with pytest.raises(ValueError):
        matrix_evals_batch(None, 4, 4, [([1, 2], [1, 2, 3]), ([1, 2], [1, 2])])          # ragged r_y
    with pytest.raises(ValueError):
        matrix_evals_batch(None, 4, 4, [([1], [1, 2, 3])] * 2)                           # all alike, but not what the pads take
    with pytest.raises(ValueError):
        matrix_evals_batch(None, 4, 4, [([1, 2], [1, 2, 3], [4])])                       # not a pair
    assert matrix_evals_batch(None, 4, 4, []) == []                                      # no call is made
