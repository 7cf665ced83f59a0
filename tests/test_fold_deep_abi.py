"""The deep fold and the small-key switch at the C ABI, without a GPU: the four symbols are declared, exported and bound; reef_fold_deep,
reef_msm_ctx_create_folded and both setters reject bad arguments before they touch a device; the Python front-ends carry the calls; the
order table the arguments share (proof_order.h) still passes its self-test untouched."""
import ctypes
import os
import subprocess

import numpy as np

from reef_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("reef_fold_deep", "reef_msm_ctx_create_folded", "reef_spartan_open_set_small_key", "reef_hyrax_set_small_key")


def test_the_new_symbols_are_declared_exported_and_bound():
    declared = _ffi.declared_symbols()
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    for lib in (_ffi.load(), _ffi.load_experiment()):
        for name in NEW:
            assert name in declared and hasattr(raw, name)
            assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is ctypes.c_int, name


def test_fold_deep_rejects_bad_arguments_without_a_device():
    lib = _ffi.load()
    w = np.zeros((2, 4), dtype=np.uint64)
    out = np.full((4, 8), 7, dtype=np.uint64)
    assert lib.reef_fold_deep(None, w.ctypes.data, w.ctypes.data, 1, out.ctypes.data, 0) == 1 and b"null" in lib.reef_last_error()
    assert (out == 7).all()
    h = ctypes.c_void_p()
    assert lib.reef_msm_ctx_create_folded(ctypes.byref(h), None, w.ctypes.data, w.ctypes.data, 1, None) == 1 and h.value is None
    assert lib.reef_msm_ctx_create_folded(None, None, None, None, 0, None) == 1


def test_the_setters_reject_bad_arguments_without_a_device():
    lib = _ffi.load()
    for fn in (lib.reef_spartan_open_set_small_key, lib.reef_hyrax_set_small_key):
        for bad in (3, 5, 6, 1000, (1 << 40) + 1):
            assert fn(None, bad) == 1 and b"power of two" in lib.reef_last_error(), bad
        for good in (0, 1, 2, 1024):                       # a power of two, but no ctx to set it on
            assert fn(None, good) == 1 and b"null" in lib.reef_last_error(), good


def test_the_front_ends_carry_the_calls():
    from reef_amd import hyrax, msm, provider, spartan
    assert callable(msm.fold_deep) and callable(msm.MsmContext.fold_deep) and callable(msm.MsmContext.folded)
    assert callable(hyrax.HyraxEval.set_small_key) and callable(spartan.Opening.set_small_key) and callable(provider.FoldedGens.resident)
    hpp = open(os.path.join(_ffi.CSRC, "host", "reef_provider.hpp")).read()
    for name in NEW:
        assert name in hpp, name
    assert "struct FoldedGens" in hpp and "materialize(" in hpp and "size_t small_key = 0" in hpp
    assert "small_key=" in open(os.path.join(_ffi.CSRC, "host", "reef_replay.cpp")).read()


def test_the_order_table_self_test_still_passes():
    """proof_order.h is untouched by the switch: the call order of the arguments is what it was."""
    exe = os.path.join(os.path.dirname(_ffi.LIB_PATH), "proof_order_selftest")
    assert os.path.exists(exe), "run __graft_entry__.build() first"
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.startswith("proof_order_selftest: ok, "), out.stdout[-800:] + out.stderr[-800:]
    order = open(os.path.join(_ffi.CSRC, "proof_order.h")).read()
    assert "small_key" not in order and "folded" not in order
