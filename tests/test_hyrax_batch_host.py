"""The Hyrax arguments of many proofs in lock-step (include/reef_msm.h 3p) without a GPU: the seven symbols in both libraries, the
header and the binding; the ABI version; the argument checks that need no device; and the batch's call order (csrc/proof_order.h:
hyb_check) twice over -- through its own host selftest, and against a table of phase x call x (rounds, right) written out here."""
import ctypes
import os
import subprocess

import pytest

from abi_text import header_prototypes
from reef_amd import _ffi

NAMES = ("reef_hyrax_batch_create", "reef_hyrax_batch_destroy", "reef_hyrax_batch_eval_begin", "reef_hyrax_batch_ipa_begin",
         "reef_hyrax_batch_ipa_round", "reef_hyrax_batch_finish", "reef_hyrax_batch_read")
SELFTEST = os.path.join(os.path.dirname(_ffi.LIB_PATH), "hyrax_batch_order_selftest")


def test_symbols_are_exported_declared_and_bound_as_the_header_says():
    for path in (_ffi.LIB_PATH, _ffi.EXPERIMENT_LIB_PATH):
        raw = ctypes.CDLL(path)
        for name in NAMES:
            assert hasattr(raw, name), (path, name)
    declared = _ffi.declared_symbols()
    protos = header_prototypes()
    lib = _ffi.load()
    kinds = {None: "void", ctypes.c_int: "i32", ctypes.c_bool: "bool", ctypes.c_size_t: "usize", ctypes.c_void_p: "ptr"}
    for name in NAMES:
        assert name in declared and name in protos, name
        fn = getattr(lib, name)
        got = (kinds[fn.restype], [kinds.get(t, "ptr" if hasattr(t, "contents") else t) for t in fn.argtypes])
        assert got == protos[name], f"{name}: _ffi.py declares {got}, the header {protos[name]}"
    assert protos["reef_hyrax_batch_create"] == ("i32", ["ptr", "ptr", "usize"])
    assert protos["reef_hyrax_batch_eval_begin"] == ("i32", ["ptr", "ptr", "ptr", "usize", "bool", "ptr", "ptr"])
    assert protos["reef_hyrax_batch_ipa_begin"] == ("i32", ["ptr", "ptr", "ptr", "ptr", "bool", "ptr", "ptr"])
    assert protos["reef_hyrax_batch_ipa_round"] == ("i32", ["ptr", "ptr", "ptr", "bool", "ptr", "ptr"])
    assert protos["reef_hyrax_batch_finish"] == ("i32", ["ptr", "ptr", "bool", "ptr", "ptr"])
    assert protos["reef_hyrax_batch_read"] == ("i32", ["ptr", "usize", "i32", "usize", "ptr", "bool"])
    assert protos["reef_hyrax_batch_destroy"] == ("void", ["ptr"])


def test_the_abi_version_stays():
    assert _ffi.load().reef_abi_version() == 7, "symbols added, none changed"
    assert _ffi.ABI_VERSION == 7


def test_argument_errors_that_need_no_device():
    from reef_amd.hyrax import HyraxBatch
    lib = _ffi.load()
    h = ctypes.c_void_p()
    assert lib.reef_hyrax_batch_create(ctypes.byref(h), None, 4) == 1 and not h.value           # no document
    assert lib.reef_hyrax_batch_eval_begin(None, None, None, 1, False, None, None) == 1         # no batch
    assert lib.reef_hyrax_batch_ipa_begin(None, None, None, None, False, None, None) == 1
    assert lib.reef_hyrax_batch_ipa_round(None, None, None, False, None, None) == 1
    assert lib.reef_hyrax_batch_finish(None, None, False, None, None) == 1
    assert lib.reef_hyrax_batch_read(None, 0, 0, 0, None, False) == 1
    lib.reef_hyrax_batch_destroy(None)
    for name in ("eval_begin", "ipa_begin", "ipa_round", "finish", "read"):
        assert callable(getattr(HyraxBatch, name))


def test_the_order_selftest_passes():
    """hyrax_batch_order_selftest is csrc/proof_order.h alone (host/Makefile: no HIP, no library): every phase against every call of
    the family with a table written out in the program.  One line, exit 1 on a mismatch."""
    run = subprocess.run([SELFTEST], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("hyrax_batch_order_selftest: ok, ") and run.stdout.count("\n") == 1, run.stdout
    assert subprocess.run([SELFTEST, "bogus"], capture_output=True, text=True, timeout=60).returncode == 2


NONE, EVAL, IPA, DONE = range(4)
B = "reef_hyrax_batch_"
# the next call at (phase, rounds, right), written out: right in {1, 2, 3}, rounds 0 .. 3
NEXT = {}
for _right in (1, 2, 3):
    for _rounds in range(4):
        NEXT[NONE, _rounds, _right] = B + "eval_begin"
        NEXT[EVAL, _rounds, _right] = B + "ipa_begin"
        NEXT[DONE, _rounds, _right] = B + "eval_begin"
NEXT.update({(IPA, 0, 1): B + "finish", (IPA, 1, 1): B + "finish", (IPA, 2, 1): B + "finish", (IPA, 3, 1): B + "finish",
             (IPA, 0, 2): B + "ipa_round", (IPA, 1, 2): B + "finish", (IPA, 2, 2): B + "finish", (IPA, 3, 2): B + "finish",
             (IPA, 0, 3): B + "ipa_round", (IPA, 1, 3): B + "ipa_round", (IPA, 2, 3): B + "finish", (IPA, 3, 3): B + "finish"})


def _want(phase, rounds, right, name):
    if name == B + "eval_begin":
        return "ok"                                      # always legal: it starts the batch over
    if name == B + "read":
        return "ok" if phase != NONE else f"{name}: a and b exist from reef_hyrax_batch_eval_begin on, the next call"
    nxt = NEXT[phase, rounds, right]
    return "ok" if name == nxt else f"{name}: out of order, the next call is {nxt}"


def test_the_order_function_against_a_table():
    run = subprocess.run([SELFTEST, "dump"], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    seen = set()
    for line in lines:
        head, got = line.split(" -> ", 1)
        phase, rounds, right, name = head.split(" ")
        key = (int(phase), int(rounds), int(right), name)
        assert got == _want(*key), line
        seen.add(key)
    names = [B + n for n in ("eval_begin", "ipa_begin", "ipa_round", "finish", "read")]
    assert seen == {(ph, ro, ri, n) for ph in range(4) for ro in range(4) for ri in (1, 2, 3) for n in names} and len(lines) == len(seen)
    # a whole argument walked through the table: right - 1 rounds between ipa_begin and finish, none at right = 1
    for right in (1, 2, 3):
        walk, phase, rounds = [], NONE, 0
        for _ in range(right + 2):
            walk.append(NEXT[phase, rounds, right])
            phase, rounds = {B + "eval_begin": (EVAL, 0), B + "ipa_begin": (IPA, 0), B + "ipa_round": (IPA, rounds + 1), B + "finish": (DONE, rounds)}[walk[-1]]
        assert walk == [B + "eval_begin", B + "ipa_begin"] + [B + "ipa_round"] * (right - 1) + [B + "finish"] and phase == DONE


def test_the_python_front_end_checks_lengths_before_the_library(monkeypatch):
    from reef_amd.hyrax import HyraxBatch
    hb = HyraxBatch.__new__(HyraxBatch)
    hb._h, hb._lib, hb.m, hb.m_max, hb.num_vars, hb.left, hb.right = None, None, 2, 4, 4, 2, 2
    with pytest.raises(ValueError, match="expected 2 challenges for 2 proofs, got 3"):
        hb.ipa_round([1, 2, 3])
    with pytest.raises(ValueError, match="expected 4 blinds for 2 proofs, got 2"):
        hb.ipa_round([1, 2], [1, 2])
    with pytest.raises(ValueError, match="expected 4 point entries, got 3"):
        hb.eval_begin(None, [[1, 2, 3]])
