"""The step's paired commitment (include/reef_msm.h 3f: reef_nifs_commit_step, reef_nifs_commit_running, reef_nifs_check_fresh)
without a GPU: the symbols are exported and declared, the ABI version stands, and the binding checks lengths before the library."""
import numpy as np
import pytest

from abi_text import header_prototypes
from reef_amd import _ffi

NEW = ("reef_nifs_commit_step", "reef_nifs_commit_running", "reef_nifs_check_fresh")


def test_the_three_symbols_are_exported_and_declared():
    lib = _ffi.load()
    protos = header_prototypes()
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in protos, f"{name} is not declared in include/reef_msm.h"
        assert getattr(lib, name).argtypes is not None, f"{name} has no ctypes declaration"
    assert protos["reef_nifs_commit_step"] == ("i32", ["ptr", "ptr", "ptr", "ptr", "i32", "bool", "ptr", "ptr"])
    assert protos["reef_nifs_commit_running"] == ("i32", ["ptr"] * 4)
    assert protos["reef_nifs_check_fresh"] == protos["reef_nifs_check_relaxed"]


def test_abi_version_stays_7():
    assert _ffi.load().reef_abi_version() == 7


def test_the_binding_refuses_wrong_lengths_before_the_library():
    from reef_amd.nifs import Nifs
    nf = Nifs.__new__(Nifs)                       # no ctx: the length checks come before any call into the library
    nf._lib, nf._h, nf.num_cons, nf.num_vars, nf.num_io = None, None, 5, 4, 2
    good_w, good_x = np.zeros((4, 4), dtype=np.uint64), np.zeros((2, 4), dtype=np.uint64)
    with pytest.raises(ValueError):
        nf.commit_step(None, np.zeros((3, 4), dtype=np.uint64), good_x)
    with pytest.raises(ValueError):
        nf.commit_step(None, good_w, np.zeros((3, 4), dtype=np.uint64))
    with pytest.raises(ValueError):
        nf.commit_step(None, np.zeros((5, 4), dtype=np.uint64), good_x)


def test_nifs_needs_a_device():
    from reef_amd import msm
    from reef_amd._ffi import ReefError
    from reef_amd.nifs import Nifs
    if msm.device_count() > 0:
        with Nifs(0, 4, 4, 1) as nf:              # with a device the three calls exist on the handle; before set_running they are refused
            with pytest.raises(ReefError) as e:
                nf.check_fresh()
            assert e.value.status == 1
        return
    with pytest.raises(ReefError) as e:
        Nifs(0, 4, 4, 1)
    assert e.value.status == 3                    # REEF_ERR_NO_GPU
