"""reef_decompress / reef_hyrax_eval_comm_compressed without a GPU (include/reef_msm.h, K4's inverse): the header declares them and the
library exports them, with ctypes signatures that match; without a device they fail as every entry point does; the 2-adic inputs of
the GPU test are what they claim to be; and the host build of decompress_kernels.inc (the fixed-trip-count square root and the
decoding rule the kernel runs, compiled with g++ and REEF_BOUNDS) agrees with the oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from abi_text import header_prototypes
from decompress_inputs import CURVE_OF, FIELDS, check_roots, special_batch, sqrt_inputs, to_abi, two_adic_inputs, zeta
from oracle.pasta_oracle import ap_bases, sqrt_mod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reef_amd", "csrc")
SO = os.path.join(ROOT, "reef_amd", "_lib", "libreef_sqrtcheck.so")
SYMBOLS = ("reef_decompress", "reef_hyrax_eval_comm_compressed")


def test_the_header_declares_and_the_library_exports_both_functions():
    from reef_amd import _ffi
    lib = _ffi.load()
    protos = header_prototypes()
    for name in SYMBOLS:
        assert name in _ffi.declared_symbols() and name in protos, name
        assert getattr(lib, name).argtypes is not None, f"{name} has no ctypes signature"
    assert protos["reef_decompress"] == ("i32", ["i32", "ptr", "usize", "i32", "ptr", "ptr", "ptr"])
    assert protos["reef_hyrax_eval_comm_compressed"] == ("i32", ["ptr", "ptr", "i32", "ptr"])
    assert lib.reef_abi_version() == _ffi.ABI_VERSION == 7


def test_without_a_gpu_both_fail_loudly():
    from reef_amd import _ffi, msm
    from reef_amd.hyrax import HyraxEval
    lib = _ffi.load()
    if lib.reef_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(msm.ReefError) as e:
        msm.decompress("pallas", bytes(64))
    assert e.value.status == 3                            # REEF_ERR_NO_GPU: no CPU fallback
    with pytest.raises(msm.ReefError) as e:               # no ctx can exist ...
        HyraxEval(0, np.zeros(16, np.uint8), 4)
    assert e.value.status == 3
    out = np.zeros(12, np.uint64)                         # ... and the entry point refuses the null one it is left with
    assert lib.reef_hyrax_eval_comm_compressed(None, bytes(64), 0, out.ctypes.data) == 1
    assert b"null" in lib.reef_last_error()


@pytest.mark.parametrize("field", [0, 1])
def test_two_adic_inputs_have_the_order_they_claim(field):
    p = FIELDS[field]
    T = (p - 1) >> 32
    assert pow(zeta(p), 1 << 31, p) == p - 1
    for k in range(33):
        vals = two_adic_inputs(p, k)
        assert len(set(vals)) == 3
        for v in vals:
            t = pow(v, T, p)
            assert pow(t, 1 << k, p) == 1 and (k == 0 or pow(t, 1 << (k - 1), p) != 1), k
            root = sqrt_mod(v, p)
            assert (root is None) == (k == 32), k
            assert root is None or root * root % p == v


@pytest.fixture(scope="module")
def host():
    src = os.path.join(CSRC, "tools", "sqrt_check.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("field.h", "ec.h", "field_consts.h", "decompress_kernels.inc")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DREEF_BOUNDS", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    vp = ctypes.c_void_p
    lib.sqrtcheck_root.argtypes = [ctypes.c_int, vp, vp, ctypes.c_size_t]
    lib.sqrtcheck_decompress.argtypes = [ctypes.c_int, vp, vp, ctypes.c_size_t]
    lib.sqrtcheck_decompress.restype = ctypes.c_size_t
    return lib


@pytest.mark.parametrize("field", [0, 1])
def test_host_build_of_the_windowed_root_at_every_two_adic_order(host, field):
    p = FIELDS[field]
    vals = sqrt_inputs(p)
    a = to_abi([v for v, _ in vals], p)
    out = np.zeros_like(a)
    host.sqrtcheck_root(field, a.ctypes.data, out.ctypes.data, len(vals))
    check_roots(vals, out, p, "host build")


@pytest.mark.parametrize("curve", [0, 1])
def test_host_build_of_the_decoding_rule(host, curve):
    cv = CURVE_OF[curve]
    pts = ap_bases(cv, 11, 3, 64)
    encs, want, bad = special_batch(curve, pts)
    assert len(bad) == 12 and {e[31] >> 7 for i, e in enumerate(encs) if i not in bad} == {0, 1}
    out = np.zeros((64, 8), np.uint64)
    assert host.sqrtcheck_decompress(curve, b"".join(encs), out.ctypes.data, 64) == len(bad)
    assert out.tobytes() == b"".join(want)
