"""reef_ipa_check_batch (include/reef_msm.h 3m) without a GPU: the symbol in both libraries, the header, the binding and
INTEGRATION.md; the layout of reef_ipa_proof; the two answers that need no device (a null key, an empty batch); and the closed form
of b_hat = <s, pad(eq(p))> as reef_amd.verify restates it, against the oracle's s vector and eq table entry by entry."""
import ctypes
import os
import random
import re

import pytest

from oracle.ipa_oracle import dot, pad, s_vector
from oracle.r1cs_oracle import field
from oracle.spartan_oracle import eq_evals
from reef_amd import _ffi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("reef_ipa_check_batch", "reef_ipa_check_batch_last_timing")


def test_symbol_is_exported_declared_bound_and_documented():
    for path in (_ffi.LIB_PATH, _ffi.EXPERIMENT_LIB_PATH):
        raw = ctypes.CDLL(path)
        for name in NAMES:
            assert hasattr(raw, name), (path, name)
    declared = _ffi.declared_symbols()
    lib = _ffi.load()
    for name in NAMES:
        assert name in declared, name
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is ctypes.c_int, name
    assert len(lib.reef_ipa_check_batch.argtypes) == 13
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "fn reef_ipa_check_batch(" in text and "struct ReefIpaProof" in text and "#[repr(C)]" in text


def test_proof_struct_matches_the_header():
    assert ctypes.sizeof(_ffi.IpaProof) == 104
    header = open(_ffi.HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} reef_ipa_proof;", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        names = re.findall(r"\*?\s*(\w+)\s*(?:,|$)", decl.strip())
        fields += [n for n in names if n]
    assert fields == [f[0] for f in _ffi.IpaProof._fields_], fields
    assert [getattr(_ffi.IpaProof, f).offset for f in fields] == [8 * i for i in range(13)]


def test_null_key_is_an_argument_error_with_nothing_written():
    lib = _ffi.load()
    acc = ctypes.c_uint32(7)
    proofs = (_ffi.IpaProof * 1)()
    rho = (ctypes.c_uint64 * 4)(1, 0, 0, 0)
    each = (ctypes.c_uint32 * 1)(9)
    assert lib.reef_ipa_check_batch(None, 4, proofs, 1, ctypes.cast(rho, ctypes.c_void_p), False, ctypes.byref(acc), ctypes.cast(each, ctypes.c_void_p),
                                    None, None, 0, None, None) == 1
    assert acc.value == 7 and each[0] == 9
    assert lib.reef_ipa_check_batch_last_timing(None, None, None, None) == 1


def test_an_empty_batch_accepts_without_a_device():
    lib = _ffi.load()
    acc = ctypes.c_uint32(7)
    assert lib.reef_ipa_check_batch(None, 4, None, 0, None, False, ctypes.byref(acc), None, None, None, 0, None, None) == 0
    assert acc.value == 1


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("k", [1, 2, 9])
def test_closed_form_b_hat_equals_the_dot_product(curve, k):
    """One and two points; v = 0 (b = the unit vector e_0), 0 < v < k, v = k."""
    from reef_amd.verify import eq_b_hat
    p = field(curve)
    n = 1 << k
    rng = random.Random(17 * curve + k)
    rs = [rng.randrange(1, p) for _ in range(k)]
    s = s_vector(rs, p)
    vs = sorted({0, k // 2, k - 1, k})
    shapes = [[v] for v in vs] + [[a, b] for a in vs for b in vs]
    assert any(0 < v < k for v in vs) or k == 1
    for shape in shapes:
        points = [[rng.randrange(p) for _ in range(v)] for v in shape]
        weights = [rng.randrange(p) for _ in shape]
        b = [0] * n
        for pt, w in zip(points, weights):
            for j, e in enumerate(eq_evals(pt, p) if pt else [1]):
                b[j] = (b[j] + w * e) % p
        assert eq_b_hat(rs, points, weights, p) == dot(s, pad(b, n), p), (k, shape)
    with pytest.raises(ValueError):
        eq_b_hat(rs, [[1] * (k + 1)], [1], p)
