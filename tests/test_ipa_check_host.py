"""The verifier's IPA check (include/reef_msm.h 3j) without a GPU: the symbols are exported and declared on every side, they fail
loudly when there is no device, and reef_amd.verify draws its challenges in the oracle verifiers' label order."""
import ctypes
import os

import numpy as np
import pytest

from abi_text import ROOT, header_prototypes
from reef_amd import _ffi, msm


def test_symbols_are_exported_and_declared():
    raw = ctypes.CDLL(_ffi.LIB_PATH)
    protos = header_prototypes()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    lib = _ffi.load()
    for name, nargs in (("reef_ipa_check", 19), ("reef_ipa_check_eq", 20)):
        assert hasattr(raw, name) and hasattr(ctypes.CDLL(_ffi.EXPERIMENT_LIB_PATH), name)
        assert name in _ffi.declared_symbols()
        assert protos[name][0] == "i32" and len(protos[name][1]) == nargs
        assert len(getattr(lib, name).argtypes) == nargs
        assert f"fn {name}(" in doc
    hdr = open(_ffi.HEADER).read()
    assert "(3j)" in hdr and hdr.index("(3i)") < hdr.index("(3j)") < hdr.index("(4) Runtime plumbing")


def test_fails_loudly_without_gpu():
    lib = _ffi.load()
    acc = ctypes.c_uint32(7)
    z = np.zeros(12, dtype=np.uint64)
    a = z.ctypes.data
    # no key, no check: there is no host fallback behind these symbols
    assert lib.reef_ipa_check(None, 4, a, a, a, a, a, a, a, a, 4, 0, None, None, False, ctypes.byref(acc), None, None, None) == 1
    assert lib.reef_ipa_check_eq(None, 4, a, a, a, a, a, a, a, a, a, a, 1, None, None, False, ctypes.byref(acc), None, None, None) == 1
    assert acc.value == 7 and b"null" in lib.reef_last_error()
    if lib.reef_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(msm.ReefError) as e:                 # and the key such a call needs cannot be made
        msm.MsmContext("pallas", np.zeros((4, 8), dtype=np.uint64))
    assert e.value.status == 3


class _Key:
    """stands in for a key ctx where no device call is made"""
    curve = 0
    _lib = None


def test_verify_draws_its_challenges_in_the_oracles_order(monkeypatch):
    """verify_opening against oracle.ipa_oracle.verify_open, verify_eval against prove_eval's order: a recording challenge callable,
    the point operations and the check itself stubbed out."""
    from oracle import ipa_oracle
    from reef_amd import verify
    p = msm.SCALAR_MODULUS[0]
    pt = lambda i: np.full(12, i, dtype=np.uint64)
    monkeypatch.setattr(verify, "compress", lambda key, jac: bytes([int(np.asarray(jac).reshape(-1)[0]) & 0xFF]))
    monkeypatch.setattr(verify, "_lincomb", lambda curve, pts, ks: pt(40 + len(ks)))
    monkeypatch.setattr(verify, "normalize", lambda curve, jac: (np.full((1, 8), 9, dtype=np.uint64), None))
    monkeypatch.setattr(verify, "comm_lz", lambda curve, rows, left, p: pt(50))
    monkeypatch.setattr(ipa_oracle, "compress", lambda curve, jac: bytes([int(np.asarray(jac).reshape(-1)[0]) & 0xFF]))
    monkeypatch.setattr(ipa_oracle, "msm", lambda curve, pts, ks: pt(40 + len(ks)) if len(ks) <= 2 else pt(60))
    monkeypatch.setattr(ipa_oracle.pasta_ref, "scalar_mul", lambda curve, base, k: pt(41))

    def recorder(log):
        def challenge(label, absorbed):
            log.append((label, [bytes(x) if isinstance(x, (bytes, bytearray)) else int(x) for x in absorbed]))
            return 1000 + len(log)
        return challenge
    proof = {"cross": 11, "L": [pt(1), pt(2), pt(3)], "R": [pt(4), pt(5), pt(6)], "a_hat": 12}
    r_x, r_y = [21, 22, 23], [30, 31, 32]                 # n = 8: eq(r_x) has 8 entries, eq(r_y[1:]) 4
    seen = {}

    def stub(key, n, comm, c, q, L, R, rs, a_hat, points, weights, **kw):
        seen.update(n=n, c=c, rs=list(rs), points=[list(x) for x in points], weights=list(weights), a_hat=a_hat, kw=kw)
        return {"accept": True}
    mine, theirs = [], []
    assert verify.verify_opening(_Key(), np.zeros(8, np.uint64), pt(7), r_x, 13, pt(8), r_y, 14, proof, recorder(mine), p, check_fn=stub) is True
    from oracle.spartan_oracle import eq_evals
    try:
        ipa_oracle.verify_open(0, np.zeros((8, 8), np.uint64), np.zeros(8, np.uint64), pt(7), eq_evals(r_x, p), 13, pt(8), eq_evals(r_y[1:], p), 14,
                               proof, recorder(theirs))
    except AssertionError:
        pass                                              # the stubbed points satisfy nothing; the order is what is compared
    assert mine == theirs and [m[0] for m in mine] == ["r", "r"] + ["challenge_r"] * 3
    r = 1001
    assert seen["n"] == 8 and seen["rs"] == [1003, 1004, 1005] and seen["points"] == [r_x, r_y[1:]] and seen["weights"] == [1, r]
    assert seen["c"] == (13 + r * r * 14 + r * 11) % p and seen["a_hat"] == 12
    # verify_eval: "r" after (comm_LZ, eval), then "challenge_r" per round, as reef_amd.hyrax.prove_eval draws them
    log = []
    point = [1, 2, 3, 4, 5]
    qs = []
    assert verify.verify_eval(_Key(), None, b"", point, 2, 77, proof, p, challenge=recorder(log), q_of=lambda r: qs.append(r) or np.zeros(8, np.uint64),
                              check_fn=stub) is True
    assert log == [("r", [bytes([50]), 77])] + [("challenge_r", [bytes([i]), bytes([i + 3])]) for i in (1, 2, 3)]
    assert qs == [1001] and seen["n"] == 8 and seen["points"] == [[3, 4, 5]] and seen["weights"] == [1] and seen["rs"] == [1002, 1003, 1004]
    assert seen["kw"] == {"h": None, "blind": None}
    # with the proof's own challenges, and a blind
    assert verify.verify_eval(_Key(), np.zeros(8, np.uint64), b"", point, 2, 77, dict(proof, rs=[5, 6, 7]), p, h=np.ones(8, np.uint64), blind_total=p + 3,
                              check_fn=stub) is True
    assert seen["rs"] == [5, 6, 7] and seen["kw"]["blind"] == 3 and seen["kw"]["h"] is not None
    # q, the challenges, h and blind_total: what is missing is named, before any device call
    for kw in (dict(q=None), dict(q=None, challenge=recorder([])), dict(proof=proof), dict(h=np.ones(8, np.uint64)), dict(blind_total=3)):
        a = dict(q=np.zeros(8, np.uint64), proof=dict(proof, rs=[5, 6, 7]), challenge=None, h=None, blind_total=None)
        a.update(kw)
        with pytest.raises(ValueError):
            verify.verify_eval(_Key(), a["q"], b"", point, 2, 77, a["proof"], p, h=a["h"], blind_total=a["blind_total"], challenge=a["challenge"],
                               check_fn=stub)
    # a proof with the wrong number of rounds is refused before any device call
    assert verify.verify_eval(_Key(), np.zeros(8, np.uint64), b"", point, 2, 77, dict(proof, L=proof["L"][:2], rs=[5, 6, 7]), p, check_fn=stub) is False
