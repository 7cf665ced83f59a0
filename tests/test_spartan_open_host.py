"""The batched IPA opening of the final SNARK on the host (include/reef_msm.h 3h): the big-integer reference of
oracle/ipa_oracle.py checked by the matching verifier -- it folds the two instances itself, rebuilds P_hat and compares it with
a_hat <s, G> + a_hat <s, b> Q, and a changed L, R, a_hat, cross term or batch order makes the check fail; the library's new symbols."""
import numpy as np
import pytest

from oracle.ipa_oracle import affine, dot, gens_of, msm, open_ref, pad, random_instances, s_vector, verify_open
from oracle.r1cs_oracle import field
from oracle.spartan_oracle import Challenger
from reef_amd._fe import _arr, _ints


def verify_pf(curve, gens, gens_s, i1, i2, pf, seed):
    verify_open(curve, gens, gens_s, i1["comm"], i1["b"], i1["eval"], i2["comm"], i2["b"], i2["eval"], pf, Challenger(field(curve), seed))


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("logn", range(1, 11))
def test_reference_opening_satisfies_the_verifier(curve, logn):
    n = 1 << logn
    gens, gens_s = gens_of(curve, n)
    n1, n2 = (n, max(2, n // 2)) if logn % 2 else (max(2, n // 4), n)        # both padding directions
    i1, i2 = random_instances(curve, n1, n2, gens, 10 * logn + curve)
    pf = open_ref(curve, gens, gens_s, i1, i2, Challenger(field(curve), logn))
    assert len(pf["L"]) == logn and len(pf["trace"][-1]["a"]) == 1
    q = field(curve)
    b0 = [(x + pf["r"] * y) % q for x, y in zip(pad(i1["b"], n), pad(i2["b"], n))]
    assert pf["b_hat"] == dot(s_vector(pf["rs"], q), b0, q)
    verify_pf(curve, gens, gens_s, i1, i2, pf, logn)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("what", ["L", "R", "a_hat", "cross", "order"])
def test_tampering_fails_the_verifier(curve, what):
    p, n = field(curve), 16
    gens, gens_s = gens_of(curve, n)
    i1, i2 = random_instances(curve, 16, 8, gens, 3 + curve)
    if what == "order":                                          # the prover batched [W, E]; the verifier checks [E, W]
        pf = open_ref(curve, gens, gens_s, i2, i1, Challenger(p, 5))
    else:
        pf = open_ref(curve, gens, gens_s, i1, i2, Challenger(p, 5))
        verify_pf(curve, gens, gens_s, i1, i2, pf, 5)
        pf = dict(pf, L=list(pf["L"]), R=list(pf["R"]))
        if what in ("L", "R"):
            pf[what][1] = msm(curve, np.stack([affine(curve, pf[what][1]), gens[0]]), [1, 1])
        elif what == "a_hat":
            pf["a_hat"] = (pf["a_hat"] + 1) % p
        else:
            pf["cross"] = (pf["cross"] + 1) % p
    with pytest.raises(AssertionError, match="P_hat"):
        verify_pf(curve, gens, gens_s, i1, i2, pf, 5)


def test_s_vector_folds_like_the_generators():
    p = field(0)
    rs = [3, 5]
    s = s_vector(rs, p)
    i3, i5 = pow(3, -1, p), pow(5, -1, p)
    assert s == [i3 * i5 % p, i3 * 5 % p, 3 * i5 % p, 15]
    b = [11, 12, 13, 14]
    f = [(b[i] * i3 + b[2 + i] * 3) % p for i in range(2)]
    assert (f[0] * i5 + f[1] * 5) % p == dot(s, b, p)


def test_library_exports_the_opening_symbols():
    from reef_amd import _ffi
    lib = _ffi.load()
    for name in ("reef_spartan_open_begin", "reef_spartan_open_fold", "reef_spartan_open_ipa_begin", "reef_spartan_open_ipa_round",
                 "reef_spartan_open_finish", "reef_spartan_open_read"):
        assert hasattr(lib, name), name
        assert name in _ffi.declared_symbols()
    assert lib.reef_abi_version() == _ffi.ABI_VERSION == 7


def test_array_helpers_round_trip():
    vals = [0, 1, field(1) - 1]
    assert _ints(_arr(vals)) == vals
