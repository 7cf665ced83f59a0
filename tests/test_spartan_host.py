"""Row N5 on the host: the big-integer reference of the two sum-checks of the final SNARK (oracle/spartan_oracle.py) checked
against the verifier's own identities -- every round's g(0) + g(1) equals the running claim, both final claims hold with every term
evaluated straight from the unpadded shape, and a broken row makes the outer identity fail; the library's new symbols."""
import pytest

from oracle.r1cs_oracle import fresh_instance, layered_shape, relaxed_instance, running_from_fresh
from oracle.spartan_oracle import Challenger, check_pads, eq_at, eq_evals, next_pow2, padded_z, prove_ref, renumber, verify


# ---------------------------------------------------------------------------------------------------------------- tests
def test_padding_and_renumbering():
    shape = layered_shape(0, 5, num_inputs=2, num_io=3, seed=2)
    nv = shape["num_vars"]
    assert renumber(nv - 1, nv, 16) == nv - 1 and renumber(nv, nv, 16) == 16 and renumber(nv + 3, nv, 16) == 19
    inst = running_from_fresh(fresh_instance(shape, 1), 5)
    z = padded_z(inst, 16)
    assert len(z) == 32 and z[:nv] == inst["W"] and z[nv:16] == [0] * (16 - nv) and z[16] == 1 and z[17:20] == inst["X"] and z[20:] == [0] * 12
    assert check_pads(shape, 8, 16) and not check_pads(shape, 4, 16) and not check_pads(shape, 8, 12) and not check_pads(shape, 8, 4)
    assert not check_pads(shape, 8, nv) or nv & (nv - 1) == 0
    ev = eq_evals([3, 5], shape["p"])
    p = shape["p"]
    assert ev == [(1 - 3) * (1 - 5) % p, (1 - 3) * 5 % p, 3 * (1 - 5) % p, 15]        # tau_0 on the most significant bit


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("kw,pads", [
    (dict(num_cons=1, num_inputs=2, num_io=1), (2, 4)),
    (dict(num_cons=37, dup_every=3, empty_every=5, extra_vars=4), None),
    (dict(num_cons=20, num_inputs=3, num_io=2, extra_vars=0), (32, 64)),              # num_vars < num_cons; num_vars_pad > num_vars
    (dict(num_cons=24, num_inputs=4, num_io=9, extra_vars=2), None),                   # num_io close to num_vars_pad
    (dict(num_cons=40, long_row=300, num_io=2), None),
])
def test_reference_prove_satisfies_the_verifier(curve, kw, pads):
    shape = layered_shape(curve, seed=len(kw) + curve, **kw)
    inst = relaxed_instance(shape, 2, 5 + curve)
    assert inst["u"] != 1 and (any(inst["E"]) or shape["num_cons"] == 1)    # one constraint: its cross terms may cancel
    ncp, nvp = pads or (next_pow2(shape["num_cons"]), next_pow2(max(shape["num_vars"], shape["num_io"] + 1)))
    pf = prove_ref(shape, inst, ncp, nvp, Challenger(shape["p"], curve))
    assert len(pf["outer"]) == ncp.bit_length() - 1 and len(pf["inner"]) == nvp.bit_length()
    verify(shape, inst, ncp, nvp, pf, Challenger(shape["p"], curve))
    assert pf["outer_final"] == eq_at(pf["tau"], pf["r_x"], shape["p"]) * (
        pf["claims_outer"][0] * pf["claims_outer"][1] - inst["u"] * pf["claims_outer"][2] - pf["claims_outer"][3]) % shape["p"]


@pytest.mark.parametrize("curve", [0, 1])
def test_a_broken_row_fails_the_outer_identity(curve):
    shape = layered_shape(curve, 30, num_io=2, extra_vars=3, seed=9 + curve)
    p = shape["p"]
    inst = relaxed_instance(shape, 1, 3)
    k = next(i for i in range(30) if shape["plan"][i] is not None)
    bad = dict(inst, E=list(inst["E"]))
    bad["E"][k] = (bad["E"][k] + 1) % p
    pf = prove_ref(shape, bad, 32, next_pow2(shape["num_vars"]), Challenger(p), strict=False)
    verify(shape, inst, 32, next_pow2(shape["num_vars"]), prove_ref(shape, inst, 32, next_pow2(shape["num_vars"]), Challenger(p)), Challenger(p))
    with pytest.raises(AssertionError, match="outer final claim"):
        verify(shape, bad, 32, next_pow2(shape["num_vars"]), pf, Challenger(p))


def test_library_exports_the_spartan_symbols():
    from reef_amd import _ffi
    lib = _ffi.load()
    for name in ("reef_spartan_begin", "reef_spartan_outer_round", "reef_spartan_outer_claims", "reef_spartan_inner_begin",
                 "reef_spartan_inner_round", "reef_spartan_inner_claims"):
        assert hasattr(lib, name), name
        assert name in _ffi.declared_symbols()
    assert lib.reef_abi_version() == _ffi.ABI_VERSION
