"""The verifier's matrix evaluations on the device (include/reef_msm.h 3k: reef_spartan_eval_matrices) and the verifier functions of
reef_amd.verify on top of it, bit for bit against the big-integer model of tests/spartan_verify_model.py: every Spartan shape, both
curves, both forms; 0/1 and edge-value points; rows that straddle the short / long / segment cuts; a ctx without a witness; calls in the
middle of a prove and of an opening; argument errors; and the sum-check and SNARK verifiers on device-made proofs."""
import random

import pytest

from gpu_drivers import PROOF_KEYS, SPARTAN_SHAPES, key_of_kind, open_shape, opening_instances, prove_dev, set_running, upload_shape
from oracle.ipa_oracle import compress, gens_of, msm, open_ref
from oracle.r1cs_oracle import relaxed_instance
from oracle.spartan_oracle import Challenger, prove_ref, renumber
from reef_amd._fe import _arr, _ints
from spartan_verify_model import (STRADDLE_PADS, bits, combine, comm_ops, ells, entry_sums, forms, model_evals, named_instance, named_prove,
                                  named_shape, random_point, replayable, straddle_shape, tamperings)

pytestmark = pytest.mark.gpu


def _nifs(curve, shape, is_mont=False):
    from reef_amd.nifs import Nifs
    nf = Nifs(curve, shape["num_cons"], shape["num_vars"], shape["num_io"])
    upload_shape(nf, shape, is_mont)
    return nf


def _dev(nf, pads, r_x, r_y, p, is_mont=False):
    from reef_amd.verify import matrix_evals
    to, frm = forms(p, is_mont)
    return [frm(v) for v in matrix_evals(nf, pads[0], pads[1], [to(v) for v in r_x], [to(v) for v in r_y], is_mont=is_mont)]


# ------------------------------------------------------------------------------------------------ 1. the Spartan shapes
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("name", list(SPARTAN_SHAPES))
def test_matches_the_model_on_every_spartan_shape(gpu_lib, curve, name):
    shape, pads = named_shape(curve, name)
    p = shape["p"]
    points = [random_point(pads, p, 31 + curve)]
    want = [model_evals(shape, pads[1], *points[0])]
    if name != "cfg4":                                   # the prover's own point: the verifier's combination is the prover's claim
        pf = named_prove(curve, name, 5)
        points.append((pf["r_x"], pf["r_y"]))
        want.append(model_evals(shape, pads[1], pf["r_x"], pf["r_y"]))
        assert combine(want[1], pf["r"], p) == pf["claims_inner"][0]
    for is_mont in (False, True):
        with _nifs(curve, shape, is_mont) as nf:           # matrices only: no running instance
            for (r_x, r_y), w in zip(points, want):
                assert _dev(nf, pads, r_x, r_y, p, is_mont) == w, f"{'Montgomery' if is_mont else 'canonical'} form"


# ------------------------------------------------------------------------------------------------ 2. corner points
def _positions(shape):
    """(row, col) of an entry with a duplicate, one in the u column, one in an X column, and an absent position"""
    nv = shape["num_vars"]
    seen, dup, ucol, xcol = set(), None, None, None
    for m in "ABC":
        mseen = set()
        for r, c, _ in zip(*shape[m]):
            if (r, c) in mseen and dup is None:
                dup = (r, c)
            mseen.add((r, c))
            if c == nv and ucol is None:
                ucol = (r, c)
            if c > nv and xcol is None:
                xcol = (r, c)
        seen |= mseen
    absent = next((r, c) for r in range(shape["num_cons"]) for c in (nv, 0, nv + 1) if (r, c) not in seen)
    assert dup and ucol and xcol
    return {"duplicate": dup, "u column": ucol, "X column": xcol, "absent": absent}


@pytest.mark.parametrize("curve", [0, 1])
def test_corner_points(gpu_lib, curve):
    shape, pads = named_shape(curve, "dup_empty")
    p, nv = shape["p"], shape["num_vars"]
    ell_x, ell_y = ells(pads)
    rng = random.Random(3 + curve)
    with _nifs(curve, shape) as nf:
        for what, (row, col) in _positions(shape).items():
            got = _dev(nf, pads, bits(row, ell_x), bits(renumber(col, nv, pads[1]), ell_y), p)
            assert got == entry_sums(shape, row, col), what
            assert any(got) == (what != "absent")
        for is_mont in (False, True):
            for _ in range(3):                           # 0, 1 and p - 1 among random entries, r_y[0] among them
                r_x = [rng.choice([0, 1, p - 1, rng.randrange(p)]) for _ in range(ell_x)]
                r_y = [rng.choice([0, 1, p - 1])] + [rng.choice([0, 1, p - 1, rng.randrange(p), rng.randrange(p)]) for _ in range(ell_y - 1)]
                assert _dev(nf, pads, r_x, r_y, p, is_mont) == model_evals(shape, pads[1], r_x, r_y)


# ------------------------------------------------------------------------------------------------ 3. rows that straddle each cut
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("c_empty", [False, True])
def test_rows_that_straddle_the_cuts(gpu_lib, curve, c_empty):
    shape, pads = straddle_shape(curve, c_empty), STRADDLE_PADS
    p = shape["p"]
    ell_x, ell_y = ells(pads)
    with _nifs(curve, shape) as nf:
        r_x, r_y = random_point(pads, p, 7 + curve)
        want = model_evals(shape, pads[1], r_x, r_y)
        assert c_empty == (want[2] == 0)
        assert _dev(nf, pads, r_x, r_y, p) == want
        assert _dev(nf, pads, r_x, r_y, p, True) == want
        for row in (0, 1, 2, 3, 4, 131, 254, 256):       # one row alone (r_x on its bits): each side of each cut by itself
            got = _dev(nf, pads, bits(row, ell_x), r_y, p)
            assert got == model_evals(shape, pads[1], bits(row, ell_x), r_y), f"row {row}"


# ------------------------------------------------------------------------------------------------ 4. a verifier's ctx
@pytest.mark.parametrize("curve", [0, 1])
def test_ctx_without_a_witness_and_a_matrix_replaced(gpu_lib, curve):
    from reef_amd._ffi import ReefError
    from reef_amd.nifs import W
    shape, pads = named_shape(curve, "long_row")
    p = shape["p"]
    r_x, r_y = random_point(pads, p, 9)
    with _nifs(curve, shape) as nf:
        assert _dev(nf, pads, r_x, r_y, p) == model_evals(shape, pads[1], r_x, r_y)
        with pytest.raises(ReefError):
            nf.read(W)                                   # there is no running instance, and the call made none
        rows, cols, vals = shape["B"]
        other = dict(shape, B=(rows[::2], cols[::2], [(v + 1) % p for v in vals[::2]]), A=shape["C"], C=shape["A"])   # the long row moves to C
        upload_shape(nf, other, False)
        want = model_evals(other, pads[1], r_x, r_y)
        assert want != model_evals(shape, pads[1], r_x, r_y)
        assert _dev(nf, pads, r_x, r_y, p) == want


# ------------------------------------------------------------------------------------------------ 5. in the middle of a prove
@pytest.mark.parametrize("curve", [0, 1])
def test_calls_inside_a_prove_and_an_opening_change_nothing(gpu_lib, curve):
    from reef_amd.nifs import E, U, W, X
    from reef_amd.spartan import prove_with_opening
    shape, pads = open_shape(curve, "cons_gt_vars")
    p, n = shape["p"], max(pads)
    inst = relaxed_instance(shape, 1, 11 + curve)
    gens, gens_s = gens_of(curve, n)
    ch = Challenger(p, curve)
    ref = prove_ref(shape, inst, pads[0], pads[1], ch)
    i1, i2 = opening_instances(curve, shape, inst, ref, gens)
    oref = open_ref(curve, gens, gens_s, i1, i2, ch)
    comm_a, q_of = comm_ops(curve, i1["comm"], i2["comm"], gens_s)
    r_x, r_y = random_point(pads, p, 4)
    want = model_evals(shape, pads[1], r_x, r_y)
    inner = Challenger(p, curve)
    calls = []

    with key_of_kind(curve, gens, "pre") as key, _nifs(curve, shape) as nf:
        set_running(nf, inst, p, False)

        def hooked(label, absorbed):                     # every challenge is drawn between two device calls of the prove
            assert _dev(nf, pads, r_x, r_y, p, len(calls) % 2 == 1) == want, f"before challenge {len(calls)} ({label})"
            calls.append(label)
            return inner(label, absorbed)
        got = prove_with_opening(nf, key, pads[0], pads[1], hooked, p, comm_a, q_of)
        assert calls.count("r") == 3 and calls.count("challenge_r") == n.bit_length() - 1      # outer_claims | inner_begin, and every IPA round
        for k in PROOF_KEYS:
            assert got[k] == ref[k], k
        assert (got["cross_term"], got["c"], got["a_hat"], got["r_ipa_rounds"]) == (oref["cross"], oref["c"], oref["a_hat"], oref["rs"])
        assert [compress(curve, x) for x in got["L"] + got["R"]] == [compress(curve, x) for x in oref["L"] + oref["R"]]
        assert _ints(nf.read(W)) == inst["W"] and _ints(nf.read(E)) == inst["E"]
        assert _ints(nf.read(U)) == [inst["u"]] and _ints(nf.read(X)) == inst["X"]
        assert nf.check_relaxed() == (0, None)


# ------------------------------------------------------------------------------------------------ 6. errors
@pytest.mark.parametrize("curve", [0, 1])
def test_argument_errors_leave_the_ctx_usable(gpu_lib, curve):
    from reef_amd._ffi import ReefError
    from reef_amd.nifs import Nifs
    from reef_amd.verify import matrix_evals
    shape, pads = named_shape(curve, "vars_lt_cons")                 # 500 rows, 253 + 1 + 3 columns, pads (512, 512)
    p = shape["p"]
    r_x, r_y = random_point(pads, p, 2)
    want = model_evals(shape, pads[1], r_x, r_y)

    def point(ncp, nvp):
        return [1] * max(ncp.bit_length() - 1, 1), [2] * max(nvp.bit_length(), 1)
    with Nifs(curve, shape["num_cons"], shape["num_vars"], shape["num_io"]) as nf:
        for k, m in enumerate("AB"):                     # C is still missing
            nf.set_matrix(k, *shape[m][:2], _arr(shape[m][2]))
        with pytest.raises(ReefError) as e:
            matrix_evals(nf, pads[0], pads[1], r_x, r_y)
        assert e.value.status == 1 and "matri" in str(e.value)
        upload_shape(nf, shape, False)
        assert _dev(nf, pads, r_x, r_y, p) == want
        for ncp, nvp in ((256, 512), (512, 128), (768, 512), (512, 384), (1, 512), (512, 1), (0, 512), (1 << 25, 512), (512, 1 << 25)):
            with pytest.raises(ReefError) as e:
                matrix_evals(nf, ncp, nvp, *point(ncp, nvp))
            assert e.value.status == 1 and "reef_spartan_eval_matrices: need powers of two" in str(e.value), (ncp, nvp)
        for bad_x, bad_y in (([p] + r_x[1:], r_y), (r_x, r_y[:-1] + [p]), (r_x[:-1] + [(1 << 256) - 1], r_y), (r_x, [p] + r_y[1:])):
            with pytest.raises(ReefError) as e:
                matrix_evals(nf, pads[0], pads[1], bad_x, bad_y)
            assert e.value.status == 1 and "not below the modulus" in str(e.value)
        assert _dev(nf, pads, r_x, r_y, p) == want
    with Nifs(curve, 100, 4, 3) as small:                # num_io must stay below num_vars_pad
        with pytest.raises(ReefError):
            matrix_evals(small, 128, 2, [0] * 7, [0] * 2)


# ------------------------------------------------------------------------------------------------ 7. the verifier functions
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("name", ["smallest", "dup_empty", "io_close"])
def test_verify_sumchecks_on_device_proofs(gpu_lib, curve, name):
    from reef_amd.verify import verify_sumchecks
    shape, pads = named_shape(curve, name)
    inst, p = named_instance(curve, name), shape["p"]
    with _nifs(curve, shape) as nf:
        set_running(nf, inst, p, False)
        pf = prove_dev(nf, shape, pads, False, 8)
    with _nifs(curve, shape) as vf:                       # the verifier's own ctx: matrices only
        assert verify_sumchecks(vf, pads[0], pads[1], inst["u"], inst["X"], replayable(pf), Challenger(p, 8), p) is True
        assert verify_sumchecks(vf, pads[0], pads[1], inst["u"], inst["X"], pf, Challenger(p, 8), p) is True
        for what, bad, u, X in tamperings(pf, inst["u"], inst["X"], p):
            assert verify_sumchecks(vf, pads[0], pads[1], u, X, replayable(bad), Challenger(p, 8), p) is False, what


@pytest.mark.parametrize("curve", [0, 1])
def test_verify_snark_on_a_device_proof(gpu_lib, curve):
    from reef_amd.spartan import prove_with_opening
    from reef_amd.verify import verify_snark
    shape, pads = open_shape(curve, "vars_gt_cons")
    p, n = shape["p"], max(pads)
    inst = relaxed_instance(shape, 1, 11 + curve)
    gens, gens_s = gens_of(curve, n)
    E, W = list(inst["E"]), list(inst["W"])
    comm_e, comm_w = msm(curve, gens[:len(E)], E), msm(curve, gens[:len(W)], W)
    comm_a, q_of = comm_ops(curve, comm_e, comm_w, gens_s)
    with key_of_kind(curve, gens, "pre") as key:
        with _nifs(curve, shape) as nf:
            set_running(nf, inst, p, False)
            got = prove_with_opening(nf, key, pads[0], pads[1], Challenger(p, 7), p, comm_a, q_of)
        with _nifs(curve, shape) as vf:
            args = (vf, key, gens_s, comm_e, comm_w, pads[0], pads[1], inst["u"], inst["X"])
            assert verify_snark(*args, got, Challenger(p, 7), p) is True
            assert verify_snark(*args, dict(got, a_hat=(got["a_hat"] + 1) % p), Challenger(p, 7), p) is False
            bad = dict(got, claims_inner=[got["claims_inner"][0], got["claims_inner"][1], (got["claims_inner"][2] + 1) % p])
            assert verify_snark(*args, bad, Challenger(p, 7), p) is False
