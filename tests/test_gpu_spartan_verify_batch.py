"""The verifier's matrix evaluations at many points in one pass (include/reef_msm.h 3o: reef_spartan_eval_matrices_batch) on the device,
bit for bit against the big-integer model of tests/spartan_verify_model.py and against the single call (3k) on the same ctx: every
small Spartan shape and the 257-row straddle shape, both curves, both forms, m = 1, 2, 3, 5; each point in both slots of a pair; rows on
each side of the short / long / segment cuts in each slot; groups under a workspace budget; m = 0; argument errors; batches in the
middle of a prove and of an opening; a replaced matrix; and verify_sumchecks_batch on device-made proofs."""
import functools
import random

import numpy as np
import pytest

from gpu_drivers import PROOF_KEYS, key_of_kind, open_shape, opening_instances, prove_dev, set_running, upload_shape
from oracle.ipa_oracle import compress, gens_of, open_ref
from oracle.r1cs_oracle import relaxed_instance
from oracle.spartan_oracle import Challenger, prove_ref
from reef_amd._fe import _arr, _ints
from spartan_verify_model import (STRADDLE_PADS, bits, comm_ops, ells, forms, model_evals, named_instance, named_shape, random_point, replayable,
                                  straddle_shape, tamperings)

pytestmark = pytest.mark.gpu

SMALL = ["smallest", "dup_empty", "long_row", "vars_lt_cons", "io_close"]


def _shape(curve, name):
    return (straddle_shape(curve, False), STRADDLE_PADS) if name == "straddle" else named_shape(curve, name)


@functools.lru_cache(maxsize=None)
def _case(curve, name):
    """(shape, pads, five random points, the model at each): computed once per shape"""
    shape, pads = _shape(curve, name)
    pts = [random_point(pads, shape["p"], 100 + 7 * k + curve) for k in range(5)]
    return shape, pads, pts, [model_evals(shape, pads[1], *pt) for pt in pts]


def _nifs(curve, shape, is_mont=False):
    from reef_amd.nifs import Nifs
    nf = Nifs(curve, shape["num_cons"], shape["num_vars"], shape["num_io"])
    upload_shape(nf, shape, is_mont)
    return nf


def _dev(nf, pads, r_x, r_y, p, is_mont=False):
    from reef_amd.verify import matrix_evals
    to, frm = forms(p, is_mont)
    return [frm(v) for v in matrix_evals(nf, pads[0], pads[1], [to(v) for v in r_x], [to(v) for v in r_y], is_mont=is_mont)]


def _batch(nf, pads, points, p, is_mont=False):
    from reef_amd.verify import matrix_evals_batch
    to, frm = forms(p, is_mont)
    got = matrix_evals_batch(nf, pads[0], pads[1], [([to(v) for v in r_x], [to(v) for v in r_y]) for r_x, r_y in points], is_mont=is_mont)
    return [[frm(v) for v in ev] for ev in got]


def _per_point(shape):
    return (shape["num_cons"] + shape["num_vars"] + 1 + shape["num_io"]) * 32


# ------------------------------------------------------------------------------------------------ 1. the model and the single call
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("name", SMALL + ["straddle"])
def test_batch_matches_the_model_and_the_single_call(gpu_lib, curve, name):
    shape, pads, pts, want = _case(curve, name)
    p = shape["p"]
    for is_mont in (False, True):
        form = "Montgomery" if is_mont else "canonical"
        with _nifs(curve, shape, is_mont) as nf:
            assert [_dev(nf, pads, *pt, p, is_mont) for pt in pts] == want, f"single calls before any batch ({form})"
            for m in (1, 2, 3, 5):
                assert _batch(nf, pads, pts[:m], p, is_mont) == want[:m], f"m = {m} ({form})"
                assert [_dev(nf, pads, *pt, p, is_mont) for pt in pts[:m]] == want[:m], f"single calls after m = {m} ({form})"


# ------------------------------------------------------------------------------------------------ 2. a point's slot does not matter
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("name", ["dup_empty", "long_row"])
def test_a_point_gives_the_same_values_in_either_slot_of_a_pair(gpu_lib, curve, name):
    shape, pads, pts, want = _case(curve, name)
    p = shape["p"]
    ell_x, ell_y = ells(pads)
    rng = random.Random(5 + curve)
    with _nifs(curve, shape) as nf:
        assert _batch(nf, pads, pts[:4], p) == want[:4]
        assert _batch(nf, pads, [pts[4]] + pts[:4], p) == [want[4]] + want[:4]      # every point moved to the other slot
        for m in (2, 5):
            assert _batch(nf, pads, [pts[1]] * m, p) == [want[1]] * m               # both slots at once, and the odd last point
        for is_mont in (False, True):
            corner = ([rng.choice([0, 1, p - 1]) for _ in range(ell_x)], [rng.choice([0, 1, p - 1]) for _ in range(ell_y)])
            cw = model_evals(shape, pads[1], *corner)
            assert _batch(nf, pads, [corner, pts[2]], p, is_mont) == [cw, want[2]]
            assert _batch(nf, pads, [pts[2], corner], p, is_mont) == [want[2], cw]


# ------------------------------------------------------------------------------------------------ 3. rows that straddle each cut, in each slot
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("c_empty", [False, True])
def test_rows_on_each_side_of_the_cuts_in_each_slot(gpu_lib, curve, c_empty):
    shape, pads = straddle_shape(curve, c_empty), STRADDLE_PADS
    p = shape["p"]
    ell_x, _ = ells(pads)
    r_x, r_y = random_point(pads, p, 7 + curve)
    rows = (0, 1, 2, 3, 4, 131, 254, 256)                # long, short, empty-in-C and last-block rows: one row alone per point
    pts = [(bits(row, ell_x), r_y) for row in rows]
    want = [model_evals(shape, pads[1], *pt) for pt in pts]
    first = model_evals(shape, pads[1], r_x, r_y)
    assert c_empty == (first[2] == 0)
    with _nifs(curve, shape) as nf:
        for got, w, row in zip(_batch(nf, pads, pts, p), want, rows):
            assert got == w, f"row {row}"
        shifted = _batch(nf, pads, [(r_x, r_y)] + pts, p)
        assert shifted[0] == first
        for got, w, row in zip(shifted[1:], want, rows):
            assert got == w, f"row {row}, other slot"


# ------------------------------------------------------------------------------------------------ 4. groups under a workspace budget
@pytest.mark.parametrize("curve", [0, 1])
def test_groups_give_the_same_results_under_any_budget(gpu_lib, curve):
    shape, pads, pts, want = _case(curve, "long_row")
    p, per = shape["p"], _per_point(shape)
    pts7, want7 = pts + pts[:2], want + want[:2]
    with _nifs(curve, shape) as nf:
        # (budget, G): whole pairs when more than one point fits; 0 is the default, far above seven points of this shape
        for budget, G in ((5 * per + 31, 4), (per, 1), (2 * per, 2), (3 * per + 1, 2), (1, 1), (0, 7), (per - 1, 1), (64 * per, 7)):
            nf.set_eval_workspace(budget)
            assert _batch(nf, pads, pts7, p) == want7, f"budget {budget}"
            info = nf.eval_batch_last_info()
            assert (info["groups"], info["points_per_group"]) == (-(-7 // G), G), f"budget {budget}"
            assert G * per <= info["workspace_bytes"] <= max(budget or 1 << 30, per), f"budget {budget}"
        nf.set_eval_workspace(2 * per)
        assert _batch(nf, pads, pts[:1], p) == want[:1]                                # fewer points than a group holds
        assert nf.eval_batch_last_info() == {"groups": 1, "points_per_group": 1, "workspace_bytes": per}


# ------------------------------------------------------------------------------------------------ 5. m = 0
@pytest.mark.parametrize("curve", [0, 1])
def test_an_empty_batch_writes_nothing(gpu_lib, curve):
    from reef_amd._ffi import ReefError
    from reef_amd.verify import matrix_evals_batch
    shape, pads, pts, want = _case(curve, "dup_empty")
    out = np.full((3, 4), 7, dtype=np.uint64)
    with _nifs(curve, shape) as nf:
        assert nf._lib.reef_spartan_eval_matrices_batch(nf._h, pads[0], pads[1], None, None, 0, False, out.ctypes.data) == 0
        assert nf._lib.reef_spartan_eval_matrices_batch(nf._h, pads[0], pads[1], None, None, 0, True, None) == 0
        assert (out == 7).all()
        assert matrix_evals_batch(nf, pads[0], pads[1], []) == []
        with pytest.raises(ReefError) as e:                  # an empty batch is no batch
            nf.eval_batch_last_info()
        assert e.value.status == 1
        assert _batch(nf, pads, pts[:2], shape["p"]) == want[:2]
        assert nf.eval_batch_last_info()["groups"] == 1


# ------------------------------------------------------------------------------------------------ 6. errors
def _raw(nf, ncp, nvp, points, m, out, *, null=None, is_mont=False):
    """the C call on host arrays of its own; null: the argument passed as NULL.  (status, message)"""
    xa = _arr([x for r_x, _ in points for x in r_x])
    ya = _arr([y for _, r_y in points for y in r_y])
    args = {"r_x": xa.ctypes.data, "r_y": ya.ctypes.data, "evals": out.ctypes.data}
    if null:
        args[null] = None
    st = nf._lib.reef_spartan_eval_matrices_batch(nf._h, ncp, nvp, args["r_x"], args["r_y"], m, is_mont, args["evals"])
    return st, nf._lib.reef_last_error().decode()


@pytest.mark.parametrize("curve", [0, 1])
def test_argument_errors_leave_the_outputs_and_the_ctx_alone(gpu_lib, curve):
    from reef_amd.nifs import Nifs
    shape, pads, pts, want = _case(curve, "vars_lt_cons")                 # 500 rows, 253 + 1 + 3 columns, pads (512, 512)
    p = shape["p"]
    out = np.full((3 * 5, 4), 7, dtype=np.uint64)

    def refused(st_msg, *words):
        st, msg = st_msg
        assert st == 1 and all(w in msg for w in words), (st, msg, words)
        assert (out == 7).all(), msg
        assert _batch(nf, pads, pts, p) == want, f"the batch after: {msg}"

    with Nifs(curve, shape["num_cons"], shape["num_vars"], shape["num_io"]) as nf:
        for k, m in enumerate("AB"):                     # C is still missing
            nf.set_matrix(k, *shape[m][:2], _arr(shape[m][2]))
        st, msg = _raw(nf, pads[0], pads[1], pts, 5, out)
        assert st == 1 and "matri" in msg and (out == 7).all()
        upload_shape(nf, shape, False)
        assert _batch(nf, pads, pts, p) == want
        bad = [(list(r_x), list(r_y)) for r_x, r_y in pts]
        bad[3][1][4] = p                                   # the modulus itself, in point 3's r_y
        refused(_raw(nf, pads[0], pads[1], bad, 5, out), "point 3", "r_y", "not below the modulus")
        bad = [(list(r_x), list(r_y)) for r_x, r_y in pts]
        bad[4][0][0] = (1 << 256) - 1
        refused(_raw(nf, pads[0], pads[1], bad, 5, out), "point 4", "r_x", "not below the modulus")
        refused(_raw(nf, pads[0], pads[1], [pts[0]] * 4097, 4097, out), "4097", "4096")
        for ncp, nvp in ((256, 512), (512, 128), (768, 512), (1, 512), (512, 1 << 25)):
            refused(_raw(nf, ncp, nvp, pts, 5, out), "reef_spartan_eval_matrices_batch: need powers of two")
        for null in ("r_x", "r_y", "evals"):
            refused(_raw(nf, pads[0], pads[1], pts, 5, out, null=null), "null")


# ------------------------------------------------------------------------------------------------ 7. in the middle of a prove
@pytest.mark.parametrize("curve", [0, 1])
def test_batches_inside_a_prove_and_an_opening_change_nothing(gpu_lib, curve):
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
    pts = [random_point(pads, p, 4 + k) for k in range(3)]
    want = [model_evals(shape, pads[1], *pt) for pt in pts]
    inner = Challenger(p, curve)
    calls = []

    with key_of_kind(curve, gens, "pre") as key, _nifs(curve, shape) as nf:
        set_running(nf, inst, p, False)

        def hooked(label, absorbed):                     # every challenge is drawn between two device calls of the prove
            m = 2 + len(calls) % 2
            assert _batch(nf, pads, pts[:m], p, len(calls) % 4 >= 2) == want[:m], f"before challenge {len(calls)} ({label})"
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


# ------------------------------------------------------------------------------------------------ 8. a matrix replaced; the workspace grows
@pytest.mark.parametrize("curve", [0, 1])
def test_a_replaced_matrix_is_seen_and_the_workspace_grows(gpu_lib, curve):
    shape, pads, pts, want = _case(curve, "long_row")
    p, per = shape["p"], _per_point(shape)
    with _nifs(curve, shape) as nf:
        assert _batch(nf, pads, pts[:1], p) == want[:1]
        assert nf.eval_batch_last_info() == {"groups": 1, "points_per_group": 1, "workspace_bytes": per}
        assert _batch(nf, pads, pts[:4], p) == want[:4]
        assert nf.eval_batch_last_info() == {"groups": 1, "points_per_group": 4, "workspace_bytes": 4 * per}
        assert _batch(nf, pads, pts[:2], p) == want[:2]                                # and does not shrink under the same budget
        assert nf.eval_batch_last_info() == {"groups": 1, "points_per_group": 2, "workspace_bytes": 4 * per}
        rows, cols, vals = shape["B"]
        other = dict(shape, B=(rows[::2], cols[::2], [(v + 1) % p for v in vals[::2]]), A=shape["C"], C=shape["A"])   # the long row moves to C
        upload_shape(nf, other, False)
        moved = [model_evals(other, pads[1], *pt) for pt in pts[:3]]
        assert moved != want[:3]
        assert _batch(nf, pads, pts[:3], p) == moved
        assert _dev(nf, pads, *pts[0], p) == moved[0]


# ------------------------------------------------------------------------------------------------ 9. the batched verifier
@pytest.mark.parametrize("curve", [0, 1])
def test_verify_sumchecks_batch_on_device_proofs(gpu_lib, curve):
    from reef_amd.verify import verify_sumchecks_batch
    name = "dup_empty"
    shape, pads = named_shape(curve, name)
    inst, p = named_instance(curve, name), shape["p"]
    with _nifs(curve, shape) as nf:
        set_running(nf, inst, p, False)
        pfs = [prove_dev(nf, shape, pads, False, seed) for seed in (8, 9, 10)]

    def instances(proofs, us=None):
        return [{"u": inst["u"] if us is None else us[i], "X": inst["X"], "proof": replayable(pf), "challenge": Challenger(p, 8 + i)}
                for i, pf in enumerate(proofs)]
    with _nifs(curve, shape) as vf:                       # the verifier's own ctx: matrices only
        assert verify_sumchecks_batch(vf, pads[0], pads[1], instances(pfs), p) == [True, True, True]
        assert vf.eval_batch_last_info()["points_per_group"] == 3
        for at, pick in ((0, "claims_inner[0]"), (1, "inner round"), (2, "claims_outer[1]"), (1, "u")):
            what, bad, u, X = next(t for t in tamperings(pfs[at], inst["u"], inst["X"], p) if t[0] == pick)
            proofs, us = list(pfs), [inst["u"]] * 3
            proofs[at], us[at] = bad, u
            assert verify_sumchecks_batch(vf, pads[0], pads[1], instances(proofs, us), p) == [i != at for i in range(3)], what
