"""The late rounds of the resident arguments on a folded key (reef_hyrax_set_small_key, reef_spartan_open_set_small_key).

Each argument runs on the same inputs and the same challenges with the switch off and with n_small in {n / 2, 8, 1} (n_small = 1 and
any n_small >= n never switch: those runs are the unswitched one).  Every L and R must be the same point (compared after
reef_normalize, as 32-byte encodings), a_hat, b_hat, c and the reads of a and b between rounds the same values bit for bit, and
reef_ipa_check_eq must accept the switched proof.  The Hyrax argument: num_vars 8, 11 and 12 (16 and 64 columns) over 1-byte symbols, with
and without the h blind term, on a small pre-shifted and on a plain source key, and one 2^22-symbol document whose 2048 columns put a
pre-shifted bucket-pipeline key at the source and a 1024-point nibble-table key after the switch.  The batched opening: a 2^6 and a 2^8
shape, both curves, a pre-shifted and a plain source key."""
import random

import numpy as np
import pytest

from gpu_drivers import hyrax_points, key_of_kind, set_running, upload_shape
from oracle import pasta_ref
from oracle.hyrax_oracle import blind_total
from oracle.ipa_oracle import affine, gens_of, msm as ref_msm
from oracle.r1cs_oracle import field, layered_shape, relaxed_instance
from oracle.spartan_oracle import Challenger, next_pow2
from reef_amd._fe import _arr

pytestmark = pytest.mark.gpu


def _enc(curve, pts):
    from reef_amd import msm
    return [msm.compress(curve, x) for x in pts]


def _run_hyrax(hx, key, point, q, h, blinds, rs, n_small):
    hx.set_small_key(n_small)
    out = {"begin": hx.eval_begin(key, point), "lz": hx.read(0, 1 << hx.right), "L": [], "R": [], "reads": []}
    bl = (lambda k: list(blinds[k])) if h is not None else (lambda k: None)
    L, R = hx.ipa_begin(q, h, bl(0))
    length = 1 << hx.right
    for k, r in enumerate(rs[:-1]):
        out["L"].append(L)
        out["R"].append(R)
        L, R = hx.ipa_round(r, bl(k + 1))
        length //= 2
        out["reads"].append((hx.read(0, length), hx.read(1, length)))
    out["L"].append(L)
    out["R"].append(R)
    out["hats"] = hx.finish(rs[-1])
    return out


def _same_argument(curve, off, on, what):
    assert _enc(curve, on["L"]) == _enc(curve, off["L"]), f"L ({what})"
    assert _enc(curve, on["R"]) == _enc(curve, off["R"]), f"R ({what})"
    for key in ("begin", "lz", "reads", "hats"):
        assert on[key] == off[key], f"{key} ({what})"


def _hyrax_case(curve, num_vars, with_h, kind, n_smalls):
    from reef_amd.hyrax import HyraxEval
    from reef_amd.verify import ipa_check_eq
    p = field(curve)
    left = num_vars // 2
    right = num_vars - left
    n = 1 << right
    gens, _ = gens_of(curve, n)
    q, h = hyrax_points(curve)
    rng = random.Random(1000 * num_vars + 10 * curve + with_h)
    point = [rng.randrange(p) for _ in range(num_vars)]
    rs = [rng.randrange(1, p) for _ in range(right)]
    blinds = [(rng.randrange(p), rng.randrange(p) if k % 2 else 0) for k in range(right)] if with_h else None
    z = np.random.default_rng(num_vars + curve).integers(0, 256, size=(1 << num_vars) - 3, dtype=np.uint64).astype(np.uint8)
    hh = h if with_h else None
    with key_of_kind(curve, gens, kind) as key, HyraxEval(curve, z, num_vars, left) as hx:
        off = _run_hyrax(hx, key, point, q, hh, blinds, rs, 0)
        comm = key.msm(_arr(off["lz"]), is_mont=False)
        kw = dict(h=h, blind=blind_total(0, blinds, rs, p)) if with_h else {}
        for ns in n_smalls:
            on = _run_hyrax(hx, key, point, q, hh, blinds, rs, ns)
            _same_argument(curve, off, on, f"n = {n}, n_small = {ns}, {kind} key")
            got = ipa_check_eq(key, n, comm, on["begin"][0], q, on["L"], on["R"], rs, on["hats"][0], [point[left:]], [1], **kw)
            assert got["accept"] is True, f"the proof with n_small = {ns} is refused"
        _same_argument(curve, off, _run_hyrax(hx, key, point, q, hh, blinds, rs, 0), "switched off again")


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("num_vars", [8, 11, 12])
@pytest.mark.parametrize("with_h", [False, True])
def test_hyrax_argument_is_the_same_on_a_folded_key(gpu_lib, curve, num_vars, with_h):
    n = 1 << (num_vars - num_vars // 2)
    kind = "pre" if (num_vars + with_h) % 2 else "plain"
    _hyrax_case(curve, num_vars, with_h, kind, sorted({n // 2, 8, 1, n, 4 * n}))


def test_hyrax_argument_from_a_bucket_pipeline_key_to_a_nibble_table_key(gpu_lib):
    """2048 columns: the source key is served by the bucket pipeline, the folded key of 1024 points by its nibble tables"""
    _hyrax_case(0, 22, False, "pre", [1024, 8])


def _run_opening(curve, shape, pads, inst, kind, gens, q, r_fold, rs, n_small):
    from reef_amd.nifs import Nifs
    from reef_amd.spartan import Opening, prove
    p = shape["p"]
    with key_of_kind(curve, gens, kind) as key, Nifs(curve, shape["num_cons"], shape["num_vars"], shape["num_io"]) as nf:
        upload_shape(nf, shape, False)
        set_running(nf, inst, p, False)
        out = {"sumchecks": prove(nf, pads[0], pads[1], Challenger(p, 3), p), "L": [], "R": [], "reads": []}
        op = Opening(nf)
        op.set_small_key(n_small)
        out["cross"] = op.begin(key)
        out["c"] = op.fold(r_fold)
        L, R = op.ipa_begin(q)
        length = max(pads)
        for r in rs[:-1]:
            out["L"].append(L)
            out["R"].append(R)
            L, R = op.ipa_round(r)
            length //= 2
            out["reads"].append((op.read(0, length), op.read(1, length)))
        out["L"].append(L)
        out["R"].append(R)
        out["hats"] = (op.finish(rs[-1]), op.read(1, 1))
    return out


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("num_cons", [50, 200])          # n = 2^6 and 2^8
@pytest.mark.parametrize("kind", ["pre", "plain"])
def test_opening_is_the_same_on_a_folded_key(gpu_lib, curve, num_cons, kind):
    from reef_amd.verify import ipa_check_eq
    shape = layered_shape(curve, num_cons, num_inputs=3, num_io=2, seed=60 + curve)
    pads = (next_pow2(shape["num_cons"]), next_pow2(max(shape["num_vars"], shape["num_io"] + 1)))
    p, n = shape["p"], max(pads)
    assert n == {50: 64, 200: 256}[num_cons]
    inst = relaxed_instance(shape, 1, 21 + curve)
    gens, gens_s = gens_of(curve, n)
    rng = random.Random(num_cons + curve)
    r_fold = rng.randrange(1, p)
    rs = [rng.randrange(1, p) for _ in range(n.bit_length() - 1)]
    q = affine(curve, pasta_ref.scalar_mul(curve, gens_s, rng.randrange(1, p)))
    off = _run_opening(curve, shape, pads, inst, kind, gens, q, r_fold, rs, 0)
    E, W = list(inst["E"]), list(inst["W"])
    comm_a = ref_msm(curve, np.stack([ref_msm(curve, gens[:len(E)], E), ref_msm(curve, gens[:len(W)], W)]), [1, r_fold])
    r_x, r_y = off["sumchecks"]["r_x"], off["sumchecks"]["r_y"]
    for ns in sorted({n // 2, 8, 1, n}):
        on = _run_opening(curve, shape, pads, inst, kind, gens, q, r_fold, rs, ns)
        _same = f"n = {n}, n_small = {ns}, {kind} key"
        assert _enc(curve, on["L"]) == _enc(curve, off["L"]) and _enc(curve, on["R"]) == _enc(curve, off["R"]), "L, R " + _same
        for name in ("sumchecks", "cross", "c", "reads", "hats"):
            assert on[name] == off[name], f"{name} ({_same})"
        with key_of_kind(curve, gens, "pre") as key:
            got = ipa_check_eq(key, n, comm_a, on["c"], q, on["L"], on["R"], rs, on["hats"][0], [list(r_x), list(r_y[1:])], [1, r_fold])
        assert got["accept"] is True, f"the opening with n_small = {ns} is refused"


def test_setters_reject_what_is_not_a_power_of_two(gpu_lib):
    from reef_amd.hyrax import HyraxEval
    from reef_amd.msm import ReefError
    from reef_amd.nifs import Nifs
    from reef_amd.spartan import Opening
    with HyraxEval(0, np.arange(16, dtype=np.uint8), 4) as hx, Nifs(0, 4, 4, 1) as nf:
        for bad in (3, 6, 1000, (1 << 20) + 1):
            with pytest.raises(ReefError) as e:
                hx.set_small_key(bad)
            assert e.value.status == 1
            with pytest.raises(ReefError) as e:
                Opening(nf).set_small_key(bad)
            assert e.value.status == 1
        for good in (0, 1, 2, 1 << 20):
            hx.set_small_key(good)
            Opening(nf).set_small_key(good)
