"""The Hyrax consistency argument on the GPU (reef_amd.hyrax over include/reef_msm.h 3i) against the big-integer reference of
oracle/hyrax_oracle.py, bit-exact call by call: eval, lz_blind, comm_LZ, every round's L and R (compressed), a_hat, b_hat and a, b
between rounds; both curves and input forms, symbols of 1 / 2 / 4 bytes and field elements, the three key kinds, with and without
row blinds and the per-round h term; a cfg4-sized 2^25 document; a after eval_begin against reef_mle_bound_rows; the device
transcript through the reference verifier; the order and key errors and the restart; a 3h opening interleaved with an argument."""
import random

import numpy as np
import pytest

from gpu_drivers import (hyrax_points, key_of_kind, open_shape, opening_instances, row_comms, run_hyrax, set_running,
                         upload_shape)
from oracle import pasta_ref
from oracle.hyrax_oracle import blind_total, hyrax_ref, verify_hyrax
from oracle.ipa_oracle import compress, gens_of, msm, open_ref
from oracle.r1cs_oracle import field, relaxed_instance
from oracle.spartan_oracle import Challenger, eq_evals, prove_ref
from reef_amd._fe import _arr

pytestmark = pytest.mark.gpu

_SYM = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def _doc(curve, eb, n, seed, is_mont=False):
    """(what the device takes, the entries as ints): symbols of eb bytes, or field elements (is_mont form)"""
    p = field(curve)
    rng = np.random.default_rng(seed)
    if eb != 32:
        top = {1: 256, 2: 65536, 4: 1 << 32}[eb]
        z = rng.integers(0, top, size=n, dtype=np.uint64).astype(_SYM[eb])
        return z, [int(v) for v in z]
    r = random.Random(seed)
    ints = [r.randrange(p) for _ in range(n)]
    return _arr([v * (1 << 256) % p for v in ints] if is_mont else ints), ints


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("eb", [1, 2, 4, 32])
@pytest.mark.parametrize("num_vars", [2, 5, 10])
def test_argument_bit_exact_against_the_reference(gpu_lib, curve, eb, num_vars):
    from reef_amd.hyrax import HyraxEval
    p = field(curve)
    left = num_vars // 2
    right = num_vars - left
    n = (1 << num_vars) - (num_vars % 3)
    gens, _ = gens_of(curve, 1 << right)
    q, h = hyrax_points(curve)
    rng = random.Random(100 * eb + num_vars + curve)
    point = [rng.randrange(p) for _ in range(num_vars)]
    mode = (eb + num_vars) % 3                           # 0 plain, 1 row blinds, 2 row blinds and the h term
    row_blinds = [rng.randrange(p) for _ in range(1 << left)] if mode else None
    blinds = [(rng.randrange(p), rng.randrange(p) if k % 2 else 0) for k in range(right)] if mode == 2 else None
    with key_of_kind(curve, gens, "pre") as key:
        for is_mont in (False, True):
            z, ints = _doc(curve, eb, n, 7 * num_vars + eb, is_mont)
            rc = row_comms(curve, gens, ints, num_vars, left, row_blinds, h)
            ref = hyrax_ref(curve, gens, ints, num_vars, left, point, q, Challenger(p, num_vars), p, row_blinds=row_blinds,
                            h=h if mode == 2 else None, blinds=blinds, row_comms=rc)
            R = (1 << 256) % p
            rb = [v * R % p for v in row_blinds] if (row_blinds and is_mont) else row_blinds
            with HyraxEval(curve, z, num_vars, left, row_blinds=rb, is_mont=is_mont) as hx:
                run_hyrax(hx, key, ref, curve, point, q, is_mont=is_mont, h=h if mode == 2 else None, blinds=blinds)
                assert compress(curve, hx.eval_comm(rc)) == compress(curve, ref["comm_lz"]), "comm_LZ"
                b0 = eq_evals(point[left:], p)
                total = blind_total(ref["lz_blind"], blinds or [], ref["rs"], p)
                verify_hyrax(curve, gens, q, ref["comm_lz"], ref["eval"], b0, ref, p, h=h if mode else None, lz_blind_total=total)


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("with_h", [False, True])
def test_key_kinds_give_the_same_argument(gpu_lib, curve, with_h):
    """The pre-shifted bucket key, byte tables and a plain key (host window combine): c q and the h term enter each route."""
    from reef_amd.hyrax import HyraxEval
    p = field(curve)
    num_vars, left = 13, 2                               # 2^11 columns: the byte-table range
    right = num_vars - left
    gens, _ = gens_of(curve, 1 << right)
    q, h = hyrax_points(curve)
    rng = random.Random(40 + curve)
    point = [rng.randrange(p) for _ in range(num_vars)]
    blinds = [(rng.randrange(p), rng.randrange(p)) for _ in range(right)] if with_h else None
    z, ints = _doc(curve, 1, 1 << num_vars, 3)
    ref = hyrax_ref(curve, gens, ints, num_vars, left, point, q, Challenger(p, 9), p, h=h if with_h else None, blinds=blinds)
    with HyraxEval(curve, z, num_vars, left) as hx:
        for kind in ("pre", "tables", "plain"):
            with key_of_kind(curve, gens, kind) as key:
                run_hyrax(hx, key, ref, curve, point, q, is_mont=False, h=h if with_h else None, blinds=blinds, trace=kind == "pre")


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("eb", [1, 2, 4, 32])
def test_a_after_eval_begin_is_mle_bound_rows(gpu_lib, curve, eb):
    from reef_amd import mle
    from reef_amd.hyrax import HyraxEval
    p = field(curve)
    num_vars, left = 12, 5
    z, ints = _doc(curve, eb, (1 << num_vars) - 5, eb + 20)
    rng = random.Random(eb)
    point = [rng.randrange(p) for _ in range(num_vars)]
    lz, ev = mle.bound_rows(curve, z if eb != 32 else ints, point, left)
    gens, _ = gens_of(curve, 1 << (num_vars - left))
    with key_of_kind(curve, gens, "plain") as key, HyraxEval(curve, z, num_vars, left) as hx:
        got, _ = hx.eval_begin(key, point)
        assert got == ev
        assert hx.read(0, 1 << (num_vars - left)) == lz


def _lz_symbols(z, num_vars, left, point, p):
    """LZ of a 1-byte symbol document on the host, independent of the library: L split into 16-bit limbs, each limb row times Z as
    an exact float64 product (4096 x 255 x 2^16 < 2^53), the limbs put back together as big integers"""
    rows, cols = 1 << left, 1 << (num_vars - left)
    zz = np.zeros(1 << num_vars, dtype=np.float64)
    zz[:len(z)] = z
    zz = zz.reshape(rows, cols)
    L = eq_evals(point[:left], p)
    limbs = np.array([[(v >> (16 * k)) & 0xFFFF for v in L] for k in range(16)], dtype=np.float64)   # 16 x rows
    acc = np.zeros((16, cols), dtype=np.float64)
    for i0 in range(0, rows, 512):
        acc += limbs[:, i0:i0 + 512] @ zz[i0:i0 + 512]
    acc = acc.astype(np.uint64)
    return [sum(int(acc[k, j]) << (16 * k) for k in range(16)) % p for j in range(cols)]


def test_cfg4_sized_document(gpu_lib):
    """A 2^25-symbol document (R = 2^13, cfg4): a and eval against a host LZ the library has no part in (and against
    reef_mle_bound_rows), then every round against the reference"""
    from reef_amd import mle
    from reef_amd.hyrax import HyraxEval, factored_lens
    curve, num_vars = 0, 25
    p = field(curve)
    left, right = factored_lens(num_vars)
    assert (left, right) == (12, 13)
    z, _ = _doc(curve, 1, (1 << num_vars) - 1000, 25)
    rng = random.Random(25)
    point = [rng.randrange(p) for _ in range(num_vars)]
    lz = _lz_symbols(z, num_vars, left, point, p)
    ev = sum(x * y for x, y in zip(lz, eq_evals(point[left:], p))) % p
    assert mle.bound_rows(curve, z, point, left) == (lz, ev)
    gens, _ = gens_of(curve, 1 << right)
    q, h = hyrax_points(curve)
    blinds = [(rng.randrange(p), rng.randrange(p)) for _ in range(right)]
    ref = hyrax_ref(curve, gens, None, num_vars, left, point, q, Challenger(p, 25), p, h=h, blinds=blinds, lz=lz)
    assert ref["eval"] == ev
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, z, num_vars) as hx:
        run_hyrax(hx, key, ref, curve, point, q, is_mont=False, h=h, blinds=blinds, trace=False)
        hx.eval_begin(key, point)
        assert hx.read(0, 1 << right) == lz
    comm = msm(curve, gens, lz)
    verify_hyrax(curve, gens, q, comm, ev, eq_evals(point[left:], p), ref, p, h=h, lz_blind_total=blind_total(0, blinds, ref["rs"], p))


@pytest.mark.parametrize("curve", [0, 1])
def test_device_transcript_passes_the_verifier(gpu_lib, curve):
    """prove_eval drives the whole argument with its own challenges; the reference verifier accepts what the device returned"""
    from reef_amd.hyrax import HyraxEval, prove_eval
    p = field(curve)
    num_vars, left = 9, 4
    right = num_vars - left
    gens, _ = gens_of(curve, 1 << right)
    q0, h = hyrax_points(curve)
    rng = random.Random(77 + curve)
    point = [rng.randrange(p) for _ in range(num_vars)]
    row_blinds = [rng.randrange(p) for _ in range(1 << left)]
    blinds = [(rng.randrange(p), rng.randrange(p)) for _ in range(right)]
    z, ints = _doc(curve, 32, 1 << num_vars, 77)
    rc = row_comms(curve, gens, ints, num_vars, left, row_blinds, h)

    def q_of(r):
        return pasta_ref.to_affine(curve, pasta_ref.scalar_mul(curve, q0, r))[0]
    for is_mont in (False, True):
        with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, z, num_vars, left, row_blinds=row_blinds) as hx:
            pf = prove_eval(hx, key, point, Challenger(p, 3), p, q_of, row_comms=rc, h=h, blinds_of=lambda k: blinds[k], is_mont=is_mont)
        q = q_of(pf["r_ipa"])
        total = blind_total(pf["lz_blind"], blinds, pf["rs"], p)
        verify_hyrax(curve, gens, q, pf["comm_lz"], pf["eval"], eq_evals(point[left:], p), pf, p, h=h, lz_blind_total=total)
        bad = dict(pf, a_hat=(pf["a_hat"] + 1) % p)
        with pytest.raises(AssertionError, match="P_hat"):
            verify_hyrax(curve, gens, q, pf["comm_lz"], pf["eval"], eq_evals(point[left:], p), bad, p, h=h, lz_blind_total=total)


def test_order_key_and_restart_errors(gpu_lib):
    from reef_amd._ffi import ReefError
    from reef_amd.hyrax import HyraxEval
    curve, num_vars, left = 0, 8, 4
    p = field(curve)
    gens, _ = gens_of(curve, 16)
    q, h = hyrax_points(curve)
    z, ints = _doc(curve, 2, 200, 5)
    rng = random.Random(5)
    point = [rng.randrange(p) for _ in range(num_vars)]
    ref = hyrax_ref(curve, gens, ints, num_vars, left, point, q, Challenger(p, 1), p)
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, z, num_vars, left) as hx:
        with pytest.raises(ReefError, match="reef_hyrax_eval_begin"):
            hx.ipa_begin(q)
        with pytest.raises(ReefError, match="reef_hyrax_eval_begin"):
            hx.read(0, 1)
        with pytest.raises(ReefError, match="reef_hyrax_eval_begin"):
            hx.eval_comm(np.zeros((16, 8), np.uint64))
        with key_of_kind(curve, gens[:8], "pre") as short, pytest.raises(ReefError, match="8 points.*exactly 2\\^\\(num_vars - left_vars\\) = 16"):
            hx.eval_begin(short, point)
        with key_of_kind(1, gens_of(1, 16)[0], "pre") as other, pytest.raises(ReefError, match="curve 1"):
            hx.eval_begin(other, point)
        with pytest.raises(ReefError, match="below the modulus"):
            hx.eval_begin(key, [p] + point[1:])
        hx.eval_begin(key, point)
        with pytest.raises(ReefError, match="out of order, the next call is reef_hyrax_ipa_begin"):
            hx.ipa_round(ref["rs"][0])
        hx.ipa_begin(q)
        with pytest.raises(ReefError, match="out of order, the next call is reef_hyrax_ipa_round"):
            hx.finish(ref["rs"][0])
        with pytest.raises(ReefError, match="took no h term"):
            hx.ipa_round(ref["rs"][0], [1, 2])
        with pytest.raises(ReefError, match="zero"):
            hx.ipa_round(0)
        hx.ipa_round(ref["rs"][0])
        run_hyrax(hx, key, ref, curve, point, q, is_mont=False)            # a second eval_begin mid-argument starts over
        with pytest.raises(ReefError, match="out of order, the next call is reef_hyrax_eval_begin"):
            hx.ipa_round(ref["rs"][0])
        run_hyrax(hx, key, ref, curve, point, q, is_mont=True)


def test_interleaved_with_a_3h_opening(gpu_lib):
    """A 3h opening on a NIFS ctx and a 3i argument on a Hyrax ctx, call for call in turn, give what each gives alone"""
    from reef_amd.hyrax import HyraxEval
    from reef_amd.nifs import Nifs
    from reef_amd.spartan import Opening, prove
    curve = 0
    shape, pads = open_shape(curve, "cons_gt_vars")
    p, n = shape["p"], max(pads)
    inst = relaxed_instance(shape, 1, 11)
    gens3, gens_s = gens_of(curve, n)
    ch = Challenger(p, 0)
    pf = prove_ref(shape, inst, pads[0], pads[1], ch)
    i1, i2 = opening_instances(curve, shape, inst, pf, gens3)
    ref3 = open_ref(curve, gens3, gens_s, i1, i2, ch)
    num_vars = 2 * (n.bit_length() - 1)
    left = num_vars // 2
    gens, _ = gens_of(curve, 1 << (num_vars - left))
    q, h = hyrax_points(curve)
    rng = random.Random(8)
    point = [rng.randrange(p) for _ in range(num_vars)]
    blinds = [(rng.randrange(p), rng.randrange(p)) for _ in range(num_vars - left)]
    z, ints = _doc(curve, 1, 1 << num_vars, 8)
    ref = hyrax_ref(curve, gens, ints, num_vars, left, point, q, Challenger(p, 8), p, h=h, blinds=blinds)
    assert len(ref["rs"]) == len(ref3["rs"])
    with key_of_kind(curve, gens3, "pre") as key3, key_of_kind(curve, gens, "plain") as key, HyraxEval(curve, z, num_vars, left) as hx, \
            Nifs(curve, shape["num_cons"], shape["num_vars"], shape["num_io"]) as nf:
        upload_shape(nf, shape, False)
        set_running(nf, inst, p, False)
        prove(nf, pads[0], pads[1], Challenger(p, 0), p)
        op = Opening(nf)
        assert op.begin(key3) == ref3["cross"]
        assert hx.eval_begin(key, point)[0] == ref["eval"]
        assert op.fold(ref3["r"]) == ref3["c"]
        outs3 = [op.ipa_begin(ref3["q"])]
        outs = [hx.ipa_begin(q, h, blinds[0])]
        for k in range(len(ref["rs"]) - 1):
            outs3.append(op.ipa_round(ref3["rs"][k]))
            outs.append(hx.ipa_round(ref["rs"][k], blinds[k + 1]))
        assert op.finish(ref3["rs"][-1]) == ref3["a_hat"]
        assert hx.finish(ref["rs"][-1]) == (ref["a_hat"], ref["b_hat"])
    for got, want in ((outs3, ref3), (outs, ref)):
        assert [compress(curve, L) for L, _ in got] == [compress(curve, x) for x in want["L"]]
        assert [compress(curve, R) for _, R in got] == [compress(curve, x) for x in want["R"]]


@pytest.mark.parametrize("eb", [1, 2, 4, 32])
def test_document_from_device_memory(gpu_lib, eb):
    """z in device memory (z_loc = REEF_DEVICE): the same argument as from host memory"""
    from reef_amd.hyrax import HyraxEval
    from reef_amd.msm import DeviceBuffer
    curve, num_vars, left = 0, 9, 4
    p = field(curve)
    z, ints = _doc(curve, eb, (1 << num_vars) - 7, 90 + eb)
    dz = DeviceBuffer.from_host(z.view(np.uint8))
    rng = random.Random(eb)
    point = [rng.randrange(p) for _ in range(num_vars)]
    gens, _ = gens_of(curve, 1 << (num_vars - left))
    q, _ = hyrax_points(curve)
    ref = hyrax_ref(curve, gens, ints, num_vars, left, point, q, Challenger(p, eb), p)
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, dz, num_vars, left, n=len(ints), elem_bytes=eb) as hx:
        assert hx.elem_bytes == eb and hx.n == len(ints)
        run_hyrax(hx, key, ref, curve, point, q, is_mont=False)
    for n, e in ((len(ints) + 1, eb), (len(ints), None), (len(ints), 8)):     # more than the buffer holds, no width, a bad width
        with pytest.raises(ValueError):
            HyraxEval(curve, dz, num_vars, left, n=n, elem_bytes=e)


def test_tall_matrix_with_row_blinds(gpu_lib):
    """left_vars = 15 (2^15 rows of two columns): the blinds' one-column table runs several rows per chunk"""
    from reef_amd.hyrax import HyraxEval
    curve, num_vars, left = 1, 16, 15
    p = field(curve)
    z, ints = _doc(curve, 1, (1 << num_vars) - 11, 16)
    rng = random.Random(16)
    point = [rng.randrange(p) for _ in range(num_vars)]
    row_blinds = [rng.randrange(p) for _ in range(1 << left)]
    gens, _ = gens_of(curve, 2)
    q, _ = hyrax_points(curve)
    ref = hyrax_ref(curve, gens, ints, num_vars, left, point, q, Challenger(p, 16), p, row_blinds=row_blinds)
    with key_of_kind(curve, gens, "plain") as key, HyraxEval(curve, z, num_vars, left, row_blinds=row_blinds) as hx:
        run_hyrax(hx, key, ref, curve, point, q, is_mont=False)


def test_eval_comm_reuses_and_replaces_the_row_commitments(gpu_lib):
    from reef_amd.hyrax import HyraxEval
    curve, num_vars, left = 0, 8, 4
    p = field(curve)
    gens, _ = gens_of(curve, 16)
    z, ints = _doc(curve, 1, 256, 31)
    rc = row_comms(curve, gens, ints, num_vars, left, None, None)
    other = np.ascontiguousarray(rc[::-1])
    rng = random.Random(31)
    point = [rng.randrange(p) for _ in range(num_vars)]
    L = eq_evals(point[:left], p)
    with key_of_kind(curve, gens, "pre") as key, HyraxEval(curve, z, num_vars, left) as hx:
        hx.eval_begin(key, point)
        for comms in (rc, rc, other, rc):
            assert compress(curve, hx.eval_comm(comms)) == compress(curve, msm(curve, comms, L))
