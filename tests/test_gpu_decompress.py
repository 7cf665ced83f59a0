"""reef_decompress and reef_hyrax_eval_comm_compressed on the GPU (include/reef_msm.h, K4's inverse) against oracle/pasta_oracle.py:
the two square roots at every 2-adic order, the round trip with reef_normalize from host and device memory, the invalid and special
encodings inside one wave, and the Hyrax route from compressed rows -- key sizes on both sides of 1024 points, the reuse of host rows,
a corrupted row, and prove() from either form of the rows."""
import functools
import random

import numpy as np
import pytest

from decompress_inputs import CURVE_OF, FIELDS, R256, check_roots, non_residue_xs, special_batch, sqrt_inputs, to_abi
from gpu_drivers import hyrax_points, key_of_kind
from oracle import pasta_ref
from oracle.ipa_oracle import compress, gens_of
from oracle.pasta_oracle import ap_bases
from oracle.spartan_oracle import Challenger

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 257, 4099]


@pytest.fixture(scope="module")
def field_cases():
    """per field: the inputs of the square-root ops, computed once"""
    return {f: sqrt_inputs(p) for f, p in FIELDS.items()}


@pytest.mark.parametrize("field", [0, 1])
@pytest.mark.parametrize("op", [8, 9], ids=["windowed", "tonelli_shanks"])
def test_square_root_at_every_two_adic_order(gpu_lib, field_cases, field, op):
    """v = r^(2^32) zeta^(m 2^(32 - k)), three per k = 0..32, then 0, 1, 4, p - 1 and 50 random values: out^2 = v with even parity,
    the 0xff marker for the non-residues (k = 32).  Only these inputs reach the short and the empty loops of either root."""
    p, vals = FIELDS[field], field_cases[field]
    a = to_abi([v for v, _ in vals], p)
    out = np.zeros_like(a)
    assert gpu_lib.reef_test_field_op(field, op, a.ctypes.data, a.ctypes.data, out.ctypes.data, len(vals)) == 0
    check_roots(vals, out, p, f"op {op}")


@pytest.mark.parametrize("field", [0, 1])
def test_the_two_roots_give_the_same_bytes(gpu_lib, field_cases, field):
    p, vals = FIELDS[field], field_cases[field]
    a = to_abi([v for v, _ in vals], p)
    outs = [np.zeros_like(a), np.zeros_like(a)]
    for op, out in zip((8, 9), outs):
        assert gpu_lib.reef_test_field_op(field, op, a.ctypes.data, a.ctypes.data, out.ctypes.data, len(vals)) == 0
    assert outs[0].tobytes() == outs[1].tobytes()


@functools.lru_cache(maxsize=None)
def _points_of(curve):
    cv = CURVE_OF[curve]
    encs = [cv.compress(pt) for pt in ap_bases(cv, 7 + curve, 5, max(SIZES))]
    return encs, [cv.affine_to_bytes(cv.decompress(e)) for e in encs]


@pytest.fixture(scope="module")
def curve_points():
    """curve -> 4099 points k G as encodings, and the 64-byte ABI form of decompress(compress(P)) by the oracle; computed once per
    curve (the oracle's 4099 square roots take a few seconds), shared by every case below and never changed"""
    return _points_of


def _jacobian_of(curve, aff: np.ndarray) -> np.ndarray:
    """affine ABI points -> Jacobian with Z = 1 (Montgomery form); (0, 0) -> Z = 0"""
    one = to_abi([1], FIELDS[curve])[0]
    jac = np.zeros((aff.shape[0], 12), np.uint64)
    jac[:, :8] = aff
    jac[aff.any(axis=1), 8:] = one
    return jac


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("where", ["host", "device"])
def test_round_trip_with_normalize(gpu_lib, curve_points, curve, n, where):
    """decompress(compress(P)) byte for byte, and reef_normalize of the result gives the encodings back.  Both parities occur in every
    batch of two or more; a batch of one holds one point, so n = 1 runs once with a point of each parity."""
    from reef_amd import msm
    encs, want = curve_points(curve)
    starts = [0] if n > 1 else [next(i for i, e in enumerate(encs) if e[31] >> 7 == s) for s in (0, 1)]
    seen = set()
    for i0 in starts:
        batch = encs[i0:i0 + n]
        seen |= {e[31] >> 7 for e in batch}
        data = np.frombuffer(b"".join(batch), np.uint8)
        if where == "host":
            aff, bad, first = msm.decompress(curve, data)
        else:
            dbuf, bad, first = msm.decompress(curve, msm.DeviceBuffer.from_host(data), n, loc=msm.REEF_DEVICE)
            aff = dbuf.to_host((n, 8))
        assert (bad, first) == (0, n)
        assert aff.tobytes() == b"".join(want[i0:i0 + n])
        assert msm.normalize(curve, _jacobian_of(curve, aff), affine=False, compressed=True)[1].tobytes() == b"".join(batch)
    assert seen == {0, 1}, "both parities"


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("where", ["host", "device"])
def test_invalid_and_special_encodings_in_one_wave(gpu_lib, curve_points, curve, where):
    from reef_amd import msm
    cv = CURVE_OF[curve]
    if curve == 0:
        assert non_residue_xs(0) == [2, 8, 9, 10]
    encs, want, bad_at = special_batch(curve, [cv.decompress(e) for e in curve_points(curve)[0][:64]])
    assert len(bad_at) == 12 and bad_at[0] == 4
    data = np.frombuffer(b"".join(encs), np.uint8)
    if where == "host":
        aff, bad, first = msm.decompress(curve, data)
    else:
        dbuf, bad, first = msm.decompress(curve, msm.DeviceBuffer.from_host(data), 64)
        aff = dbuf.to_host((64, 8))
    assert (bad, first) == (len(bad_at), bad_at[0])
    assert not aff[bad_at].any(), "(0, 0) at the invalid slots"
    assert aff.tobytes() == b"".join(want), "the neighbours of an invalid entry are bit-exact"
    good = [e for i, e in enumerate(encs) if i not in bad_at]
    _, bad, first = msm.decompress(curve, b"".join(good))
    assert (bad, first) == (0, len(good))


def _encode(curve, aff: np.ndarray) -> bytes:
    """affine ABI points -> their 32-byte encodings, on the host"""
    cv, p = CURVE_OF[curve], FIELDS[curve]
    rinv = pow(R256, -1, p)
    out = []
    for row in aff:
        raw = row.tobytes()
        x, y = (int.from_bytes(raw[k:k + 32], "little") * rinv % p for k in (0, 32))
        out.append(cv.compress((x, y)))
    return b"".join(out)


def _hyrax(curve, left, seed):
    """the smallest document with 2^left rows (two columns), its key, a point and 2^left row commitments"""
    from reef_amd.hyrax import HyraxEval
    p = FIELDS[1 - curve]
    rng = random.Random(seed)
    num_vars = left + 1
    z = np.random.default_rng(seed).integers(0, 256, size=1 << num_vars, dtype=np.uint64).astype(np.uint8)
    point = [rng.randrange(p) for _ in range(num_vars)]
    rows = pasta_ref.gen_bases_ap(curve, 1000 + seed, 3, 1 << left)
    return HyraxEval(curve, z, num_vars, left), key_of_kind(curve, gens_of(curve, 2)[0], "plain"), point, rows


@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("left", [3, 7, 11])
def test_eval_comm_from_compressed_rows(gpu_lib, curve, left):
    """2^3, 2^7 and 2^11 rows: comms keys on both sides of 1024 points.  Host and device rows, the same host bytes twice, then one
    corrupted row -- REEF_ERR_ARG naming it, and the ctx still serves the rows it had and new ones."""
    from reef_amd.msm import DeviceBuffer, ReefError
    hx, key, point, rows = _hyrax(curve, left, 20 + left)
    enc = _encode(curve, rows)
    other = np.ascontiguousarray(rows[::-1])
    with hx, key:
        hx.eval_begin(key, point)
        want = compress(curve, hx.eval_comm(rows))
        want_other = compress(curve, hx.eval_comm(other))
        assert want != want_other
        assert compress(curve, hx.eval_comm_compressed(enc)) == want, "host rows"
        assert compress(curve, hx.eval_comm_compressed(enc)) == want, "the same host bytes again"
        assert compress(curve, hx.eval_comm_compressed(DeviceBuffer.from_host(np.frombuffer(_encode(curve, other), np.uint8)))) == want_other, "device rows"
        assert compress(curve, hx.eval_comm_compressed(enc)) == want, "host rows after device rows"
        j = (1 << left) - 3
        x = non_residue_xs(curve)[1]
        bad = enc[:32 * j] + (x | 1 << 255).to_bytes(32, "little") + enc[32 * (j + 1):]
        with pytest.raises(ReefError, match=rf"row {j} ") as e:
            hx.eval_comm_compressed(bad)
        assert e.value.status == 1
        assert compress(curve, hx.eval_comm_compressed(enc)) == want, "the rows of before the failure"
        assert compress(curve, hx.eval_comm_compressed(_encode(curve, other))) == want_other, "new rows after the failure"
        assert compress(curve, hx.eval_comm(rows)) == want, "affine rows after compressed ones"
        assert compress(curve, hx.eval_comm_compressed(_encode(curve, other))) == want_other, "compressed rows after affine ones"


@pytest.mark.parametrize("curve", [0, 1])
def test_prove_from_compressed_rows_is_the_proof_from_affine_rows(gpu_lib, curve):
    from reef_amd import hyrax
    hx, key, point, rows = _hyrax(curve, 4, 44)
    p = FIELDS[1 - curve]
    q0, _ = hyrax_points(curve)

    def q_of(r):
        return pasta_ref.to_affine(curve, pasta_ref.scalar_mul(curve, q0, r))[0]
    with hx, key:
        a = hyrax.prove(hx, key, point, Challenger(p, 6), p, q_of, row_comms=rows)
        b = hyrax.prove(hx, key, point, Challenger(p, 6), p, q_of, row_comms_compressed=_encode(curve, rows))
        with pytest.raises(ValueError):
            hyrax.prove(hx, key, point, Challenger(p, 6), p, q_of, row_comms=rows, row_comms_compressed=_encode(curve, rows))
    assert compress(curve, a["comm_lz"]) == compress(curve, b["comm_lz"])
    for k in ("eval", "lz_blind", "r_ipa", "rs", "a_hat", "b_hat"):
        assert a[k] == b[k], k
    for k in ("L", "R"):
        assert [compress(curve, x) for x in a[k]] == [compress(curve, x) for x in b[k]], k
