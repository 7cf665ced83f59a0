"""Inputs and reference decoding shared by tests/test_decompress_host.py and tests/test_gpu_decompress.py."""
import random

import numpy as np

from oracle.pasta_oracle import CURVES, P, Q, sqrt_mod

R256 = 1 << 256
FIELDS = {0: P, 1: Q}                       # the field numbers of reef_test_field_op; curve c has base field c
CURVE_OF = {0: CURVES["pallas"], 1: CURVES["vesta"]}
MARKER = b"\xff" * 32                       # what the square-root ops return for a non-residue


def zeta(p: int) -> int:
    """a generator of the 2^32 subgroup: g^T for the least non-residue g, p - 1 = 2^32 T"""
    g = 2
    while pow(g, (p - 1) // 2, p) != p - 1:
        g += 1
    return pow(g, (p - 1) >> 32, p)


def two_adic_inputs(p: int, k: int, count: int = 3, seed: int = 0):
    """count values v = r^(2^32) zeta^(m 2^(32 - k)), m odd: v^T has order exactly 2^k in the 2^32 subgroup (k = 0..32), so a
    Tonelli-Shanks loop over v runs k levels deep; k = 32 is a non-residue.  Random curve points never reach k < 18."""
    rng = random.Random(1000 * k + seed)
    z = zeta(p)
    out = []
    for _ in range(count):
        r, m = rng.randrange(1, p), rng.randrange(1 << 32) | 1
        e = (m << (32 - k)) % (1 << 32)
        out.append(pow(r, 1 << 32, p) * pow(z, e, p) % p)
    return out


def sqrt_inputs(p: int, seed: int = 5):
    """[(v, k or None)]: three values of every 2-adic order, then 0, 1, 4, p - 1 and 50 random values"""
    rng = random.Random(seed)
    vals = [(v, k) for k in range(33) for v in two_adic_inputs(p, k, 3, seed)]
    return vals + [(v, None) for v in [0, 1, 4, p - 1] + [rng.randrange(p) for _ in range(50)]]


def to_abi(vals, p: int) -> np.ndarray:
    """canonical integers -> (n, 4) uint64 limbs in the ABI's Montgomery form"""
    return np.array([[(v * R256 % p >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def check_roots(vals, out: np.ndarray, p: int, what: str) -> None:
    """out[i] (ABI form) is the even root of vals[i] = (v, k), or the marker for a non-residue"""
    rinv = pow(R256, -1, p)
    for i, (v, k) in enumerate(vals):
        raw = out[i].tobytes()
        residue = (k < 32) if k is not None else sqrt_mod(v, p) is not None
        if not residue:
            assert raw == MARKER, f"{what}: entry {i} (k = {k}) is a non-residue"
            continue
        m = int.from_bytes(raw, "little")
        assert raw != MARKER and m < p, f"{what}: entry {i} (k = {k})"
        y = m * rinv % p
        assert y * y % p == v and y % 2 == 0, f"{what}: entry {i} (k = {k}): not the even root"


def decode_ref(curve: int, enc: bytes):
    """(point or None for the identity, valid) by oracle.pasta_oracle.Curve.decompress, whose assertions are the invalid cases"""
    try:
        return CURVE_OF[curve].decompress(enc), True
    except AssertionError:
        return None, False


def non_residue_xs(curve: int, count: int = 4):
    """the first small x with no point on the curve (Pallas: 2, 8, 9, 10)"""
    p = FIELDS[curve]
    return [x for x in range(1, 200) if sqrt_mod(x ** 3 + 5, p) is None][:count]


def special_batch(curve: int, points):
    """64 encodings that interleave valid points with the identity, x = p, x = p + 1, 32 x 0xff, 00..80 and four small non-residue
    x under both sign bits; returns (the encodings, the expected 64-byte ABI points, the indices of the invalid ones)"""
    cv, p = CURVE_OF[curve], FIELDS[curve]
    odd = [bytes(32), p.to_bytes(32, "little"), (p + 1).to_bytes(32, "little"), MARKER, bytes(31) + b"\x80", bytes(32)]
    for x in non_residue_xs(curve):
        odd += [x.to_bytes(32, "little"), (x | 1 << 255).to_bytes(32, "little")]
    encs, it = [], iter(points)
    for i in range(64):
        encs.append(odd[i // 3] if i % 3 == 1 and i // 3 < len(odd) else cv.compress(next(it)))
    want, bad = [], []
    for i, e in enumerate(encs):
        pt, ok = decode_ref(curve, e)
        want.append(cv.affine_to_bytes(pt))
        if not ok:
            bad.append(i)
    return encs, want, bad
