"""Inputs shared by tests/test_keygen_inputs_host.py and tests/test_gpu_keygen_edges.py: the domain-separation strings that put the
BLAKE2b messages of row N1 on their block edges, the crafted parameter sets that reach the two branches of sswu_iso a hashed u
never takes, and the indices around the seams of the engine's pieces.  Everything is deterministic and built on the CPU from
oracle/keygen_oracle.py; the host file proves that each input hits what it claims.

Three numbers here are the CODE's own constants, restated; tests/test_keygen_inputs_host.py reads them back out of the sources,
so a change there fails a host test instead of silently moving these inputs off the edges:
    PIECE = 32768       reef_amd/csrc/keygen_engine.inc: `constexpr size_t PIECE`, generators per piece (one launch, streams alternate)
    B0_FIXED = 164      reef_amd/csrc/keygen_kernels.inc, k_hash_to_curve: 128 (Z_pad) + 32 (chunk) + 3 (I2OSP(128, 2), 0) + 1 (the length
                        byte of DST'); the message of b0 is B0_FIXED + dl bytes
    B12_FIXED = 66      same kernel: 64 (b0, or b0 ^ b1) + 1 (round) + 1 (the length byte); the messages of b1 and b2 are B12_FIXED + dl bytes
BLOCK = 128 is BLAKE2b's (RFC 7693), BUF = 128 + 32 + 3 + 256 the kernel's message buffer."""
import functools
import hashlib
from typing import List, Tuple

from oracle import keygen_oracle as K

PIECE = 32768
B0_FIXED = 164
B12_FIXED = 66
BLOCK = 128
BUF = 128 + 32 + 3 + 256

# b0 is exactly 2 and 3 blocks at dl = 92 and 220, b1 and b2 exactly 1 and 2 blocks at dl = 62 and 190, each with both neighbours;
# 0, 1 and the ABI's largest (255 fills BUF), with its neighbour
EXACT_B0 = (92, 220)
EXACT_B12 = (62, 190)
DST_LENGTHS = (0, 1, 61, 62, 63, 91, 92, 93, 189, 190, 191, 219, 220, 221, 254, 255)
BOTH_ORDERS = EXACT_B12[:1] + EXACT_B0[:1] + EXACT_B12[1:] + EXACT_B0[1:] + (0, 255)    # the lengths also run little-endian

REGULAR_LABEL, REGULAR_N = b"reef test label", 67      # the "regular" input of tests/test_gpu_keygen.py
TV2_TARGETS = ((0, 0), (0, 1), (1, 0), (1, 1))          # (generator, lane) of the crafted-z cases, n = 2
ISO_TARGETS = ((2, 0, 0), (2, 1, 1), (70, 37, 0), (70, 37, 1))   # (n, generator, lane): generator 37 sits in the second workgroup


standin = functools.lru_cache(maxsize=None)(K.standin_params)     # (curve, root_index, little_endian) -> a shared set: copy (with_params), never change


def dst_of(dl: int) -> bytes:
    """A fixed pseudo-random string of dl bytes; from 3 bytes on it holds 0x80 first, a NUL second and 0xff last."""
    s = bytearray(hashlib.shake_256(b"reef keygen dst %d" % dl).digest(dl))
    if dl >= 3:
        s[0], s[1], s[-1] = 0x80, 0x00, 0xFF
    return bytes(s)


def with_params(k: K.KeygenParams, **changed) -> K.KeygenParams:
    f = dict(p=k.p, a=k.a, b=k.b, z=k.z, iso=list(k.iso), dst=k.dst, little_endian=k.little_endian)
    f.update(changed)
    return K.KeygenParams(**f)


def field_elements(label: bytes, n: int, k: K.KeygenParams) -> List[List[int]]:
    """[u0, u1] of every generator: what the two lanes of a generator map"""
    return [K.hash_to_field(c, k.dst, k.p, 2, 64, k.little_endian) for c in K.shake256_chunks(label, n)]


def tv2_of(u: int, k: K.KeygenParams) -> int:
    tv1 = k.z * u * u % k.p
    return (tv1 * tv1 + tv1) % k.p


@functools.lru_cache(maxsize=None)
def tv2_zero_case(curve: str, little_endian: bool, gi: int, which: int) -> Tuple[bytes, K.KeygenParams]:
    """(label, params) for n = 2 with z = -1/u^2 for u = lane `which` of generator gi, so that tv1 = -1 and tv2 = 0 there.  That z is a
    square (-1 is one in the Pasta fields), so the other three maps need a square g(x1): the first label b"tv2-zero-%d" whose
    derivation the oracle completes."""
    base = standin(curve, 0, little_endian)
    for t in range(1000):
        label = b"tv2-zero-%d" % t
        u = field_elements(label, 2, base)[gi][which]
        if u == 0:
            continue
        k = with_params(base, z=-pow(u * u, -1, base.p))
        try:
            K.from_label(label, 2, k)
        except AssertionError:
            continue
        return label, k
    raise AssertionError("no label found")


@functools.lru_cache(maxsize=None)
def iso_kernel_case(curve: str, little_endian: bool, n: int, gi: int, which: int) -> Tuple[bytes, K.KeygenParams]:
    """(label, params) with b = x0 (-a tv2)/(tv2 + 1) for the target u, so that x1 = b (tv2 + 1)/(-a tv2) is x0, the abscissa of the
    isogeny's kernel (x0^3 = 540, root 0 of the stand-in set): where g(x1) is a square the map's image is the identity.  Z stays the
    stand-in non-square, so every other map has a square g(x1) or g(x2).  The first label b"iso-kernel-%d" that works."""
    base = standin(curve, 0, little_endian)
    p = base.p
    x0 = K.cube_roots(540, p)[0]
    for t in range(1000):
        label = b"iso-kernel-%d" % t
        tv2 = tv2_of(field_elements(label, n, base)[gi][which], base)
        if tv2 == 0 or tv2 == p - 1:
            continue
        k = with_params(base, b=x0 * (-base.a * tv2) % p * pow(tv2 + 1, -1, p))
        try:
            if images(label, n, k)[gi][which] is None:
                return label, k
        except AssertionError:
            pass
    raise AssertionError("no label found")


def images(label: bytes, n: int, k: K.KeygenParams):
    """[Q0, Q1] of every generator: the two isogeny images the kernel adds"""
    return [[K.iso_map(K.sswu(u, k), k) for u in us] for us in field_elements(label, n, k)]


def textbook_sswu(u: int, k: K.KeygenParams) -> Tuple[int, int]:
    """RFC 9380 6.6.2 as written: both candidates x1, x2, the one whose g is a square, the sign of u"""
    p, A, B, Z = k.p, k.a, k.b, k.z
    g = lambda x: (x * x * x + A * x + B) % p                                   # noqa: E731
    d = (Z * Z * pow(u, 4, p) + Z * u * u) % p
    x1 = B * pow(Z * A, -1, p) % p if d == 0 else (-B) * pow(A, -1, p) * (1 + pow(d, -1, p)) % p
    x2 = Z * u * u * x1 % p
    x, y = x1, K.sqrt_mod(g(x1), p)
    if y is None:
        x, y = x2, K.sqrt_mod(g(x2), p)
        assert y is not None
    return x, (-y) % p if K.sgn0(u) != K.sgn0(y) else y


def sswu_branches(u: int, k: K.KeygenParams) -> Tuple[bool, bool]:
    """(the first square root succeeds, the sign is flipped) along the straight-line form the oracle and the kernel share.  The flip
    is stated for the root Tonelli-Shanks returns from r = x^((T+1)/2) with the 2^32-th root of unity 5^T: K.sqrt_mod and the kernel's
    fe_sqrt (FC::TS_ROOT) both run exactly that."""
    p = k.p
    tv1 = k.z * u * u % p
    tv2 = (tv1 * tv1 + tv1) % p
    x1 = k.b * (tv2 + 1) * pow(k.a * (k.z if tv2 == 0 else -tv2), -1, p) % p
    ratio = (x1 * x1 * x1 + k.a * x1 + k.b) % p
    y = K.sqrt_mod(ratio, p)
    square = y is not None
    if not square:
        y = tv1 * u * K.sqrt_mod(k.z * ratio, p) % p
    return square, K.sgn0(u) != K.sgn0(y)


def seam_indices(n: int) -> List[int]:
    """the indices within 8 of every multiple of PIECE below n, the first 8 and the last 8"""
    idx = set(range(min(8, n))) | set(range(max(0, n - 8), n))
    for m in range(PIECE, n, PIECE):
        idx |= set(range(m - 8, min(n, m + 9)))
    return sorted(idx)
