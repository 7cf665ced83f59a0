"""What the inputs of tests/test_gpu_keygen_edges.py are (tests/keygen_inputs.py), stated on the host: the domain-separation lengths
end the BLAKE2b messages on block boundaries, the crafted parameter sets reach tv2 = 0 and the isogeny's kernel in exactly the map
they name, the regular input takes both outcomes of the square root and of the sign on both lanes, and the oracle's straight-line
SSWU is the two-candidate map of RFC 9380 6.6.2.  A pass of the GPU file means something only where these hold."""
import os
import random
import re

import pytest

import keygen_inputs as I
from oracle import keygen_oracle as K

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "reef_amd", "csrc")
CURVES = ("pallas", "vesta")


def test_the_restated_constants_are_the_sources():
    engine = open(os.path.join(CSRC, "keygen_engine.inc")).read()
    kernels = open(os.path.join(CSRC, "keygen_kernels.inc")).read()
    assert [int(v) for v in re.findall(r"constexpr size_t PIECE = (\d+);", engine)] == [I.PIECE]
    assert "const bool two = n > PIECE;" in engine and "lanes[piece & 1]" in engine
    assert "unsigned char buf[128 + 32 + 3 + 256], b0[64], uniform[128];" in kernels and I.BUF == 128 + 32 + 3 + 256
    assert "while (len - off > 128)" in kernels and I.BLOCK == 128
    # the two messages as k_hash_to_curve lays them out: every `buf[len++]` outside the DST loop is one fixed byte
    body = kernels[kernels.index("const u32 dl = kd.dst_len;"):kernels.index("const fe u = fe_from_64_bytes")]
    first, rounds = body.split("for (int round = 1;")
    fixed = lambda text: sum(int(n) for n in re.findall(r"for \(int k = 0; k < (\d+); \+\+k\) buf\[len\+\+\]", text)) + \
        len(re.findall(r"(?<!\) )buf\[len\+\+\] = ", text))                                 # noqa: E731
    assert fixed(first) == I.B0_FIXED == 128 + 32 + 3 + 1 and fixed(rounds) == I.B12_FIXED == 64 + 1 + 1
    assert first.count("for (u32 k = 0; k < dl; ++k) buf[len++] = kd.dst[k];") == 1 == rounds.count("for (u32 k = 0; k < dl; ++k) buf[len++] = kd.dst[k];")


def test_dst_lengths_sit_on_the_block_edges():
    assert I.DST_LENGTHS == (0, 1, 61, 62, 63, 91, 92, 93, 189, 190, 191, 219, 220, 221, 254, 255)
    for fixed, exact, blocks in ((I.B0_FIXED, I.EXACT_B0, (2, 3)), (I.B12_FIXED, I.EXACT_B12, (1, 2))):
        for dl, nb in zip(exact, blocks):
            assert fixed + dl == nb * I.BLOCK
            assert {dl - 1, dl, dl + 1} <= set(I.DST_LENGTHS)
            assert (fixed + dl - 1) % I.BLOCK == I.BLOCK - 1 and (fixed + dl + 1) % I.BLOCK == 1
    assert I.B0_FIXED + 255 == 419 == I.BUF and max(I.DST_LENGTHS) == 255
    assert set(I.BOTH_ORDERS) == set(I.EXACT_B0) | set(I.EXACT_B12) | {0, 255}
    # the oracle's own messages have these lengths: expand_message_xmd hashes Z_pad || msg || l_i_b || 0 || DST' and b || i || DST'
    for dl in I.DST_LENGTHS:
        dst = I.dst_of(dl)
        assert len(bytes(128) + bytes(32) + (128).to_bytes(2, "big") + b"\x00" + dst + bytes([dl])) == I.B0_FIXED + dl
        assert len(bytes(64) + b"\x01" + dst + bytes([dl])) == I.B12_FIXED + dl


def test_dst_strings():
    for dl in I.DST_LENGTHS + (256,):
        s = I.dst_of(dl)
        assert len(s) == dl and s == I.dst_of(dl)
        if dl >= 3:
            assert (s[0], s[1], s[-1]) == (0x80, 0x00, 0xFF)
    assert len({I.dst_of(dl) for dl in I.DST_LENGTHS}) == len(I.DST_LENGTHS)
    assert I.dst_of(255)[:62] != I.dst_of(62)                              # not prefixes of one another


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("le", (False, True))
def test_crafted_z_reaches_tv2_zero_in_the_target_map_only(curve, le):
    for gi, which in I.TV2_TARGETS:
        label, k = I.tv2_zero_case(curve, le, gi, which)
        base = K.standin_params(curve, 0, le)
        assert (k.a, k.b, k.iso, k.dst, k.little_endian) == (base.a, base.b, base.iso, base.dst, le) and k.z != base.z
        us = I.field_elements(label, 2, k)
        assert [[I.tv2_of(u, k) == 0 for u in pair] for pair in us] == [[(g, w) == (gi, which) for w in (0, 1)] for g in (0, 1)]
        assert k.z * us[gi][which] ** 2 % k.p == k.p - 1                   # tv1 = -1, not u = 0
        pts = K.from_label(label, 2, k)
        assert None not in pts and all(None not in pair for pair in I.images(label, 2, k))
        assert all((y * y - x * x * x - 5) % k.p == 0 for x, y in pts)
        assert all(K.sswu(u, k) == I.textbook_sswu(u, k) for pair in us for u in pair)


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("le", (False, True))
def test_crafted_b_reaches_the_kernel_in_the_target_map_only(curve, le):
    x0 = K.cube_roots(540, K.standin_params(curve).p)[0]
    for n, gi, which in I.ISO_TARGETS:
        label, k = I.iso_kernel_case(curve, le, n, gi, which)
        base = K.standin_params(curve, 0, le)
        assert (k.a, k.z, k.iso, k.dst) == (base.a, base.z, base.iso, base.dst) and k.b != base.b
        assert (k.iso[4], k.iso[5]) == (-2 * x0 % k.p, x0 * x0 % k.p)      # x_den = (x - x0)^2
        im = I.images(label, n, k)
        assert [(g, w) for g in range(n) for w in (0, 1) if im[g][w] is None] == [(gi, which)]
        assert K.sswu(I.field_elements(label, n, k)[gi][which], k)[0] == x0
        pts = K.from_label(label, n, k)
        assert pts[gi] == im[gi][1 - which] and None not in pts
    assert 2 * 37 >= 64                                                    # generator 37: lanes 74 and 75, the second workgroup of one wave


@pytest.mark.parametrize("curve", CURVES)
def test_the_regular_input_takes_every_branch_on_both_lanes(curve):
    k = K.standin_params(curve)
    assert next(g for g in range(2, 9) if pow(g, (k.p - 1) // 2, k.p) == k.p - 1) == 5      # K.sqrt_mod's root of unity is the kernel's 5^T
    us = I.field_elements(I.REGULAR_LABEL, I.REGULAR_N, k)
    for which in (0, 1):
        seen = {I.sswu_branches(pair[which], k) for pair in us}
        assert seen == {(s, f) for s in (False, True) for f in (False, True)}
    assert all(I.tv2_of(u, k) != 0 for pair in us for u in pair) and None not in [q for pair in I.images(I.REGULAR_LABEL, I.REGULAR_N, k) for q in pair]
    squares = sum(I.sswu_branches(u, k)[0] for pair in us for u in pair)
    assert 40 <= squares <= 94                                             # 134 maps: both outcomes are common, neither a fluke


@pytest.mark.parametrize("curve", CURVES)
def test_oracle_sswu_is_the_two_candidate_map(curve):
    k = K.standin_params(curve)
    rng = random.Random(9380)
    us = [rng.randrange(k.p) for _ in range(50)] + [0, 1, k.p - 1]
    crafted = [I.tv2_zero_case(curve, False, gi, which) for gi, which in ((0, 0), (1, 1))]
    us += [I.field_elements(label, 2, kz)[gi][which] for (label, kz), (gi, which) in zip(crafted, ((0, 0), (1, 1)))]
    assert I.tv2_of(0, k) == 0                                             # u = 0: the nominal z's only way into the exceptional case
    for u in us:
        x, y = K.sswu(u, k)
        assert (x, y) == I.textbook_sswu(u, k)
        assert (y * y - x * x * x - k.a * x - k.b) % k.p == 0 and K.sgn0(y) == K.sgn0(u)


def test_seam_indices():
    assert I.seam_indices(3) == [0, 1, 2] and I.seam_indices(67) == list(range(8)) + list(range(59, 67))
    assert I.seam_indices(I.PIECE) == list(range(8)) + list(range(I.PIECE - 8, I.PIECE))
    s = I.seam_indices(I.PIECE + 1)
    assert s == list(range(8)) + list(range(I.PIECE - 8, I.PIECE + 1)) and I.PIECE - 1 in s and I.PIECE in s
    s = I.seam_indices(2 * I.PIECE + 1)
    assert {I.PIECE - 8, I.PIECE - 1, I.PIECE, I.PIECE + 8, 2 * I.PIECE - 1, 2 * I.PIECE} <= set(s) and len(s) == 8 + 17 + 9
    assert len(I.seam_indices(1 << 17)) == 8 + 3 * 17 + 8 and max(I.seam_indices(1 << 17)) == (1 << 17) - 1
