"""field.h and fe_vec.h ON THE DEVICE, at the bounds each function states, against Python integers.

tests/test_mont_reduction.py checks the Montgomery products at their limb and value bounds through the host build, whose
row operations are plain C++.  On gfx950 the products run the v_mad_u64_u32 rows of field_mad_gfx950.h instead, and the lazy
accumulators of fe_vec.h exist only on the device.  reef_amd/csrc/tools/field_check.hip (libreef_fieldcheck.so, release
flags) exposes both on raw 9 x 29-bit limbs or 9 x u64 columns, so an operand can sit exactly at a stated bound; every result
here must be the exact integer with exact limbs and within the value bound the function's comment promises."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mont_grid import KINDS, MASK, PAIRS, RP, check_limbs, mont, operand, value
from oracle.pasta_oracle import CURVES

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reef_amd", "csrc")
SO = os.path.join(ROOT, "reef_amd", "_lib", "libreef_fieldcheck.so")
FIELDS = {"pallas": 0, "vesta": 1}
BIASES = [2, 4, 8, 16, 32]
TOP = 1 << 256


@pytest.fixture(scope="module")
def fc():
    """The device check library, brought up to date by its Makefile target (make checks the sources).  Missing or unloadable is
    a failure, not a skip."""
    subprocess.check_call(["make", "-C", CSRC, "../_lib/libreef_fieldcheck.so"], stdout=subprocess.DEVNULL)
    h = ctypes.CDLL(SO)
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    h.fc_op.argtypes = [i, i, i, vp, vp, vp, vp, vp, sz]
    h.fc_wide.argtypes = [i, i, vp, vp, sz]
    h.fc_wide18.argtypes = [i, i, vp, vp, sz, vp, sz]
    h.fc_wave_sum.argtypes = [vp, vp, sz]
    h.fc_convert.argtypes = [i, i, i, i, i, vp, vp, sz]
    for f in (h.fc_op, h.fc_wide, h.fc_wide18, h.fc_wave_sum, h.fc_convert):
        f.restype = ctypes.c_int
    return h


def limbs(v, n=9):
    """Strict 29-bit limbs of v (the top one holds the rest)."""
    return [(v >> (29 * i)) & MASK for i in range(n - 1)] + [v >> (29 * (n - 1))]


def words(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)] + [0]


def from_words(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w[:8]))


def spread(v, lmax, rng):
    """Limbs of v with limbs 0..7 in [0, lmax] (not strict): each limb borrows a random amount from the one above."""
    l = limbs(v)
    for i in range(8):
        t = min(l[i + 1], (lmax - l[i]) >> 29)
        if t > 0:
            t = int(rng.integers(0, t + 1)) if rng is not None else t
            l[i] += t << 29
            l[i + 1] -= t
    assert value(l) == v and all(0 <= x <= lmax for x in l[:8])
    return l


def op(fc, f, code, k, ops):
    n = len(ops[0])
    arrs = [np.array(x, dtype=np.uint32).reshape(n, 9) for x in ops]
    while len(arrs) < 4:
        arrs.append(np.zeros((n, 9), dtype=np.uint32))
    out = np.zeros((n, 9), dtype=np.uint32)
    assert fc.fc_op(f, code, k, *[a.ctypes.data for a in arrs], out.ctypes.data, n) == 0
    return [[int(x) for x in r] for r in out]


def strict(r):
    return all(x <= MASK for x in r[:8])


# ---------------------------------------------------------------- products: the grid of mont_grid.py, on the device ----------

@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("ab", PAIRS)
def test_mul(fc, name, ab):
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(100 + f)
    xs = [operand(rng, m, ab[0], kd) for kd in KINDS]
    ys = [operand(rng, m, ab[1], kd) for kd in reversed(KINDS)]
    out, wide = op(fc, f, 0, 0, (xs, ys)), op(fc, f, 5, 0, (xs, ys))
    for x, y, r, w in zip(xs, ys, out, wide):
        want = mont(value(x) * value(y), m)
        check_limbs(r, m, 2, want)
        check_limbs(w, m, 2, want)


@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("a", [1.0, 4.0, 11.3])
def test_sqr(fc, name, a):
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(200 + f)
    xs = [operand(rng, m, a, kd) for kd in KINDS]
    for x, r in zip(xs, op(fc, f, 1, 0, (xs,))):
        check_limbs(r, m, 2, mont(value(x) ** 2, m))


@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("bounds", [(1.0, 1.0, 1.0, 1.0), (8.0, 7.9, 8.0, 7.9), (2.0, 2.0, 11.0, 11.0)])
def test_mul2_add(fc, name, bounds):
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(300 + f)
    ops = [[operand(rng, m, bd, kd) for kd in (KINDS if i % 2 == 0 else list(reversed(KINDS)))] for i, bd in enumerate(bounds)]
    for a, b, c, d, r in zip(*ops, op(fc, f, 2, 0, ops)):
        check_limbs(r, m, 2, mont(value(a) * value(b) + value(c) * value(d), m))


@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("k", BIASES)
@pytest.mark.parametrize("sqr", [False, True])
def test_fused_sub(fc, name, k, sqr):
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(400 + 10 * k + f + 2 * sqr)
    ab = (11.3, 11.3) if sqr else (9.02, 5.04)
    cb = k * (1 - 2e-5)
    xs = [operand(rng, m, ab[0], kd) for kd in KINDS]
    ys = [operand(rng, m, ab[1], kd) for kd in reversed(KINDS)]
    cs = [operand(rng, m, cb, kd) for kd in KINDS[1:] + KINDS[:1]]
    for x, y, c, r in zip(xs, ys, cs, op(fc, f, 4 if sqr else 3, k, (xs, ys, cs))):
        t = value(x) ** 2 if sqr else value(x) * value(y)
        check_limbs(r, m, 2 + k, mont(t, m) + k * m - value(c))


# ------------------------------------------------------------------------------------ the rest of field.h the rows use ----

def _normalised(r):
    return r[0] <= MASK and all(x <= MASK + 8 for x in r[1:8])


@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("ab", [(1.0, 1.0), (2.0, 2.0), (11.3, 11.3), (32.0, 31.9), (1.0, 62.9)])
def test_add(fc, name, ab):
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(500 + f)
    xs = [operand(rng, m, ab[0], kd) for kd in KINDS]
    ys = [operand(rng, m, ab[1], kd) for kd in reversed(KINDS)]
    for x, y, r in zip(xs, ys, op(fc, f, 6, 0, (xs, ys))):
        assert _normalised(r), [hex(v) for v in r]
        assert value(r) == value(x) + value(y)


@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("k", BIASES)
def test_sub(fc, name, k):
    """a + K*M - b for b < K*M with limbs up to 2^31 - 5 (the contract) and a normalised."""
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(600 + 10 * k + f)
    bias_top = (k * m) >> 232   # the bias's top limb, less what its widened low limbs took (>= the strict top limb - 4)
    xs, ys = [], []
    for i, kd in enumerate(KINDS):
        xs.append(operand(rng, m, 2.0, kd))
        if i % 3 == 0:      # limbs 0..7 at the contract's edge, the top limb as large as b < K*M and the bias's top limb allow
            low = [(1 << 31) - 5] * 8
            rest = k * m - 1 - value(low + [0])
            top = min(rest >> 232, bias_top - 4)
            y = low + [top - int(rng.integers(0, 4)) * (i % 2)]
        else:
            y = operand(rng, m, k * (1 - 2e-5), kd)
        ys.append(y)
    for x, y, r in zip(xs, ys, op(fc, f, 7, k, (xs, ys))):
        assert _normalised(r), [hex(v) for v in r]
        assert value(r) == value(x) + k * m - value(y)
        assert value(r) < (2 + k) * m


@pytest.mark.parametrize("lmax", [MASK, MASK + 8, (1 << 32) - 9])
def test_norm_strict(fc, lmax):
    rng = np.random.default_rng(700)
    xs = [[lmax] * 8 + [(1 << 30)], [0] * 9] + [[int(rng.integers(0, lmax + 1)) for _ in range(8)] + [int(rng.integers(0, 1 << 31))]
                                               for _ in range(62)]
    for x, r in zip(xs, op(fc, 0, 8, 0, (xs,))):
        assert strict(r) and value(r) == value(x)


def _canon_inputs(m, rng):
    vals = [0, 1, m - 1, m, TOP - 1 if TOP - 1 < 64 * m else 0, 64 * m - 1]
    for k in range(1, 65):
        vals += [k * m - 1, k * m, k * m - (1 << 200)]
    vals += [int(rng.integers(0, 64)) * m + int(rng.integers(0, 1 << 62)) * (m >> 62) for _ in range(32)]
    return vals


@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("rep", ["strict", "normalised", "wide"])
def test_canon(fc, name, rep):
    """Fully reduced from any value below 64 M, from strict limbs, normalised limbs and limbs up to 2^32 - 9; k*M for k <= 64."""
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(800 + f)
    vals = _canon_inputs(m, rng)
    lmax = {"strict": MASK, "normalised": MASK + 8, "wide": (1 << 32) - 9}[rep]
    xs = [limbs(v) if rep == "strict" else spread(v, lmax, rng if i % 2 else None) for i, v in enumerate(vals)]
    for v, r in zip(vals, op(fc, f, 9, 0, (xs,))):
        assert strict(r), [hex(x) for x in r]
        assert value(r) == v % m, (hex(v), hex(value(r)))


@pytest.mark.parametrize("name", list(FIELDS))
def test_inv(fc, name):
    """a^(M-2) in the internal form: r = R'^2 / a mod M, value < 2 M; inv(0) = 0 for 0 and M."""
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(900 + f)
    xs = [[0] * 9, limbs(m), limbs(1), limbs(m - 1), limbs(TOP - 1), operand(rng, m, 63.9, "max"), operand(rng, m, 1.0, "max")]
    xs += [operand(rng, m, b, "rand") for b in (1.0, 2.0, 63.9) for _ in range(3)]
    for x, r in zip(xs, op(fc, f, 10, 0, (xs,))):
        assert strict(r) and value(r) < 2 * m
        a = value(x) % m
        want = 0 if a == 0 else RP * RP * pow(a, m - 2, m) % m
        assert value(r) % m == want


def _words_inputs(m, rng):
    return [0, 1, m - 1, m, TOP - 1, (1 << 254) - 1, 2 * m, 3 * m + 7] + [int(rng.integers(0, 1 << 62)) << 194 | int(rng.integers(0, 1 << 62))
                                                                  for _ in range(8)]


@pytest.mark.parametrize("name", list(FIELDS))
def test_pack_unpack(fc, name):
    f, m = FIELDS[name], CURVES[name].base
    vals = _words_inputs(m, np.random.default_rng(1000 + f))
    for v, r in zip(vals, op(fc, f, 11, 0, ([words(v) for v in vals],))):
        assert strict(r) and value(r) == v
    for v, r in zip(vals, op(fc, f, 12, 0, ([limbs(v) for v in vals],))):
        assert from_words(r) == v and r[8] == 0


@pytest.mark.parametrize("name", list(FIELDS))
def test_abi_and_integer_forms(fc, name):
    """The conversions on their contract's inputs -- canonical words for fe_from_abi / fe_from_integer / fe_abi_to_integer
    (field.h), normalised elements for fe_to_abi / fe_to_integer -- and BEYOND it: the words M, 2 M, 3 M + 7, 2^256 - 1 and
    elements up to 127.9 M.  The beyond-contract cases pin what the arithmetic gives there (the unpacked word is below 4 M and
    the product takes (A/M)(B/M) < 128); no caller relies on them.  Canonical outputs where packed."""
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(1100 + f)
    vals = _words_inputs(m, rng)
    ws = [words(v) for v in vals]
    for v, r in zip(vals, op(fc, f, 13, 0, (ws,))):                       # v = x 2^256 -> x 2^261
        assert strict(r) and value(r) < 2 * m and value(r) % m == v * 32 % m
    for v, r in zip(vals, op(fc, f, 15, 0, (ws,))):                       # x -> x 2^261
        assert strict(r) and value(r) < 2 * m and value(r) % m == v * RP % m
    for v, r in zip(vals, op(fc, f, 17, 0, (ws,))):                       # x 2^256 -> x
        assert from_words(r) == v * pow(2, -256, m) % m and r[8] == 0
    xs = [limbs(0), limbs(m - 1), limbs(m), operand(rng, m, 127.9, "max"), operand(rng, m, 2.0, "max")]
    xs += [operand(rng, m, 127.9, kd) for kd in ("top", "rand", "rand")]
    for x, r in zip(xs, op(fc, f, 14, 0, (xs,))):                         # x 2^261 -> x 2^256, canonical
        assert from_words(r) == value(x) * pow(2, -5, m) % m and r[8] == 0
    for x, r in zip(xs, op(fc, f, 16, 0, (xs,))):                         # x 2^261 -> x, canonical
        assert from_words(r) == value(x) * pow(RP, -1, m) % m and r[8] == 0


# ------------------------------------------------------------------------------------------------------------ fe_vec.h ----

def _wide(fc, f, code, cols):
    n = len(cols)
    a = np.array(cols, dtype=np.uint64).reshape(n, 9)
    out = np.zeros((n, 9), dtype=np.uint32)
    assert fc.fc_wide(f, code, a.ctypes.data, out.ctypes.data, n) == 0
    return [[int(x) for x in r] for r in out]


def colval(c):
    return sum(int(x) << (29 * i) for i, x in enumerate(c))


@pytest.mark.parametrize("name", list(FIELDS))
def test_from_wide(fc, name):
    """Columns of up to 2^34 normalised elements (every limb <= 2^29 + 7): the exact residue, exact limbs, value < 2 M.  Past
    2^290 the carry above 2^261 has a part c1 above 2^29, which only the largest column sums reach."""
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(1200 + f)
    cmax = (1 << 34) * (MASK + 8)
    cols = [[cmax] * 9, [cmax - 1] * 9, [0] * 9, [cmax] * 8 + [0], [0] * 8 + [cmax], [MASK] * 9, limbs(m), limbs(m - 1)]
    cols += [[int(rng.integers(0, cmax + 1, dtype=np.uint64)) for _ in range(9)] for _ in range(40)]
    cols += [[int(rng.integers(0, 1 << 40)) for _ in range(8)] + [int(rng.integers(1 << 58, cmax + 1, dtype=np.uint64))] for _ in range(16)]
    assert any(colval(c) >> 290 for c in cols)
    for c, r in zip(cols, _wide(fc, f, 0, cols)):
        assert strict(r) and value(r) < 2 * m, [hex(x) for x in r]
        assert value(r) % m == colval(c) % m


@pytest.mark.parametrize("name", list(FIELDS))
def test_from_limb_sums(fc, name):
    """Limbs below 2^58, value below 2^30 M (its whole envelope), and what its callers feed: sums of up to 2^28 reduced
    elements (N2) and of products < 2 M with exact limbs (N5, the opening, Hyrax).  Canonical result."""
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(1300 + f)
    lim = (1 << 30) * m - 1
    low = [(1 << 58) - 1] * 8
    cols = [low + [(lim - colval(low + [0])) >> 232], low + [0], [0] * 9, limbs(lim), limbs(m), limbs(m - 1), limbs(m + 1)]
    n28 = (1 << 28) - 1
    cols.append([n28 * MASK] * 8 + [n28 * ((m - 1) >> 232)])                   # 2^28 - 1 elements with canonical limbs, < M
    cols.append([n28 * MASK] * 8 + [n28 * ((2 * m - 1) >> 232)])               # products < 2 M
    for _ in range(48):
        c = [int(rng.integers(0, 1 << 58, dtype=np.uint64)) for _ in range(8)]
        rest = lim - colval(c + [0])
        c.append(int(rng.integers(0, (rest >> 232) + 1, dtype=np.uint64)))
        cols.append(c)
    for c in cols:
        assert colval(c) < (1 << 30) * m and all(x < (1 << 58) for x in c[:8])
    for c, r in zip(cols, _wide(fc, f, 1, cols)):
        assert strict(r), [hex(x) for x in r]
        assert value(r) == colval(c) % m


def _wide18(fc, f, reduce, sets):
    n, mm = len(sets), len(sets[0])
    a = np.array([p[0] for s in sets for p in s], dtype=np.uint32).reshape(n * mm, 9)
    b = np.array([p[1] for s in sets for p in s], dtype=np.uint32).reshape(n * mm, 9)
    out = np.zeros((n, 9), dtype=np.uint32)
    assert fc.fc_wide18(f, reduce, a.ctypes.data, b.ctypes.data, mm, out.ctypes.data, n) == 0
    return [[int(x) for x in r] for r in out]


@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("nprod", [1, 3, 4, 5, 8, 64, 1024])
def test_wide18_mont(fc, name, nprod):
    """N products with sum (A/M)(B/M) < 128 and limbs up to 2^29 + 7, a carry after every fourth: wide18_mont(w, 2) is the
    exact Montgomery reduction of the sum, value < 2 M (the Merkle and MLE form)."""
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(1400 + 7 * nprod + f)
    share = 127.9 / nprod
    sets = []
    for s in range(6):
        ab = [(1.0, share), (share, 1.0), (share ** 0.5, share ** 0.5)][s % 3]
        kinds = ["max"] * nprod if s < 3 else [KINDS[int(rng.integers(0, len(KINDS)))] for _ in range(nprod)]
        sets.append([(operand(rng, m, ab[0], kd), operand(rng, m, ab[1], kd)) for kd in kinds])
    for s, r in zip(sets, _wide18(fc, f, 0, sets)):
        check_limbs(r, m, 2, mont(sum(value(x) * value(y) for x, y in s), m))


@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("nprod", [1, 5, 256, 1024])
def test_wide18_reduce(fc, name, nprod):
    """Up to 1024 products of a 256-bit value (< 4.25 M) and a reduced one, w < 34 * 128 * M^2 at 1024: wide18_reduce returns
    the same residue as the sum's Montgomery reduction times one, exact limbs, value < 2 M."""
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(1500 + nprod + f)
    one = RP % m
    sets = [[(operand(rng, m, 4.2499, "max"), operand(rng, m, 1.0, "max")) for _ in range(nprod)],
            [(limbs(TOP - 1), limbs(m - 1)) for _ in range(nprod)],
            [(operand(rng, m, 4.2499, kd), operand(rng, m, 1.0, kd)) for kd in rng.choice(KINDS, nprod)]]
    for s, r in zip(sets, _wide18(fc, f, 1, sets)):
        w = sum(value(x) * value(y) for x, y in s)
        assert w < 34 * 128 * m * m
        check_limbs(r, m, 2, mont(mont(w, m) * one, m))


def _wave_sum(fc, lanes):
    v = np.array(lanes, dtype=np.uint64)
    assert v.size % 64 == 0
    out = np.zeros(v.size // 64, dtype=np.uint64)
    assert fc.fc_wave_sum(v.ctypes.data, out.ctypes.data, out.size) == 0
    return [int(x) for x in out]


def test_wave_sum63(fc):
    """Every lane below 2^46: all lanes at 2^46 - 1, one hot lane at each of the 64 positions, distinct lanes, random."""
    top = (1 << 46) - 1
    rng = np.random.default_rng(1600)
    waves = [[top] * 64, [0] * 64]
    waves += [[top if j == h else 0 for j in range(64)] for h in range(64)]
    waves += [[top if j == h else (h * 64 + j) for j in range(64)] for h in range(64)]
    waves += [[top - j * 0x10_0001 for j in range(64)], [(1 << (20 + j % 26)) - 1 for j in range(64)], [j << 40 | j for j in range(64)]]
    waves += [[int(x) for x in rng.integers(0, top + 1, 64, dtype=np.uint64)] for _ in range(16)]
    got = _wave_sum(fc, [x for w in waves for x in w])
    assert got == [sum(w) for w in waves]


def _convert(fc, f, direction, a, b, in_place, vals):
    n = len(vals)
    src = np.array([words(v)[:8] for v in vals], dtype=np.uint32)
    out = np.zeros_like(src)
    assert fc.fc_convert(f, direction, a, b, in_place, src.ctypes.data, out.ctypes.data, n) == 0
    return [from_words(r) for r in out]


@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("in_place", [0, 1])
@pytest.mark.parametrize("n", [1000, 256, 5])
def test_import_export(fc, name, in_place, n):
    """k_fe_import / k_fe_export in all four form combinations, in place and out of place, counts not a multiple of 256.  The
    words M, 2 M - 1 and 2^256 - 1 are beyond the contract (canonical inputs, field.h): they pin what the arithmetic gives there."""
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(1700 + n + f)
    edge = [0, 1, m - 1, m, TOP - 1, (1 << 254) - 1, 2 * m - 1]
    vals = (edge + [int(rng.integers(0, 1 << 62)) << 192 | int(rng.integers(0, 1 << 62)) for _ in range(n)])[:n]
    r5 = pow(2, -5, m)
    # import: a canonical integer x -> x R'; pasta Montgomery v -> v 2^5
    assert _convert(fc, f, 0, 0, 0, in_place, vals) == [v * RP % m for v in vals]
    assert _convert(fc, f, 0, 1, 0, in_place, vals) == [v * 32 % m for v in vals]
    # export from the table form: t -> t / R', t -> t 2^-5 (canonical t, then every word as a beyond-contract case)
    tabs = [v % m for v in vals]
    assert _convert(fc, f, 1, 0, 0, in_place, tabs) == [t * pow(RP, -1, m) % m for t in tabs]
    assert _convert(fc, f, 1, 0, 1, in_place, tabs) == [t * r5 % m for t in tabs]
    assert _convert(fc, f, 1, 0, 0, in_place, vals) == [t * pow(RP, -1, m) % m for t in vals]
    # export from an integer source: a copy, or the pasta Montgomery form x 2^256
    assert _convert(fc, f, 1, 1, 0, in_place, vals) == vals
    assert _convert(fc, f, 1, 1, 1, in_place, tabs) == [t * (1 << 256) % m for t in tabs]
