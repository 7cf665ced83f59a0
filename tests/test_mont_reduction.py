"""The Montgomery reduction of field.h (biased columns, five-MAD rounds, serial final carry) against Python integers.

The host build of the same templates (REEF_BOUNDS, reef_amd/csrc/tools/mont_check.cpp, g++) runs on raw 29-bit limbs, so the
operands can sit at the limb and value bounds each function states: limbs 1..7 at 2^29 + 7, limb 0 at 2^29 - 1, the top
limb as large as the value bound allows.  Every result must be the exact integer (T + Q*M) / 2^261 (plus K*M - c for the
fused subtractions), where Q < 2^261 is the one quotient with T + Q*M = 0 mod 2^261 -- the value the digit-by-digit
reduction defines, whatever the carry scheme -- with exact 29-bit limbs and the stated value bound.

What this covers: the carry scheme and the bound bookkeeping (REEF_BOUNDS aborts on a violated precondition).  What it does not:
the host build runs the plain C++ forms of mad_row_*, mad_reduce and sqr_row<I>, not the v_mad_u64_u32 rows of
field_mad_gfx950.h that gfx950 runs, and fe_vec.h's accumulators do not exist on the host.  tests/test_gpu_field_bounds.py
runs the same grid, and those accumulators, on the device through the release-flag build of tools/field_check.hip."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mont_grid import KINDS, PAIRS, check_limbs, mont, operand, value
from oracle.pasta_oracle import CURVES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reef_amd", "csrc")
SO = os.path.join(ROOT, "reef_amd", "_lib", "libreef_montcheck.so")
FIELDS = {"pallas": 0, "vesta": 1}


@pytest.fixture(scope="module")
def lib():
    src = os.path.join(CSRC, "tools", "mont_check.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("field.h", "field_consts.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DREEF_BOUNDS", "-shared", "-fPIC", src, "-o", SO])
    h = ctypes.CDLL(SO)
    vp = ctypes.c_void_p
    h.mc_op.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, vp, vp, ctypes.c_size_t]
    return h


def run(lib, f, op, k, ops, bounds):
    n = len(ops[0])
    arrs = [np.array(x, dtype=np.uint32).reshape(n, 9) for x in ops]
    while len(arrs) < 4:
        arrs.append(np.zeros((n, 9), dtype=np.uint32))
    out = np.zeros((n, 9), dtype=np.uint32)
    b = np.array(list(bounds) + [0.0] * (4 - len(bounds)), dtype=np.float64)
    lib.mc_op(f, op, k, *[a.ctypes.data for a in arrs], b.ctypes.data, out.ctypes.data, n)
    return out


@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("ab", PAIRS)
def test_mul(lib, name, ab):
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(100 + f)
    xs = [operand(rng, m, ab[0], kd) for kd in KINDS]
    ys = [operand(rng, m, ab[1], kd) for kd in reversed(KINDS)]
    out = run(lib, f, 0, 0, (xs, ys), ab)
    wide = run(lib, f, 5, 0, (xs, ys), ab)
    for x, y, r, w in zip(xs, ys, out, wide):
        want = mont(value(x) * value(y), m)
        check_limbs(r, m, 2, want)
        check_limbs(w, m, 2, want)


@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("a", [1.0, 4.0, 11.3])
def test_sqr(lib, name, a):
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(200 + f)
    xs = [operand(rng, m, a, kd) for kd in KINDS]
    out = run(lib, f, 1, 0, (xs,), (a,))
    for x, r in zip(xs, out):
        check_limbs(r, m, 2, mont(value(x) ** 2, m))


@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("bounds", [(1.0, 1.0, 1.0, 1.0), (8.0, 7.9, 8.0, 7.9), (2.0, 2.0, 11.0, 11.0)])
def test_mul2_add(lib, name, bounds):
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(300 + f)
    ops = [[operand(rng, m, bd, kd) for kd in (KINDS if i % 2 == 0 else list(reversed(KINDS)))] for i, bd in enumerate(bounds)]
    out = run(lib, f, 2, 0, ops, bounds)
    for a, b, c, d, r in zip(*ops, out):
        check_limbs(r, m, 2, mont(value(a) * value(b) + value(c) * value(d), m))


# every bias the group law uses (ec.h: fe_mul_sub K = 8 and 4, fe_sqr_sub K = 4) and the others fe_bias offers
@pytest.mark.parametrize("name", list(FIELDS))
@pytest.mark.parametrize("k", [2, 4, 8, 16, 32])
@pytest.mark.parametrize("sqr", [False, True])
def test_fused_sub(lib, name, k, sqr):
    f, m = FIELDS[name], CURVES[name].base
    rng = np.random.default_rng(400 + 10 * k + f + 2 * sqr)
    ab = (11.3, 11.3) if sqr else (9.02, 5.04)
    cb = k * (1 - 2e-5)
    xs = [operand(rng, m, ab[0], kd) for kd in KINDS]
    ys = [operand(rng, m, ab[1], kd) for kd in reversed(KINDS)]
    cs = [operand(rng, m, cb, kd) for kd in KINDS[1:] + KINDS[:1]]
    out = run(lib, f, 4 if sqr else 3, k, (xs, ys, cs), (ab[0], ab[1], cb))
    for x, y, c, r in zip(xs, ys, cs, out):
        t = value(x) ** 2 if sqr else value(x) * value(y)
        check_limbs(r, m, 2 + k, mont(t, m) + k * m - value(c))
