"""The loop-form key-table record (reef_amd/csrc/ec.h: affine_limbs -- what k_limb_tables stores once per key and k_accum0 loads per
entry) on the host, compiled with g++ and REEF_BOUNDS like tests/test_host_math.py.  Runs without a GPU.  A record must hold, limb for
limb, what the loop computes from the packed entry today: fe_from_table of x and of y, fe_neg<F, 2> of y; the identity is zero limbs and
a set flag; and the loop on records must walk through the same accumulators as the loop on packed entries."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle.pasta_oracle import CURVES, SplitMix64, uniform_scalar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reef_amd", "csrc")
SO = os.path.join(ROOT, "reef_amd", "_lib", "libreef_limbcheck.so")
CID = {"pallas": 0, "vesta": 1}
X, TOP, Y, NEG_Y = 0, 8, 12, 20            # word offsets of a record (ec.h)


@pytest.fixture(scope="module")
def host():
    src = os.path.join(CSRC, "tools", "limb_check.cpp")
    deps = [src] + [os.path.join(CSRC, f) for f in ("field.h", "ec.h", "field_consts.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DREEF_BOUNDS", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    vp = ctypes.c_void_p
    lib.limb_record.argtypes = [ctypes.c_int, vp, vp, vp, vp, vp]
    lib.limb_entry.argtypes = [ctypes.c_int, vp, ctypes.c_int, vp, vp]
    lib.limb_to_table.argtypes = [ctypes.c_int, vp, vp]
    lib.limb_chains.argtypes = [ctypes.c_int, vp, vp, ctypes.c_size_t, vp]
    return lib


def words(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def value(limbs):
    """The integer nine 29-bit-radix limbs stand for (limbs may exceed 29 bits: the radix is what counts)."""
    return sum(int(l) << (29 * i) for i, l in enumerate(limbs))


def record(host, f, x, y):
    packed = np.array(words(x) + words(y), dtype=np.uint32)
    rec = np.zeros(32, dtype=np.uint32)
    fx, fy, fn = (np.zeros(9, dtype=np.uint32) for _ in range(3))
    host.limb_record(f, packed.ctypes.data, rec.ctypes.data, fx.ctypes.data, fy.ctypes.data, fn.ctypes.data)
    return rec, fx, fy, fn


def normalised(limbs):
    """field.h: l0 < 2^29 exactly, l1 .. l7 <= 2^29 + 7, the top limb holds the rest."""
    return limbs[0] < (1 << 29) and all(int(l) <= (1 << 29) + 7 for l in limbs[1:8])


def edge_values(m):
    ones = [(1 << (32 * j)) - 1 for j in range(1, 8)] + [(1 << 254) - 1]       # packed words all ones, below M = 2^254 + delta
    return [0, 1, m - 1, 2, m - 2, (1 << 29) - 1, 1 << 29, (1 << 232) - 1, 1 << 232, 1 << 254] + ones


@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_record_holds_what_the_loop_computes(name, host):
    f, m = CID[name], CURVES[name].base
    rng = SplitMix64(2300 + f)
    vals = edge_values(m) + [uniform_scalar(rng, m) for _ in range(300)]
    assert all(v < m for v in vals)
    pairs = [(x, y) for x in edge_values(m) for y in edge_values(m) if (x, y) != (0, 0)]
    pairs += [(vals[i], vals[-1 - i]) for i in range(len(vals))] + [(uniform_scalar(rng, m), uniform_scalar(rng, m)) for _ in range(300)]
    pairs = [p for p in pairs if p != (0, 0)]
    for x, y in pairs:
        rec, fx, fy, fn = record(host, f, x, y)
        rx = list(rec[X:X + 8]) + [rec[TOP]]
        ry = list(rec[Y:Y + 8]) + [rec[TOP + 1]]
        rn = list(rec[NEG_Y:NEG_Y + 8]) + [rec[TOP + 2]]
        assert rx == list(fx) and ry == list(fy), (hex(x), hex(y))                 # fe_from_table, limb for limb
        assert rn == list(fn), (hex(x), hex(y))                                    # fe_neg<F, 2>, limb for limb
        assert rec[TOP + 3] == 0 and not rec[28:].any(), (hex(x), hex(y))          # not the identity; the padding is zero
        assert value(rx) == x and value(ry) == y and value(rn) == 2 * m - y        # x < 1 M, y < 1 M, -y <= 2 M: the bounds of ec.h
        assert normalised(rx) and normalised(ry) and normalised(rn), (hex(x), hex(y))
        assert all(int(l) < (1 << 29) for l in rx + ry)                            # unpacked limbs are exact
        assert int(rn[8]) < (1 << 29)                                              # fe_norm's top limb did not overflow
        for neg in (0, 1):                                                         # what the loop reads back for either sign
            ex, ey = np.zeros(9, dtype=np.uint32), np.zeros(9, dtype=np.uint32)
            assert host.limb_entry(f, rec.ctypes.data, neg, ex.ctypes.data, ey.ctypes.data) == 0
            assert list(ex) == rx and list(ey) == (rn if neg else ry)


@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_identity_record(name, host):
    f = CID[name]
    rec, fx, fy, _ = record(host, f, 0, 0)
    assert not rec[:TOP + 3].any() and not rec[Y:].any()                           # x, y and -y are zero limbs ...
    assert rec[TOP + 3] != 0                                                       # ... and the flag is set
    assert not fx.any() and not fy.any()
    for neg in (0, 1):
        ex, ey = np.zeros(9, dtype=np.uint32), np.zeros(9, dtype=np.uint32)
        assert host.limb_entry(f, rec.ctypes.data, neg, ex.ctypes.data, ey.ctypes.data) == 1
        assert not ex.any() and not ey.any()


@pytest.mark.parametrize("name", ["pallas", "vesta"])
def test_both_loops_walk_through_the_same_accumulators(name, host, cref):
    """Chains with sign flips, a repeated point (the doubling branch), an immediate cancellation, identity entries (also as the
    first entry and with a negative digit): the accumulators agree limb for limb after every entry, no bound is missed (REEF_BOUNDS
    aborts), and the sum is the oracle's."""
    cid, C = CID[name], CURVES[name]
    n = 400
    pts = cref.gen_bases_ap(cid, 23, 5, n)
    neg = (np.arange(n) % 3 == 1).astype(np.uint8)
    pts[0] = 0; neg[0] = 1                         # the identity first, with a negative digit
    pts[5] = pts[4]; neg[5] = neg[4] = 0           # P + P
    pts[6] = pts[4]; neg[6] = 1
    pts[10] = 0; neg[10] = 0
    pts[20] = pts[19]; neg[19] = 0; neg[20] = 1    # cancels the addend before it
    tab = np.zeros((n, 16), dtype=np.uint32)
    for i in range(n):
        host.limb_to_table(cid, pts[i].ctypes.data, tab[i].ctypes.data)
    out = np.zeros(36, dtype=np.uint32)
    assert host.limb_chains(cid, tab.ctypes.data, neg.ctypes.data, n, out.ctypes.data) == 1
    acc = None
    for i in range(n):
        p = C.affine_from_bytes(pts[i].tobytes())
        acc = C.add(acc, C.neg(p) if neg[i] else p)
    # XYZZ in the internal Montgomery radix R' = 2^261: x = X / ZZ, y = Y / ZZZ
    m = C.base
    Xv, Yv, ZZ, ZZZ = (value(out[9 * k:9 * k + 9]) % m for k in range(4))
    x = Xv * pow(ZZ, -1, m) % m
    y = Yv * pow(ZZZ, -1, m) % m
    assert (x, y) == (acc[0], acc[1])
    two = np.stack([tab[7], tab[7]])               # P - P: the identity falls out as ZZ = 0
    assert host.limb_chains(cid, two.ctypes.data, np.array([0, 1], dtype=np.uint8).ctypes.data, 2, out.ctypes.data) == 1
    assert value(out[18:27]) % m == 0
