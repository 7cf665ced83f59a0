"""The grid of tests/ec_grid.py through the HOST build of ec.h (reef_amd/csrc/tools/host_check.cpp, REEF_BOUNDS): every raw-limb entry
point the device harness has, except the four-wave operations, which exist on the device alone.  This proves the generator and
its reference before a GPU is involved -- tests/test_gpu_ec_bounds.py runs the same checks on gfx950 -- with every operand's
tracked bound set from its representation, so that a violated bound comment of ec.h still aborts the process.  It also settles
the two conditions on the inputs: the P + P cases of the mixed addition make U2 - X1 + 8M take every multiple 1..8 of M, and the
direct grid of fe_is_zero is complete."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ec_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reef_amd", "csrc")
SO = os.path.join(ROOT, "reef_amd", "_lib", "libreef_hostcheck.so")
NAMES = ["pallas", "vesta"]


def u32(rows, width):
    return np.array(rows, dtype=np.uint32).reshape(len(rows), width)


class Host:
    def __init__(self, lib):
        self.lib = lib

    @staticmethod
    def bounds(ops, name):
        m = ec_grid.CURVES[name].base
        return np.array([o.bounds(m) for o in ops], dtype=np.float64)

    def pred(self, cid, op, rows, bounds):
        stride = len(rows[0])
        a, b, out = u32(rows, stride), np.array(bounds, dtype=np.float64), np.zeros(len(rows), dtype=np.uint32)
        self.lib.host_ec_raw_pred(cid, op, a.ctypes.data, stride, b.ctypes.data, out.ctypes.data, len(rows))
        return out.tolist()

    def one_wave(self, cid, op, a, b, flags):
        n, name = len(a), NAMES[cid]
        wa, wb, fl, out = u32([o.words for o in a], 36), u32([o.words for o in b], 36), np.array(flags, dtype=np.uint32), np.zeros((len(a), 36), dtype=np.uint32)
        ba, bb = self.bounds(a, name), self.bounds(b, name)
        self.lib.host_ec_raw_one_wave(cid, op, wa.ctypes.data, ba.ctypes.data, wb.ctypes.data, bb.ctypes.data, fl.ctypes.data, out.ctypes.data, n)
        return out

    def entry(self, cid, table, pay, acc, empty):
        n, tab = len(pay), u32(table, 16)
        assert all((p & 0x7FFFFFFF) < len(table) for p in pay)
        wa, ba = u32([o.words for o in acc], 36), self.bounds(acc, NAMES[cid])
        pw, ew = np.array(pay, dtype=np.uint32), np.array(empty, dtype=np.uint32)
        o1, o2, rec = np.zeros((n, 36), dtype=np.uint32), np.zeros((n, 36), dtype=np.uint32), np.zeros((len(table), 32), dtype=np.uint32)
        self.lib.host_ec_raw_entry(cid, tab.ctypes.data, len(table), pw.ctypes.data, wa.ctypes.data, ba.ctypes.data, ew.ctypes.data,
                                   o1.ctypes.data, o2.ctypes.data, rec.ctypes.data, n)
        return o1, o2, rec

    def chain(self, cid, table, pay):
        tab, pw = u32(table, 16), u32(pay, len(pay[0]))
        assert int((pw & 0x7FFFFFFF).max()) < len(table)
        out = np.zeros(pw.shape + (36,), dtype=np.uint32)
        self.lib.host_ec_raw_chain(cid, tab.ctypes.data, pw.ctypes.data, pw.shape[1], out.ctypes.data, pw.shape[0])
        return out

    def convert(self, cid, op, ops):
        w, b, out = u32([o.words for o in ops], 36), self.bounds(ops, NAMES[cid]), np.zeros((len(ops), 36), dtype=np.uint32)
        self.lib.host_ec_raw_convert(cid, op, w.ctypes.data, b.ctypes.data, out.ctypes.data, len(ops))
        return out


@pytest.fixture(scope="module")
def dev():
    src = os.path.join(CSRC, "tools", "host_check.cpp")
    deps = [src, os.path.join(CSRC, "tools", "ec_ops.h")] + [os.path.join(CSRC, f) for f in ("field.h", "ec.h", "field_consts.h", "glv_host.h", "glv_consts.h", "host_combine.h")]
    if not os.path.exists(SO) or os.path.getmtime(SO) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(SO), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-DREEF_BOUNDS", "-shared", "-fPIC", src, "-o", SO])
    lib = ctypes.CDLL(SO)
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    lib.host_ec_raw_pred.argtypes = [i, i, vp, sz, vp, vp, sz]
    lib.host_ec_raw_one_wave.argtypes = [i, i, vp, vp, vp, vp, vp, vp, sz]
    lib.host_ec_raw_entry.argtypes = [i, vp, sz, vp, vp, vp, vp, vp, vp, vp, sz]
    lib.host_ec_raw_chain.argtypes = [i, vp, vp, sz, vp, sz]
    lib.host_ec_raw_convert.argtypes = [i, i, vp, vp, vp, sz]
    return Host(lib)


@pytest.mark.parametrize("name", NAMES)
def test_the_generator_itself(name):
    """Representations are what they claim: the point comes back, the designed coordinates really have limbs above 2^29 - 1, every lift
    occurs, and the constants read from field_consts.h are the ones the reference assumes."""
    g = ec_grid.Grid(name)
    m = g.m
    assert ec_grid.value(g.one) == ec_grid.RP % m == ec_grid.value(ec_grid.consts(name, "ONE")) and ec_grid.value(g.bias2) == 2 * m
    lifts, over = set(), 0
    for i in range(80):
        o = g.rep_own() if i % 5 == 0 else g.rep(g.points[i % 64])
        assert g.point_of(o.words) == o.pt and g.C.is_on_curve(o.pt)
        parts = g.parts(o.words)
        assert all(ec_grid.is_normalised(p) for p in parts)
        assert all(ec_grid.value(p) < b * m for p, b in zip(parts, (8, 4, 2, 2)))
        lifts |= {(c, ec_grid.value(p) // m) for c, p in enumerate(parts)}
        over += sum(x > ec_grid.MASK for p in parts for x in p[1:8])
    assert lifts >= {(0, k) for k in range(8)} | {(1, k) for k in range(4)} | {(2, 0), (2, 1), (3, 0), (3, 1)}
    assert over >= 7 * 2 * 16 + 7 * 12                        # all of limbs 1..7 of every designed X and ZZ
    for f in range(g.IDENTITY_FORMS):
        assert g.point_of(g.identity(f).words) is None


@pytest.mark.parametrize("name", NAMES)
def test_zero_test_grid_is_complete(name):
    assert ec_grid.zero_grid_is_complete(name)


@pytest.mark.parametrize("name", NAMES)
def test_predicates(dev, name):
    ec_grid.check_predicates(dev, name)


@pytest.mark.parametrize("name", NAMES)
def test_doubling_and_the_small_operations(dev, name):
    ec_grid.check_doubling(dev, name)


@pytest.mark.parametrize("name", NAMES)
def test_additions_and_the_multiples_their_doubling_test_meets(dev, name):
    assert ec_grid.check_additions(dev, name) >= set(range(1, 9))


@pytest.mark.parametrize("name", NAMES)
def test_loop_form_entries(dev, name):
    assert ec_grid.check_entries(dev, name) >= set(range(1, 9))


@pytest.mark.parametrize("name", NAMES)
def test_chains(dev, name):
    ec_grid.check_chains(dev, name)


@pytest.mark.parametrize("name", NAMES)
def test_conversions(dev, name):
    ec_grid.check_conversions(dev, name)


@pytest.mark.parametrize("name", NAMES)
def test_lane_layouts_are_the_ones_wanted(name):
    """The layouts the device test runs: whole waves of one kind, single lanes, the mix, and ragged ends whose last lane is a P + P lane."""
    kinds = [k for k in ec_grid.KINDS_ADD if k != "generic"]
    lay = dict(ec_grid.layouts(kinds))
    for k in kinds:
        assert lay["all " + k] == [k] * 64
        assert [x != "generic" for x in lay["one %s at 17" % k]] == [i == 17 for i in range(64)]
    assert {"double", "cancel", "a_inf", "generic"} == set(lay["side by side"])
    one = lay["one double, one identity operand"]
    assert len(one) == 64 and sorted(set(one)) == ["a_inf", "double", "generic"] and one.count("double") == one.count("a_inf") == 1
    for tail in (37, 1):
        l = lay["ragged %d" % tail]
        assert len(l) % 64 and l[-1] == "double" and set(l[:256]) == {"generic"}
    assert len(lay["n = 150"]) == 150 and set(lay["n = 150"]) == set(kinds) | {"generic"} and len(lay["n = 1, double"]) == 1
