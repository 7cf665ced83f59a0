"""ec.h and ec_coop.h ON THE DEVICE, at the bounds and in the exceptional cases the group law states, against Python integers.

tests/test_host_math.py and tests/test_ec_grid_host.py check the formulas and their value bounds through the host build, whose
products are plain C++.  On gfx950 the products run the v_mad_u64_u32 rows of field_mad_gfx950.h, the wave-wide tests
(REEF_ANY, __any) skip selects or a whole shared doubling per wave, and the four-wave forms exist on the device alone.
reef_amd/csrc/tools/ec_check.hip (libreef_eccheck.so, release flags) exposes all of it on raw limbs, so that an operand can be
any representation the loose bounds allow -- X < 8, Y < 4, ZZ, ZZZ < 2, limbs up to 2^29 + 7, the identity as any ZZ = 0 mod M
-- and tests/ec_grid.py supplies the operands, the lane layouts and the check of every raw result: the point, ZZ^3 = ZZZ^2,
exact limbs where promised, and the value bound ec.h states for the routine."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import ec_grid

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reef_amd", "csrc")
SO = os.path.join(ROOT, "reef_amd", "_lib", "libreef_eccheck.so")
NAMES = ["pallas", "vesta"]
EXCEPTIONAL = [k for k in ec_grid.KINDS_ADD if k != "generic"]


def u32(rows, width):
    return np.ascontiguousarray(np.array(rows, dtype=np.uint32).reshape(len(rows), width))


class Device:
    """The five calls ec_grid's checks make, and the four-wave one."""

    def __init__(self, lib):
        self.lib = lib

    def pred(self, cid, op, rows, bounds):
        stride = len(rows[0])
        a, out = u32(rows, stride), np.zeros(len(rows), dtype=np.uint32)
        assert self.lib.ec_check_pred(cid, op, a.ctypes.data, stride, out.ctypes.data, len(rows)) == 0
        return out.tolist()

    def one_wave(self, cid, op, a, b, flags):
        wa, wb, fl = u32([o.words for o in a], 36), u32([o.words for o in b], 36), np.array(flags, dtype=np.uint32)
        out = np.zeros((len(a), 36), dtype=np.uint32)
        assert self.lib.ec_check_one_wave(cid, op, wa.ctypes.data, wb.ctypes.data, fl.ctypes.data, out.ctypes.data, len(a)) == 0
        return out

    def entry(self, cid, table, pay, acc, empty):
        n, tab, wa = len(pay), u32(table, 16), u32([o.words for o in acc], 36)
        pw, ew = np.array(pay, dtype=np.uint32), np.array(empty, dtype=np.uint32)
        o1, o2, rec = np.zeros((n, 36), dtype=np.uint32), np.zeros((n, 36), dtype=np.uint32), np.zeros((len(table), 32), dtype=np.uint32)
        assert self.lib.ec_check_entry(cid, tab.ctypes.data, len(table), pw.ctypes.data, wa.ctypes.data, ew.ctypes.data,
                                       o1.ctypes.data, o2.ctypes.data, rec.ctypes.data, n) == 0
        return o1, o2, rec

    def chain(self, cid, table, pay):
        tab, pw = u32(table, 16), u32(pay, len(pay[0]))
        out = np.zeros(pw.shape + (36,), dtype=np.uint32)
        assert self.lib.ec_check_chain(cid, tab.ctypes.data, len(table), pw.ctypes.data, pw.shape[1], out.ctypes.data, pw.shape[0]) == 0
        return out

    def convert(self, cid, op, ops):
        w, out = u32([o.words for o in ops], 36), np.zeros((len(ops), 36), dtype=np.uint32)
        assert self.lib.ec_check_convert(cid, op, w.ctypes.data, out.ctypes.data, len(ops)) == 0
        return out

    def coop(self, cid, op, a, b):
        wa, wb, out = u32([o.words for o in a], 36), u32([o.words for o in b], 36), np.zeros((len(a), 36), dtype=np.uint32)
        assert self.lib.ec_check_coop(cid, op, wa.ctypes.data, wb.ctypes.data, out.ctypes.data, len(a)) == 0
        return out


@pytest.fixture(scope="module")
def dev():
    """The device check library, brought up to date by its Makefile target (make checks the sources).  Missing or unloadable is
    a failure, not a skip."""
    subprocess.check_call(["make", "-C", CSRC, "../_lib/libreef_eccheck.so"], stdout=subprocess.DEVNULL)
    h = ctypes.CDLL(SO)
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    h.ec_check_pred.argtypes = [i, i, vp, sz, vp, sz]
    h.ec_check_one_wave.argtypes = [i, i, vp, vp, vp, vp, sz]
    h.ec_check_entry.argtypes = [i, vp, sz, vp, vp, vp, vp, vp, vp, sz]
    h.ec_check_chain.argtypes = [i, vp, sz, vp, sz, vp, sz]
    h.ec_check_coop.argtypes = [i, i, vp, vp, vp, sz]
    h.ec_check_convert.argtypes = [i, i, vp, vp, sz]
    for f in (h.ec_check_pred, h.ec_check_one_wave, h.ec_check_entry, h.ec_check_chain, h.ec_check_coop, h.ec_check_convert):
        f.restype = ctypes.c_int
    return Device(h)


@pytest.mark.parametrize("name", NAMES)
def test_predicates(dev, name):
    """fe_is_zero at every multiple j < 64 of M, beside every near miss that keeps the low limb, in strict and in spread limbs;
    fe_is_literal_zero, xyzz_is_inf on every identity form, affine_is_inf."""
    ec_grid.check_predicates(dev, name)


@pytest.mark.parametrize("name", NAMES)
def test_doubling(dev, name):
    """xyzz_dbl and xyzz_dbl_affine over the representation grid (an identity of any form stays the identity), the negations and
    xyzz_from_affine."""
    ec_grid.check_doubling(dev, name)


@pytest.mark.parametrize("name", NAMES)
def test_additions(dev, name):
    """xyzz_add and xyzz_madd_flags over generic, Q = P in another representation, Q = -P, either operand or both the identity (and
    a_known_empty, p_inf) times the representation grid.  The P + P cases of the mixed addition meet every multiple 1..8 of M in
    fe_is_zero (asserted on the host by tests/test_ec_grid_host.py, and here again on what ran)."""
    assert ec_grid.check_additions(dev, name) >= set(range(1, 9))


@pytest.mark.parametrize("name", NAMES)
def test_loop_form_against_packed_form(dev, name):
    """One entry as k_accum0 composes it from either table form: the same 36 words from both, for both signs and the identity
    record, and the 32-word records word for word."""
    assert ec_grid.check_entries(dev, name) >= set(range(1, 9))


@pytest.mark.parametrize("name", NAMES)
def test_madd_lane_layouts(dev, name):
    """The wave-wide selects of xyzz_madd_flags (REEF_ANY(a_inf), REEF_ANY(p_inf)) and its divergent doubling branch, with whole waves,
    single lanes and ragged ends of each exceptional kind."""
    g, pool = ec_grid.pools(name, "madd")
    for label, layout in ec_grid.layouts(EXCEPTIONAL + ["a_known_empty"]):
        ec_grid.run_cases(dev, g, ec_grid.OP_MADD_FLAGS, ec_grid.lanes_of(pool, layout), label)


@pytest.mark.parametrize("name", NAMES)
def test_four_wave_addition_in_every_lane_layout(dev, name):
    """xyzz_add_coop: every result within the bounds of xyzz_add / xyzz_dbl and the same point as the one-wave addition gives, in
    every layout -- a workgroup in which every lane doubles (the shared doubling with all lanes selected), exactly one lane, the
    mix, the ragged last workgroup whose idle lanes repeat a P + P lane, n = 150 and n = 1."""
    g, pool = ec_grid.pools(name, "add")
    for label, layout in ec_grid.layouts(EXCEPTIONAL):
        cases = ec_grid.lanes_of(pool, layout)
        a, b = [c.a for c in cases], [c.b for c in cases]
        four = dev.coop(g.cid, 0, a, b)
        one = dev.one_wave(g.cid, ec_grid.OP_ADD, a, b, [0] * len(cases))
        for i, (c, w4, w1) in enumerate(zip(cases, four, one)):
            g.check(c, w4, (label, i))
            assert g.point_of(w4) == g.point_of(w1), (label, i, c.kind)


@pytest.mark.parametrize("name", NAMES)
def test_four_wave_doubling(dev, name):
    """xyzz_dbl_coop over the representation grid, every identity form among them; ragged sizes, n = 1."""
    g = ec_grid.Grid(name)
    ops = ec_grid.doubling_operands(g, 150)
    for n in (150, 64, 1):
        four = dev.coop(g.cid, 1, ops[:n], ops[:n])
        one = dev.one_wave(g.cid, ec_grid.OP_DBL, ops[:n], ops[:n], [0] * n)
        for i, (o, w4, w1) in enumerate(zip(ops, four, one)):
            g.check_point(w4, g.C.add(o.pt, o.pt), *ec_grid.DBL, what=(n, i))
            assert g.point_of(w4) == g.point_of(w1), (n, i)


@pytest.mark.parametrize("name", NAMES)
def test_chains(dev, name):
    """The device twin of test_accumulate_chain_bounds: 300-step chains in the loop's form with sign flips, P + P at Z = 1 and right
    after a cancellation, identity entries, immediate cancellations and all-cancelling chains; every intermediate accumulator is
    the running sum and within the result bounds."""
    ec_grid.check_chains(dev, name)


@pytest.mark.parametrize("name", NAMES)
def test_conversions(dev, name):
    """Identity forms come out as (0, 0, 0), (0, 0) and 32 zero bytes; xyzz_from_abi_jacobian o xyzz_to_abi_jacobian is the same point;
    xyzz_to_affine through fe_inv; the parity bit of affine_compress for y and M - y."""
    ec_grid.check_conversions(dev, name)
