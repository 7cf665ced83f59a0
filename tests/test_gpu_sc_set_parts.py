"""reef_sc_set_table_parts: the sum-check table (row N2) set from what the caller knows it to be -- field elements, one repeated
value, document symbols of 1, 2 or 4 bytes -- through ONE kernel that writes the resident table, its 4-byte copy and the row classes.
The call must leave the ctx as reef_sc_set_table leaves it for the same values written out as integers, so the checks are the
Python oracle (oracle/sumcheck_oracle.py) where the row structure is forced on at small sizes, and the unchanged old call itself
at the size where the shipped gate opens.  Bit-exact: every value is a canonical integer mod q."""
import ctypes

import numpy as np
import pytest

from oracle.pasta_oracle import SplitMix64, uniform_scalar
from oracle.sumcheck_oracle import Q, gen_eq_table, linear_mle_coeffs, linear_mle_fold

pytestmark = pytest.mark.gpu

_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.uint32}


def _written_out(parts, n):
    """The table the parts describe, as integers (what reef_sc_set_table would be given), zero up to n."""
    t = []
    for part in parts:
        if part[0] == "fe":
            t += [int(v) for v in part[1]]
        elif part[0] == "fill":
            t += [int(part[1])] * part[2]
        else:
            t += [int(v) for v in part[1]]
    assert len(t) <= n
    return t + [0] * (n - len(t))


def _hybrid_parts(ell, rng):
    """The shape of Reef's hybrid table as parts: a public table of cols + 3 field elements (so the fill starts mid-row), one value
    up to the half, then symbols of 1, 2 and 4 bytes that stop short of the end (37 entries short; where the symbol half itself has
    no more than 37 entries, at ell = 4 and 6, 3 short)."""
    n, cols = 1 << ell, 1 << (ell // 2)
    half = n // 2
    n_fe = cols + 3
    cut = 37 if half > 37 else 3
    n_sym = half - cut
    a = (n_sym // 3) & ~1                                        # even: the 2-byte run starts on a dword of the staged symbols
    parts = [("fe", [uniform_scalar(rng, Q) for _ in range(n_fe)]), ("fill", uniform_scalar(rng, Q), half - n_fe),
             ("symbols", np.array([rng.next() % 256 for _ in range(a)], dtype=np.uint8)),
             ("symbols", np.array([rng.next() % 65536 for _ in range(a)], dtype=np.uint16)),
             ("symbols", np.array([rng.next() % (1 << 30) for _ in range(n_sym - 2 * a)], dtype=np.uint32))]
    return parts, _written_out(parts, n)


def _eq_inputs(ell, nq, rng):
    n = 1 << ell
    qs = [rng.next() % n for _ in range(nq)]
    qs[0], qs[-1] = 0, n - 1
    rs = [uniform_scalar(rng, Q) for _ in range(nq + 1)]
    last_q = [uniform_scalar(rng, Q) for _ in range(ell)]
    return rs, qs, last_q


def _check_two_steps(sc, t, ell, rs, qs, last_q, rng, tag):
    """Two folding steps with reset_table between them, the first through fold_and_next_coeffs, the second through fold +
    round_coeffs: every round's coefficients, the folded table after folds 1 and 2, the final values."""
    e = gen_eq_table(rs, qs, last_q, Q)
    for step, fused in ((0, True), (1, False)):
        tt, ee = list(t), list(e)
        sc.reset_table()
        sc.gen_eq_table(rs, qs, last_q)
        g = sc.round_coeffs(1)
        for i in range(1, ell + 1):
            assert g == linear_mle_coeffs(tt, ee, ell, i, Q), (tag, step, i)
            r = uniform_scalar(rng, Q) if not (step == 1 and i == 1) else Q - 1
            linear_mle_fold(tt, ee, ell, i, r, Q)
            live = 1 << (ell - i)
            if fused and i < ell:
                g = sc.fold_and_next_coeffs(i, r)
            else:
                sc.fold(i, r)
                if i < ell:
                    g = sc.round_coeffs(i + 1)
            if i <= 2:
                assert sc.read(0, live) == tt[:live], (tag, step, i)
        assert sc.read(0, 1) == [tt[0]] and sc.read(1, 1) == [ee[0]], (tag, step)


@pytest.mark.parametrize("ell,nq", [(4, 2), (6, 2), (7, 5), (10, 7), (12, 33), (13, 17)])
def test_hybrid_parts_vs_oracle(ell, nq, gpu_lib, experiment_build, monkeypatch):
    """(a) The hybrid-shaped table given as parts, the structured path forced on: ell = 4 has fewer than 64 columns (an atomic per
    offending entry), ell = 12 and 13 have 64 (the first size with one atomic per 64 entries)."""
    from reef_amd.sumcheck import SumCheck
    monkeypatch.setenv("REEF_SC_RANK1_MIN_POW", "1")
    rng = SplitMix64(ell * 263 + nq)
    parts, t = _hybrid_parts(ell, rng)
    rs, qs, last_q = _eq_inputs(ell, nq, rng)
    with SumCheck("pallas", ell) as sc:
        sc.set_table_parts(parts)
        assert sc.read(0, 1 << ell) == t
        _check_two_steps(sc, t, ell, rs, qs, last_q, rng, ell)


def test_parts_match_set_table_where_the_shipped_gate_opens(gpu_lib):
    """(b) Release build, ell = 22, nothing forced: the same table set with reef_sc_set_table from integers and with
    reef_sc_set_table_parts gives the same first-round coefficients, the same next two fused rounds, the same first 4096 entries
    and the same value in entry 0 after all 22 rounds.  The oracle is the old call, which this change leaves as it was."""
    from reef_amd.sumcheck import SumCheck, ints_to_array
    ell = 22
    n, half = 1 << ell, 1 << (ell - 1)
    rng = SplitMix64(2206)
    fe = ints_to_array([uniform_scalar(rng, Q) for _ in range((1 << 12) + 3)])
    fill = uniform_scalar(rng, Q)
    doc = np.random.default_rng(22).integers(0, 4, size=half - 37, dtype=np.uint8)
    whole = np.zeros((n, 4), dtype=np.uint64)
    whole[:len(fe)] = fe
    whole[len(fe):half] = ints_to_array([fill])[0]
    whole[half:half + len(doc), 0] = doc
    rs, qs, last_q = _eq_inputs(ell, 33, rng)
    challenges = [uniform_scalar(rng, Q) for _ in range(ell)]
    seen = []
    for route in ("integers", "parts"):
        with SumCheck("pallas", ell) as sc:
            if route == "integers":
                sc.set_table(0, whole)
            else:
                sc.set_table_parts([("fe", fe), ("fill", fill, half - len(fe)), ("symbols", doc)])
            sc.gen_eq_table(rs, qs, last_q)
            got = [sc.read(0, 4096), sc.round_coeffs(1)]
            for i in range(1, ell):
                g = sc.fold_and_next_coeffs(i, challenges[i - 1])
                if i <= 2:
                    got.append(g)
            sc.fold(ell, challenges[ell - 1])
            got.append(sc.read(0, 1))
            seen.append(got)
    assert seen[0] == seen[1]
    assert len(seen[0]) == 5 and seen[0][1] != (0, 0, 0)


def test_row_classes_at_their_edges(gpu_lib, experiment_build, monkeypatch):
    """(c) ell = 10, rows of 32: the largest small symbols (S), one entry of 2^30 (W), 0xFFFFFFFF (not small), a fill of 2^30 or more
    (K, not S), a fill of 5 (K and S), a fill of q - 1, a constant row whose last entry belongs to the next part (not K), and symbols
    that happen to be all equal (K)."""
    from reef_amd.sumcheck import SumCheck
    monkeypatch.setenv("REEF_SC_RANK1_MIN_POW", "1")
    ell, cols = 10, 32
    rng = SplitMix64(1010)
    row_s = [(1 << 30) - 1 - (rng.next() % 3) for _ in range(cols)]
    row_w = [rng.next() % 4 for _ in range(cols - 1)] + [1 << 30]
    row_f = [0xFFFFFFFF] * cols
    tail = [9] + [3] * cols + [rng.next() % 7 for _ in range(8 * cols + 5)]      # ends row 6, all of row 7, rows of symbols
    parts = [("symbols", np.array(row_s + row_w + row_f, dtype=np.uint32)), ("fill", (1 << 30) + 12345, cols), ("fill", 5, cols),
             ("fill", Q - 1, cols), ("fill", 7, cols - 1), ("symbols", np.array(tail, dtype=np.uint8)),
             ("fe", [uniform_scalar(rng, Q) for _ in range(cols - 5)])]
    t = _written_out(parts, 1 << ell)
    rs, qs, last_q = _eq_inputs(ell, 9, rng)
    with SumCheck("pallas", ell) as sc:
        sc.set_table_parts(parts)
        _check_two_steps(sc, t, ell, rs, qs, last_q, rng, "edges")


def _geometry_cases(rng, n):
    from reef_amd.msm import DeviceBuffer
    dev_syms = np.array([rng.next() % 256 for _ in range(202)], dtype=np.uint8)
    d = DeviceBuffer.from_host(dev_syms)
    eight = [("fe", [uniform_scalar(rng, Q) for _ in range(5)]), ("symbols", np.array([rng.next() % 256 for _ in range(13)], dtype=np.uint8)),
             ("fill", uniform_scalar(rng, Q), 27), ("symbols", np.array([rng.next() % 65536 for _ in range(50)], dtype=np.uint16)),
             ("symbols", np.array([rng.next() % (1 << 32) for _ in range(7)], dtype=np.uint32)), ("symbols", np.zeros(0, dtype=np.uint8)),
             ("fill", 11, 33), ("symbols", np.array([rng.next() % 256 for _ in range(n - 135)], dtype=np.uint8))]
    assert sum(len(p[1]) if p[0] != "fill" else p[2] for p in eight) == n
    odd = [("symbols", np.array([1, 2, 3], dtype=np.uint8)), ("symbols", d.ptr + 1, np.uint8, 201), ("fill", 10, 10)]
    odd_out = [1, 2, 3] + [int(v) for v in dev_syms[1:]] + [10] * 10
    return d, [("eight parts, one of them empty, up to the last entry", eight, _written_out(eight, n)),
               ("no parts", [], [0] * n),
               ("device symbols at an odd address", odd, odd_out + [0] * (n - len(odd_out))),
               ("one short run of 2-byte symbols", [("symbols", np.arange(77, dtype=np.uint16) * 700)], [700 * i for i in range(77)] + [0] * (n - 77))]


def test_part_geometry(gpu_lib, either_build, monkeypatch):
    """(d) ell = 8: eight parts, a part of count 0, a total equal to the table length, no parts at all, a device symbol part at an
    odd byte address, counts that are no multiple of 4 or 16 -- each against reef_sc_set_table on the table written out."""
    from reef_amd.sumcheck import SumCheck
    monkeypatch.setenv("REEF_SC_RANK1_MIN_POW", "1")
    ell = 8
    n = 1 << ell
    rng = SplitMix64(808)
    keep, cases = _geometry_cases(rng, n)
    rs, qs, last_q = _eq_inputs(ell, 3, rng)
    for what, parts, t in cases:
        with SumCheck("pallas", ell) as old, SumCheck("pallas", ell) as new:
            new.set_table(0, [uniform_scalar(rng, Q) for _ in range(n)])      # whatever was there before is gone
            old.set_table(0, t)
            new.set_table_parts(parts)
            assert new.read(0, n) == old.read(0, n) == t, what
            old.gen_eq_table(rs, qs, last_q)
            new.gen_eq_table(rs, qs, last_q)
            assert new.round_coeffs(1) == old.round_coeffs(1), what
    keep.free()


@pytest.mark.parametrize("ell,nq", [(10, 7), (9, 4)])
def test_gen_eq_before_set_table_parts_gives_the_same_step(ell, nq, gpu_lib, experiment_build, monkeypatch):
    """(e) The results do not depend on the order of the calls: gen_eq_table first, then the parts -- also when they replace a
    table without structure that was there at gen_eq_table time."""
    from reef_amd.sumcheck import SumCheck
    monkeypatch.setenv("REEF_SC_RANK1_MIN_POW", "1")
    rng = SplitMix64(ell * 977 + nq + 1)
    parts, t = _hybrid_parts(ell, rng)
    n = 1 << ell
    dense = [uniform_scalar(rng, Q) for _ in range(n)]
    rs, qs, last_q = _eq_inputs(ell, nq, rng)
    e = gen_eq_table(rs, qs, last_q, Q)
    for first in (None, dense):
        with SumCheck("pallas", ell) as sc:
            if first is not None:
                sc.set_table(0, first)
            sc.gen_eq_table(rs, qs, last_q)
            sc.set_table_parts(parts)
            tt, ee = list(t), list(e)
            g = sc.round_coeffs(1)
            for i in range(1, ell + 1):
                assert g == linear_mle_coeffs(tt, ee, ell, i, Q), (first is None, i)
                r = uniform_scalar(rng, Q)
                linear_mle_fold(tt, ee, ell, i, r, Q)
                if i < ell:
                    g = sc.fold_and_next_coeffs(i, r)
                else:
                    sc.fold(i, r)
            assert sc.read(0, 1) == [tt[0]] and sc.read(1, 1) == [ee[0]]


def test_argument_errors_leave_the_table_usable(gpu_lib):
    """(f) Every argument error is REEF_ERR_ARG with a message, found before the ctx is touched: the table set before still gives
    its round-one coefficients."""
    from reef_amd import _ffi
    from reef_amd.msm import DeviceBuffer
    from reef_amd.sumcheck import SumCheck, ints_to_array
    ell = 8
    n = 1 << ell
    rng = SplitMix64(88)
    t = [rng.next() % 131 for _ in range(n)]
    rs, qs, last_q = _eq_inputs(ell, 3, rng)
    syms = np.arange(16, dtype=np.uint8)
    wide = np.arange(n + 1, dtype=np.uint16)
    one = ints_to_array([5])
    d = DeviceBuffer(64)
    P = _ffi.ScPart

    def sym(arr, count=None, eb=None, ptr=None, loc=_ffi.REEF_HOST):
        return P(_ffi.SC_PART_SYMBOLS, arr.dtype.itemsize if eb is None else eb, arr.ctypes.data if ptr is None else ptr, len(arr) if count is None else count, loc)
    bad = {
        "more than REEF_SC_MAX_PARTS parts": ([sym(syms)] * (_ffi.SC_MAX_PARTS + 1), None),
        "an unknown kind": ([P(7, 0, one.ctypes.data, 1, _ffi.REEF_HOST)], None),
        "symbols of 3 bytes": ([sym(syms, eb=3)], None),
        "a count without data": ([P(_ffi.SC_PART_FE, 0, None, 4, _ffi.REEF_HOST)], None),
        "device symbols of 2 bytes at an odd address": ([sym(wide, count=8, ptr=d.ptr + 1, loc=_ffi.REEF_DEVICE)], None),
        "more entries than the table has": ([sym(syms), sym(wide, count=n - 15)], None),
        "no parts array": (None, 1),
    }
    with SumCheck("pallas", ell) as sc:
        sc.set_table(0, t)
        sc.gen_eq_table(rs, qs, last_q)
        want = sc.round_coeffs(1)
        assert want == linear_mle_coeffs(t, gen_eq_table(rs, qs, last_q, Q), ell, 1, Q)
        for what, (parts, nparts) in bad.items():
            arr = (P * len(parts))(*parts) if parts is not None else None
            status = sc._lib.reef_sc_set_table_parts(sc._h, arr, len(parts) if nparts is None else nparts)
            assert status == 1, (what, status)                                  # REEF_ERR_ARG
            assert sc._lib.reef_last_error(), what
            assert sc.round_coeffs(1) == want, what
        with pytest.raises(_ffi.ReefError):
            sc.set_table_parts([("fill", 1, n + 1)])
        assert sc.round_coeffs(1) == want
    d.free()
    assert ctypes.sizeof(P) == 32
