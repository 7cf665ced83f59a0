"""The verifier's key of a committed document on the GPU (reef_hyrax_vk_*, include/reef_msm.h 3n; reef_amd.verify.HyraxVk) against
oracle/: comm_LZ[t] = sum_i eq(points[t])_i C_i, every comparison bit-exact on the normalised points -- the eq weights built as
tests/test_gpu_hyrax_eval.py builds them (oracle.spartan_oracle.eq_evals), through the oracle's MSM over the rows.  The rows are
the oracle's own arithmetic progression of points and their encodings the oracle's; up to 64 rows the MSM runs over the oracle's
DECODING of those encodings (it is asserted to give the points back), above that over the points themselves, since a Python
square root per row would take longer than everything else in the file.

The row pipeline (engine.inc, v_msm_rows) switches forms by row_len (rows of 8192 entries and more are sorted as whole MSMs, in
batches of at most 64), by rows (a single row takes the single-MSM routes: nibble tables, byte tables, the bucket pipeline) and by
rows x (bucket keys per row) against MAX_SCAN_KEYS (beyond it the rows run one by one).  `_thresholds` restates that arithmetic
from the constants in the sources, and the shapes below sit on both sides of each."""
import ctypes
import functools
import os
import random
import re
import threading

import numpy as np
import pytest

from decompress_inputs import CURVE_OF, FIELDS, R256, non_residue_xs
from gpu_drivers import hyrax_points, key_of_kind, row_comms
from oracle import pasta_ref
from oracle.ipa_oracle import compress, gens_of, msm
from oracle.r1cs_oracle import field
from oracle.spartan_oracle import Challenger, eq_evals
from reef_amd._fe import _arr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = bytes(32)
PRE = dict(bucket_groups=1, byte_tables=2)          # a pre-shifted key, as gpu_drivers.key_of_kind("pre") makes it
TABLES = dict(bucket_groups=1, byte_tables=1)       # the same with byte tables


# ------------------------------------------------------------------------------------------------------------ rows and the reference
@functools.lru_cache(maxsize=None)
def _rows(curve, left, seed=0, identities=()):
    """(affine ABI rows, their 32-byte encodings by the oracle); the rows listed in `identities` are the identity (32 zero bytes)"""
    n = 1 << left
    aff = pasta_ref.gen_bases_ap(curve, 1000 + 17 * left + seed, 3, n)
    one = np.frombuffer((R256 % FIELDS[curve]).to_bytes(32, "little"), dtype=np.uint64)
    jac = np.concatenate([aff, np.tile(one, (n, 1))], axis=1)
    for i in identities:
        aff[i] = 0
        jac[i] = 0
    enc = pasta_ref.compress(curve, np.ascontiguousarray(jac))
    assert all(enc[32 * i:32 * i + 32] == IDENTITY for i in identities)
    if n <= 64:                                      # the oracle's decoding gives the rows back
        cv = CURVE_OF[curve]
        dec = b"".join(cv.affine_to_bytes(None if enc[32 * i:32 * i + 32] == IDENTITY else cv.decompress(enc[32 * i:32 * i + 32])) for i in range(n))
        assert dec == aff.tobytes()
    aff.setflags(write=False)
    return aff, enc


_WANT = {}                                           # (curve, rows, point) -> encoding: every reference sum is computed once per session


def _want(curve, aff, points):
    """the encodings of sum_i eq(point)_i C_i, one oracle MSM per DISTINCT point; identity rows drop out of the sum"""
    p = field(curve)
    live = [i for i in range(aff.shape[0]) if aff[i].any()]
    rows_id = hash(aff.tobytes())
    out = []
    for pt in points:
        key = (curve, rows_id, tuple(pt))
        if key not in _WANT:
            w = eq_evals(pt, p)
            _WANT[key] = compress(curve, msm(curve, aff[live], [w[i] for i in live])) if live else IDENTITY
        out.append(_WANT[key])
    return out


def _points(curve, left, m, seed):
    p = field(curve)
    rng = random.Random(1000 * seed + 10 * left + curve)
    return [[rng.randrange(p) for _ in range(left)] for _ in range(m)]


def _check(curve, vk, aff, points, what=""):
    from reef_amd import msm as rmsm
    jac, enc = vk.comm_lz(points)
    want = _want(curve, aff, points)
    assert enc == want, f"comm_lz32 {what}"
    assert [compress(curve, j) for j in jac] == want, f"comm_lz {what}"
    assert rmsm.normalize(curve, jac, affine=False, compressed=True)[1].tobytes() == b"".join(want), f"reef_normalize of comm_lz {what}"
    only_jac, none = vk.comm_lz(points, compressed=False)
    assert none is None and [compress(curve, j) for j in only_jac] == want, f"comm_lz alone {what}"


# ------------------------------------------------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("curve", [0, 1])
@pytest.mark.parametrize("left", [1, 2, 5])
def test_small_shapes_against_the_oracle(gpu_lib, curve, left):
    from reef_amd.verify import HyraxVk
    aff, enc = _rows(curve, left)
    with HyraxVk(curve, enc, left) as vk:
        for m in (1, 2, 3, 5):
            _check(curve, vk, aff, _points(curve, left, m, m), f"left = {left}, m = {m}")


def _const(name, text):
    return int(re.search(name + r"\s*=\s*(\d+)", text).group(1))


def _thresholds():
    """(MAX_SCAN_KEYS, the row_len from which rows are sorted as whole MSMs, rows per batch there, bucket keys per row of a plain key's
    rows of 2 entries, of a pre-shifted key's rows, of a plain key's rows of 2^11 entries): the arithmetic of v_msm_rows for full-width scalars, from the sources' constants"""
    eng = open(os.path.join(ROOT, "reef_amd", "csrc", "engine.inc")).read()
    ker = open(os.path.join(ROOT, "reef_amd", "csrc", "msm_plan.h")).read()         # the pipeline's constants, kernels' and engine's alike
    max_scan = _const("SCAN_BLOCK", ker) * _const("SCAN_ITEMS", ker) * 1024
    assert "MAX_SCAN_KEYS = SCAN_TILE * 1024" in ker and "SCAN_TILE = SCAN_BLOCK * SCAN_ITEMS" in ker
    assert "MAX_SCAN_KEYS =" not in eng and "SCAN_TILE =" not in eng + open(os.path.join(ROOT, "reef_amd", "csrc", "msm_kernels.inc")).read()
    long_rows = int(re.search(r"rows > 1 && row_len >= (\d+) && bits \+ 1 > 13", eng).group(1))
    per_batch = int(re.search(r"\(size_t\)\(\(\(1ull << 31\) - 1\) / \(\(u64\)row_len \* key->W\)\), \(size_t\)(\d+)\}\)", eng).group(1))

    def plain_keys(n):                               # choose_window(n, 0) capped at 11, G = W = ceil(256 / c)
        best, best_c = None, 0
        for c in range(3, 21):
            w = (256 + c - 1) // c
            cost = (255 // c + (0.5 if 255 % c == 0 else 1.0)) * n + 4.0 * w * (1 << (c - 1))
            if best is None or cost < best:
                best, best_c = cost, c
        c = min(best_c, 11)
        return ((256 + c - 1) // c) << (c - 1)
    pre_keys = 1 << (13 - 1)                         # choose_window(n, 1) = 13 below 61440 points, one bucket group
    return max_scan, long_rows, per_batch, plain_keys(2), pre_keys, plain_keys(1 << 11)


def test_the_thresholds_are_the_ones_this_file_assumes():
    max_scan, long_rows, per_batch, plain2, pre, plain2048 = _thresholds()
    assert (max_scan, long_rows, per_batch, plain2, pre, plain2048) == (1 << 22, 8192, 64, 344, 4096, 4096)


@pytest.mark.parametrize("curve", [0, 1])
def test_row_len_threshold_and_reefs_own_size(gpu_lib, curve):
    """left = 12 and 13 (rows of 4096 and 8192 entries: the LDS row sort / whole MSMs), a single point (the single-MSM route) and two;
    left = 13, m = 2 is Reef's own size.  Then 65 points at left = 13: the whole-MSM route's second batch (two distinct points, so that
    the oracle runs two MSMs)."""
    from reef_amd.verify import HyraxVk
    assert _thresholds()[1] == 1 << 13 and _thresholds()[2] == 64
    for left in (12, 13):
        aff, enc = _rows(curve, left)
        with HyraxVk(curve, enc, left) as vk:
            pts = _points(curve, left, 2, 7)
            _check(curve, vk, aff, pts[:1], f"left = {left}, m = 1")
            _check(curve, vk, aff, pts, f"left = {left}, m = 2")
            if left == 13:
                many = [pts[t % 2] for t in range(65)]
                jac, got = vk.comm_lz(many)
                assert got == _want(curve, aff, many), "left = 13, m = 65"


def _many_two_entry_rows(curve, vk, aff, m, seed):
    """m points over two rows against the oracle's row MSM (one call for all of them)"""
    p = field(curve)
    rng = random.Random(seed)
    xs = [rng.randrange(p) for _ in range(m)]
    sc = _arr([w for x in xs for w in ((1 - x) % p, x)])
    want = pasta_ref.compress(curve, pasta_ref.row_msm(curve, np.ascontiguousarray(aff), sc, m, 2, mont=False, threads=4))
    jac, enc = vk.comm_lz([[x] for x in xs])
    assert b"".join(enc) == want, f"m = {m}"
    assert pasta_ref.compress(curve, np.ascontiguousarray(jac)) == want, f"m = {m}, Jacobian"


@pytest.mark.parametrize("curve", [0, 1])
def test_rows_times_keys_threshold_on_a_pre_shifted_key(gpu_lib, curve):
    """A pre-shifted key has 4096 bucket keys per row: 1024 points are the last batch the row sort takes whole, 1025 run one by one.  A
    key of two rows also has nibble tables: m = 1 takes them."""
    from reef_amd.verify import HyraxVk
    max_scan, _, _, _, pre, _ = _thresholds()
    edge = max_scan // pre
    aff, enc = _rows(curve, 1)
    with HyraxVk(curve, enc, 1, **PRE) as vk:
        _check(curve, vk, aff, _points(curve, 1, 1, 1), "nibble tables")
        _check(curve, vk, aff, _points(curve, 1, 2, 2), "m = 2")
        _many_two_entry_rows(curve, vk, aff, edge, 31)
        _many_two_entry_rows(curve, vk, aff, edge + 1, 32)
        _check(curve, vk, aff, _points(curve, 1, 3, 3), "m = 3 after the large batches")


@pytest.mark.parametrize("curve", [0, 1])
def test_rows_times_keys_threshold_on_the_default_key(gpu_lib, curve):
    """The default (plain) key sorts rows of 2^11 entries into 4096 bucket keys each, the most a row below the row_len threshold gets
    (the smallest m that reaches MAX_SCAN_KEYS): 1024 points are the last whole batch, 1025 run one by one.  Two distinct points, so
    that the oracle runs two MSMs; each appears at both ends of the batch."""
    from reef_amd.verify import HyraxVk
    max_scan, _, _, _, _, plain2048 = _thresholds()
    edge = max_scan // plain2048
    left = 11
    aff, enc = _rows(curve, left)
    pts = _points(curve, left, 2, 41)
    with HyraxVk(curve, enc, left) as vk:
        for m in (edge, edge + 1):
            many = [pts[(t + t // 7) % 2] for t in range(m - 2)] + [pts[1], pts[0]]
            jac, got = vk.comm_lz(many)
            assert got == _want(curve, aff, many), f"m = {m}"
            assert pasta_ref.compress(curve, np.ascontiguousarray(jac)) == b"".join(got), f"m = {m}, Jacobian"


@pytest.mark.parametrize("curve", [0, 1])
def test_key_kinds_give_the_same_points(gpu_lib, curve):
    """2^11 rows under the default key, a pre-shifted key and one with byte tables (a single point takes them)"""
    from reef_amd.verify import HyraxVk
    left = 11
    aff, enc = _rows(curve, left)
    pts = _points(curve, left, 2, 11)
    want = _want(curve, aff, pts)
    for kw in ({}, PRE, TABLES):
        with HyraxVk(curve, enc, left, **kw) as vk:
            assert vk.comm_lz(pts[:1])[1] == want[:1], kw
            assert vk.comm_lz(pts)[1] == want, kw


# ------------------------------------------------------------------------------------------------------------ 2. the existing routes
@pytest.mark.parametrize("curve", [0, 1])
def test_agreement_with_the_existing_routes(gpu_lib, curve):
    """comm_lz32[t] = compress(comm_lz[t]) = verify.comm_lz for the same rows = reef_hyrax_eval_comm_compressed on a ctx with a document"""
    from reef_amd import msm as rmsm
    from reef_amd import verify
    from reef_amd.hyrax import HyraxEval
    p = field(curve)
    left, num_vars = 4, 5
    aff, enc = _rows(curve, left)
    pts = _points(curve, left, 3, 21)
    z = np.random.default_rng(5).integers(0, 256, size=1 << num_vars, dtype=np.uint64).astype(np.uint8)
    with verify.HyraxVk(curve, enc, left) as vk, HyraxEval(curve, z, num_vars, left) as hx, key_of_kind(curve, gens_of(curve, 2)[0], "plain") as key:
        jac, enc32 = vk.comm_lz(pts)
        for t, pt in enumerate(pts):
            assert enc32[t] == rmsm.compress(curve, jac[t])
            assert enc32[t] == rmsm.compress(curve, verify.comm_lz(curve, enc, pt, p)), "verify.comm_lz"
            hx.eval_begin(key, pt + [7])
            assert enc32[t] == rmsm.compress(curve, hx.eval_comm_compressed(enc)), "reef_hyrax_eval_comm_compressed"
        assert enc32 == _want(curve, aff, pts)


# ------------------------------------------------------------------------------------------------------------ 3. degenerate inputs
@pytest.mark.parametrize("curve", [0, 1])
def test_degenerate_points_and_rows(gpu_lib, curve):
    from reef_amd.msm import DeviceBuffer
    from reef_amd.verify import HyraxVk
    p = field(curve)
    left = 3
    rnd = _points(curve, left, 4, 9)
    zeros, ones, top = [0] * left, [1] * left, [p - 1] * left
    mixed = [0, p - 1, 1]
    batch = [zeros, ones, top, rnd[0], mixed, rnd[0], rnd[1]]          # rnd[0] twice in one batch
    R = R256 % p
    for ids in ((), (0, 5), (7,)):
        aff, enc = _rows(curve, left, 1, ids)
        with HyraxVk(curve, enc, left) as vk, HyraxVk(curve, DeviceBuffer.from_host(np.frombuffer(enc, np.uint8)), left) as vk_dev:
            _check(curve, vk, aff, batch, f"identities {ids}")
            want = _want(curve, aff, batch)
            assert want[0] == enc[:32], "a point of zeros: the weight is 1 on row 0 only"
            assert want[1] == enc[-32:], "a point of ones: row 2^left - 1"
            assert vk_dev.comm_lz(batch)[1] == want, "device rows"
            assert vk.comm_lz([[x * R % p for x in pt] for pt in batch], is_mont=True)[1] == want, "Montgomery form"
            for m in (2, 9, 1):                                        # larger, then smaller: the buffers are reused
                pts = (batch + rnd)[:m]
                assert vk.comm_lz(pts)[1] == _want(curve, aff, pts), f"m = {m} on the same vk"
            jac0, enc0 = vk.comm_lz([])
            assert jac0.shape == (0, 12) and enc0 == [], "no points: no call, nothing back"
    everything = tuple(range(1 << left))
    aff, enc = _rows(curve, left, 2, everything)
    assert enc == IDENTITY * (1 << left)
    with HyraxVk(curve, enc, left) as vk:
        jac, got = vk.comm_lz(batch)
        assert got == [IDENTITY] * len(batch), "a key of identities"
        assert [compress(curve, j) for j in jac] == [IDENTITY] * len(batch)


# ------------------------------------------------------------------------------------------------------------ 4. the contract's errors
def _raw_create(lib, curve, ptr, left, loc, device=-1):
    h = ctypes.c_void_p()
    st = lib.reef_hyrax_vk_create(ctypes.byref(h), curve, ptr, left, loc, device, None)
    return st, h, lib.reef_last_error().decode()


@pytest.mark.parametrize("curve", [0, 1])
def test_create_errors_leave_out_null(gpu_lib, curve):
    from reef_amd._ffi import REEF_DEVICE, REEF_HOST
    from reef_amd.msm import DeviceBuffer
    from reef_amd.verify import HyraxVk
    lib = gpu_lib
    left = 4
    aff, enc = _rows(curve, left)
    host = np.frombuffer(enc, np.uint8).copy()
    for bad_left in (0, 26):
        st, h, msg = _raw_create(lib, curve, host.ctypes.data, bad_left, REEF_HOST)
        assert st == 1 and not h.value and "left_vars" in msg and "1 .. 25" in msg, msg
    j = 11
    x = non_residue_xs(curve)[1]
    bad = host.copy()
    bad[32 * j:32 * j + 32] = np.frombuffer((x | 1 << 255).to_bytes(32, "little"), np.uint8)
    bad[32 * 13:32 * 14] = np.frombuffer((x | 1 << 255).to_bytes(32, "little"), np.uint8)
    for loc, ptr, keep in ((REEF_HOST, bad.ctypes.data, bad), (REEF_DEVICE, None, DeviceBuffer.from_host(bad))):
        st, h, msg = _raw_create(lib, curve, ptr if ptr is not None else keep.ptr, left, loc)
        assert st == 1 and not h.value, msg
        assert re.search(rf"row {j} is not the encoding of a point \(2 such rows\)", msg), msg
    dbuf = DeviceBuffer.from_host(np.concatenate([np.zeros(8, np.uint8), host]))
    st, h, msg = _raw_create(lib, curve, dbuf.ptr + 8, left, REEF_DEVICE)
    assert st == 1 and not h.value and "16-byte aligned" in msg, msg
    st, h, msg = _raw_create(lib, curve, host.ctypes.data, left, REEF_HOST, device=99)
    assert st == 1 and not h.value and "device" in msg, msg
    st, h, msg = _raw_create(lib, 7, host.ctypes.data, left, REEF_HOST)
    assert st == 1 and not h.value and "curve" in msg, msg
    with HyraxVk(curve, enc, left) as vk:                             # the library serves a good key after all of that
        _check(curve, vk, aff, _points(curve, left, 2, 3), "after the refused keys")


@pytest.mark.parametrize("curve", [0, 1])
def test_comm_lz_errors_write_nothing_and_leave_the_vk_usable(gpu_lib, curve):
    from reef_amd.verify import HyraxVk
    lib = gpu_lib
    p = field(curve)
    left = 5
    aff, enc = _rows(curve, left)
    good = _points(curve, left, 3, 5)
    with HyraxVk(curve, enc, left) as vk:
        def call(points_arr, m, jac=True, enc32=True, is_mont=False):
            j = np.full((max(m, 1) if m < 64 else 1, 12), 0xA5A5A5A5A5A5A5A5, np.uint64)
            e = np.full((max(m, 1) if m < 64 else 1, 32), 0x5A, np.uint8)
            st = lib.reef_hyrax_vk_comm_lz(vk._h, None if points_arr is None else points_arr.ctypes.data, m, is_mont,
                                           j.ctypes.data if jac else None, e.ctypes.data if enc32 else None)
            untouched = bool((j == 0xA5A5A5A5A5A5A5A5).all() and (e == 0x5A).all())
            return st, lib.reef_last_error().decode(), untouched
        pa = _arr([x for pt in good for x in pt])
        cases = []
        late = [list(pt) for pt in good]
        late[1][2] = p                                                # the modulus itself
        cases.append((call(_arr([x for pt in late for x in pt]), 3), r"points\[1\]\[2\] is not below the modulus"))
        late[1][2] = (1 << 256) - 1
        cases.append((call(_arr([x for pt in late for x in pt]), 3, is_mont=True), r"points\[1\]\[2\] is not below the modulus"))
        cases.append((call(pa, 1 << (31 - left)), r"reaches 2\^31"))   # refused before a point is read: the array is never indexed
        cases.append((call(pa, 3, jac=False, enc32=False), "both NULL"))
        cases.append((call(None, 3), "null argument"))
        for (st, msg, untouched), pattern in cases:
            assert st == 1 and re.search(pattern, msg) and untouched, (st, msg, pattern)
            _check(curve, vk, aff, good, f"after the error '{pattern}'")
        st, _, untouched = call(pa, 0)
        assert st == 0 and untouched, "m = 0 is REEF_OK with nothing written"
    assert lib.reef_hyrax_vk_comm_lz(None, pa.ctypes.data, 1, False, pa.ctypes.data, None) == 1
    lib.reef_hyrax_vk_destroy(None)                                   # a null vk is destroyed quietly


# ------------------------------------------------------------------------------------------------------------ 5. verify_eval_batch
@pytest.mark.parametrize("curve", [0, 1])
def test_verify_eval_batch_with_vk_instances(gpu_lib, curve):
    """Three arguments of the device prover over ONE document at three points, as tests/test_gpu_ipa_check_batch.py makes them: accepted
    through one vk with exactly one reef_hyrax_vk_comm_lz call, a wrong evaluation found, and every verdict that of the row_comms32 route"""
    from reef_amd.hyrax import HyraxEval, prove_eval
    from reef_amd.verify import HyraxVk, verify_eval, verify_eval_batch
    p = field(curve)
    num_vars, left = 6, 3
    right = num_vars - left
    gens, _ = gens_of(curve, 1 << right)
    q0, h = hyrax_points(curve)

    def q_of(r):
        return pasta_ref.to_affine(curve, pasta_ref.scalar_mul(curve, q0, r))[0]

    def weights(absorbed):
        ch = Challenger(p, 99)
        return [ch("rho", item) or 1 for item in absorbed]
    rng = random.Random(500 + curve)
    ints = [rng.randrange(p) for _ in range((1 << num_vars) - 1)]
    rc = row_comms(curve, gens, ints, num_vars, left, None, h)
    rc32 = b"".join(compress(curve, pasta_ref.scalar_mul(curve, a, 1)) for a in rc)
    with key_of_kind(curve, gens, "pre") as key, HyraxVk(curve, rc32, left) as vk:
        calls = []
        inner = vk.comm_lz

        def counted(points, *a, **kw):
            calls.append(len(points))
            return inner(points, *a, **kw)
        vk.comm_lz = counted
        base = []
        with HyraxEval(curve, _arr(ints), num_vars, left) as hx:
            for i in range(3):
                point = [rng.randrange(p) for _ in range(num_vars)]
                pf = prove_eval(hx, key, point, Challenger(p, 3 + i), p, q_of, row_comms=rc)
                base.append(dict(point=point, left=left, eval=pf["eval"], proof=pf, q=q_of(pf["r_ipa"])))

        def insts(route, tamper=None):
            out = []
            for i, b in enumerate(base):
                it = dict(b, **({"vk": vk} if route == "vk" else {"row_comms32": rc32}))
                if i == 0:                                            # the first one re-draws its challenges, the others bring them
                    it.update(q=None, challenge=Challenger(p, 3), q_of=q_of)
                if i == tamper:
                    it["eval"] = (it["eval"] + 1) % p
                out.append(it)
            return out
        assert verify_eval_batch(key, insts("vk"), p, weights) is True
        assert calls == [3], "one reef_hyrax_vk_comm_lz call for the three instances of one vk"
        assert verify_eval_batch(key, insts("vk"), p, weights, each=True) == (True, [True] * 3)
        assert verify_eval_batch(key, insts("vk", tamper=1), p, weights, each=True) == (False, [True, False, True])
        assert calls == [3, 3, 3]
        for tamper in (None, 0, 2):
            assert verify_eval_batch(key, insts("vk", tamper), p, weights, each=True) == verify_eval_batch(key, insts("rows", tamper), p, weights, each=True)
        mixed = insts("vk")[:2] + insts("rows")[2:]
        del calls[:]
        assert verify_eval_batch(key, mixed, p, weights) is True and calls == [2]
        one = insts("vk")[1]                                          # verify_eval takes the vk where it takes the rows
        assert verify_eval(key, one["q"], vk, one["point"], left, one["eval"], one["proof"], p) is True
        assert verify_eval(key, one["q"], vk, one["point"], left, (one["eval"] + 1) % p, one["proof"], p) is False
        assert verify_eval(key, one["q"], rc32, one["point"], left, one["eval"], one["proof"], p) is True


# ------------------------------------------------------------------------------------------------------------ 6. two vks, two threads
def test_two_vks_from_two_threads(gpu_lib):
    from reef_amd.verify import HyraxVk
    jobs = []
    for curve, left in ((0, 6), (1, 4)):
        aff, enc = _rows(curve, left, 3)
        pts = _points(curve, left, 5, 13)
        jobs.append((curve, left, enc, pts, _want(curve, aff, pts)))
    got, errors = {}, []
    start = threading.Barrier(2)

    def work(k, vk, pts):
        try:
            start.wait()
            got[k] = [vk.comm_lz(pts[:1 + r % 5])[1] for r in range(40)]
        except Exception as e:                                        # noqa: BLE001 -- reported by the assertion below
            errors.append(repr(e))
    with HyraxVk(jobs[0][0], jobs[0][2], jobs[0][1]) as a, HyraxVk(jobs[1][0], jobs[1][2], jobs[1][1], **PRE) as b:
        ts = [threading.Thread(target=work, args=(k, vk, jobs[k][3])) for k, vk in enumerate((a, b))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    assert not errors, errors
    for k in (0, 1):
        assert got[k] == [jobs[k][4][:1 + r % 5] for r in range(40)], f"vk {k}"
