"""The decisions of the sum-check engine (reef_amd/csrc/sumcheck_plan.h: the switches from their text, the grids, the row lists of a structured table,
and sc_round_plan -- which route a round takes) on the host, compiled with g++ (csrc/tools/sc_plan_check.cpp).  Runs without a GPU.  Plans derived
BY HAND from the text of v_sc_coeffs, v_sc_fold and v_sc_fold_coeffs as it stood before the plan was split off (both sides of every branch; the
derivations are in the comments), whole steps walked on the host with the invariants a step must keep, the row lists against a direct transcription of
their definitions, the switch parser at its clamps, and everything once more through the same functions built as a program of its own with
-fsanitize=address,undefined."""
import ctypes
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reef_amd", "csrc")
LIBDIR = os.path.join(ROOT, "reef_amd", "_lib")
SO = os.path.join(LIBDIR, "libreef_scplancheck.so")
EXE = os.path.join(LIBDIR, "sc_plan_check_san")
SRC = os.path.join(CSRC, "tools", "sc_plan_check.cpp")
DEPS = [SRC, os.path.join(CSRC, "sumcheck_plan.h"), os.path.join(CSRC, "msm_plan.h")]
COEFFS, FOLD, FOLD_COEFFS = 0, 1, 2             # sumcheck_plan.h: ScCall
(SUMS_STRUCT, SUMS_R1, SUMS_DENSE, FOLD_R1, FOLD_DENSE, FC_R1, FC_STRUCT, FC_DEFER, FC_SECOND, FC_LAST_R1, FC_SPLIT, FC_DENSE) = range(12)   # ScRoute
ROUTE_NAMES = "SUMS_STRUCT SUMS_R1 SUMS_DENSE FOLD_R1 FOLD_DENSE FC_R1 FC_STRUCT FC_DEFER FC_SECOND FC_LAST_R1 FC_SPLIT FC_DENSE".split()
# every variable unset
SWITCHES = dict(one_launch=1, rank1=1, structured=1, identity=1, defer=1, r1_min_pow=1 << 21, floor_blocks=256, one_launch_max=64, split_max=1 << 14,
                split_blocks=64, items=8, order=2, set_sub=8, blocks_cap=2048)
LISTS = "sum0W sum0S sum0K sum1W sum1S sum1K fast gen f8 f8x frest g8 d8_0S d8_0K d8_1S d8_1K d8_2S d8_2K d8_3S d8_3K".split()
STATE = "len valid_t valid_e nblocks r1 r1_hi r1_hi0 r1_lo r1_nq r1_prev_pow fresh st_ok defer_on defer_pow defer_hq".split()


def _stale(path):
    return not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(d) for d in DEPS)


@pytest.fixture(scope="module")
def host():
    if _stale(SO):
        os.makedirs(LIBDIR, exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", SO])
    lib = ctypes.CDLL(SO)
    for f in (lib.sc_plan_in_names, lib.sc_plan_switch_names, lib.sc_plan_out_names):
        f.restype = ctypes.c_char_p
    lib.sc_plan_round.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.sc_plan_switches.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.sc_plan_grid.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]
    lib.sc_plan_row_lists.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_long]
    lib.sc_plan_row_lists.restype = ctypes.c_long
    lib.out_names = lib.sc_plan_out_names().decode().split()
    assert lib.sc_plan_in_names().decode().split() == ["call", "pow"] + STATE + LISTS
    assert lib.sc_plan_switch_names().decode().split() == list(SWITCHES)
    return lib


def sw_values(sw):
    s = dict(SWITCHES, **sw)
    assert set(s) == set(SWITCHES), sw
    return [s[k] for k in SWITCHES]


def plan_inputs(call, pow_, st, sw):
    return [call, pow_] + [int(st[k]) for k in STATE] + [int(st.get(k, 0)) for k in LISTS] + sw_values(sw)


def plan(host, call, pow_, st, **sw):
    """(status, {field: value})"""
    inp = plan_inputs(call, pow_, st, sw)
    a = (ctypes.c_int64 * len(inp))(*inp)
    out = (ctypes.c_uint64 * len(host.out_names))()
    rs = host.sc_plan_round(a, out)
    return rs, dict(zip(host.out_names, (int(v) for v in out)))


def grid_fn(host, fn, a, b=0, **sw):
    v = sw_values(sw)
    out = (ctypes.c_uint64 * 3)()
    n = host.sc_plan_grid(fn.encode(), a, b, (ctypes.c_int64 * len(v))(*v), out)
    assert n > 0, fn
    return int(out[0]) if n == 1 else tuple(int(x) for x in out[:n])


def check(host, call, pow_, st, sw=None, **want):
    rs, p = plan(host, call, pow_, st, **(sw or {}))
    assert rs == 0
    got = {k: p[k] for k in want}
    assert got == want, (ROUTE_NAMES[p["route"]], p)
    return p


def state(ell=12, **kw):
    """A step's start at 2^ell entries with EQ rank-one and a plain table: what gen_eq_table and set_table leave when REEF_SC_RANK1_MIN_POW allows."""
    n = 1 << ell
    lo = ell // 2
    st = dict(len=n, valid_t=n, valid_e=n, nblocks=min(2048, max(1, n // 512)), r1=1, r1_hi=ell - lo, r1_hi0=ell - lo, r1_lo=lo, r1_nq=0, r1_prev_pow=0, fresh=1,
              st_ok=0, defer_on=0, defer_pow=0, defer_hq=0)
    st.update(kw)
    return st


def ceil_div(a, b):
    return -(-a // b)


ZERO = dict(blocks=0, fold_blocks=0, grid_x=0, grid_y=0, rows_per_chunk=0, prep_blocks=0, hq=0, const_blocks=0, points_blocks=0, one_launch=0, ident=0, materialize=0)
MIN1 = dict(r1_min_pow=1)


# ---------------------------------------------------------------------------------------------- plans derived by hand
# The rules, as the three entry points stated them (len = 2^ell; lo = ell / 2 column bits, gx = ceil(2^lo / 256)):
#   r1_round(pow)       EQ is rank-one, r1_hi >= 1, valid_t == valid_e == 2 pow, pow >= RANK1_MIN_POW
#   struct_round(pow)   st_ok, fresh, 2 pow == len, r1_hi == r1_hi0, STRUCT
#   coeffs              flush if defer_on; error unless 2 pow <= min(valid);  r1_round and struct_round: structured sums;  r1_round: k_sc_r1_coeffs on
#                       sc_r1_grid(hn = 2^(r1_hi - 1));  else write EQ out if it is rank-one, k_sc_coeffs on dense_blocks(pow)
#   fold                flush if defer_on; error likewise;  r1_round: prep, k_sc_r1_fold on min(4096, ceil(pow / 256)), EQ written out if r1_hi is 0 then;
#                       else write EQ out if rank-one, k_sc_fold on the same count
#   fold_coeffs         error likewise;  fused = r1_round and r1_hi >= 2 and pow / 2 >= MIN_POW;  flush if defer_on and not (pow == defer_pow and fused)
#                       fused: hn = 2^(r1_hi - 2), ident = (r1_prev_pow == pow and IDENTITY);  struct_round: defer if DEFER, r1_hi >= 3, pow / 4 >= MIN_POW and
#                       f8 has rows, else fast + general lists;  else if defer_on (still): second fold;  else the general kernel on sc_r1_grid(hn)
#                       r1_round only: prep, k_sc_r1_fold, EQ written out, k_sc_coeffs on dense_blocks(pow / 2)
#                       else: write EQ out if rank-one; ONE_LAUNCH and pow / 2 <= SPLIT_MAX: split kernel on min(SPLIT_BLOCKS, ceil(pow / 2 / 64)), one launch;
#                       else k_sc_fold_coeffs on dense_blocks(pow / 2)
#   dense_blocks(w)     min(nblocks, ceil(w / 256), max(FLOOR, ceil(w / (256 ITEMS))));  one launch if ONE_LAUNCH and blocks <= ONE_LAUNCH_MAX
#   sc_r1_grid(hn)      chunks = max(1, min(hn, max(1, 1024 / gx))), rows_per_chunk = ceil(hn / chunks), grid (gx, ceil(hn / rows_per_chunk))
#   sc_list_grid(n)     (gx, max(1, min(n, max(1024 / gx, ceil(n / 256)))))
def test_round_coeffs_routes(host):
    # ell = 12: len 4096, lo = hi = 6, gx = 1, nblocks = min(2048, 4096 / 512) = 8.  First round, pow = 2048, hn = 2^5 = 32: chunks = min(32, 1024) = 32,
    # one row each, grid (1, 32).  The gate: MIN_POW = pow exactly keeps the round rank-one; one more and EQ is written out (materialize) and
    # k_sc_coeffs runs on min(8, ceil(2048 / 256) = 8, max(256, 1)) = 8 blocks, one launch (8 <= 64).
    r1 = dict(ZERO, route=SUMS_R1, flush=0, hn=32, grid_x=1, grid_y=32, rows_per_chunk=1)
    check(host, COEFFS, 2048, state(), MIN1, **r1)
    check(host, COEFFS, 2048, state(), dict(r1_min_pow=2048), **r1)
    dense = dict(ZERO, route=SUMS_DENSE, flush=0, hn=0, materialize=1, blocks=8, one_launch=1)
    check(host, COEFFS, 2048, state(), dict(r1_min_pow=2049), **dense)
    check(host, COEFFS, 2048, state(), **dense)                                              # the default gate, 2^21
    check(host, COEFFS, 2048, state(r1=0), MIN1, **dict(dense, materialize=0))              # EQ was given dense: nothing to write out
    check(host, COEFFS, 2048, state(r1_hi=0), MIN1, **dense)                                # no FH bit left
    # a round that is not the next one of the step (pow = 1024 on whole tables): valid != 2 pow -> dense, min(8, 4, 256) = 4 blocks
    check(host, COEFFS, 1024, state(), MIN1, **dict(dense, blocks=4))
    # second round after a rank-one fold: valid = 2048, r1_hi = 5 -> hn = 16
    check(host, COEFFS, 1024, state(valid_t=2048, valid_e=2048, r1_hi=5, fresh=0), MIN1, **dict(r1, hn=16, grid_y=16))
    # the structured sums: st_ok, pristine, whole tables, all FH bits.  Lists: side 0 has 3 W, 5 S, 24 K rows, side 1 is constant (32 K): grids
    # (1, min(3, max(1024, 1))) = (1, 3) and (1, 5); an empty list has no grid; the K rows of both sides in one launch of max(ceil(24/256), ceil(32/256)) = 1 x 2
    lists = dict(sum0W=3, sum0S=5, sum0K=24, sum1K=32)
    st = state(st_ok=1, **lists)
    p = check(host, COEFFS, 2048, st, MIN1, **dict(ZERO, route=SUMS_STRUCT, hn=32, const_blocks=1, g_sum0W_x=1, g_sum0W_y=3, g_sum0S_x=1, g_sum0S_y=5))
    assert p["g_sum1W_x"] == p["g_sum1W_y"] == p["g_sum1S_x"] == p["g_sum1S_y"] == 0
    check(host, COEFFS, 2048, dict(st, sum0K=0, sum1K=0), MIN1, route=SUMS_STRUCT, const_blocks=0)      # no K rows: no launch for them
    check(host, COEFFS, 2048, dict(st, sum1K=257), MIN1, route=SUMS_STRUCT, const_blocks=2)
    for other in (dict(st_ok=0), dict(fresh=0), dict(r1_hi=5)):                                       # each condition of struct_round
        check(host, COEFFS, 2048, dict(st, **other), MIN1, route=SUMS_R1)
    check(host, COEFFS, 2048, st, dict(r1_min_pow=1, structured=0), **r1)
    check(host, COEFFS, 2048, st, dict(r1_min_pow=2049), **dense)                                      # struct_round alone is not enough
    # a deferred fold is written out before any sums are taken, whatever the route
    for s, sw in ((state(defer_on=1), MIN1), (state(defer_on=1), {}), (dict(st, defer_on=1), MIN1)):
        check(host, COEFFS, 2048, s, sw, flush=1)


def test_fold_routes(host):
    # pow = 2048 of 4096: ceil(2048 / 256) = 8 blocks either way.  Rank-one while r1_hi >= 1; the fold that uses the last FH bit up writes EQ out after it.
    for hi, want in ((3, dict(route=FOLD_R1, materialize=0)), (2, dict(route=FOLD_R1, materialize=0)), (1, dict(route=FOLD_R1, materialize=1)),
                     (0, dict(route=FOLD_DENSE, materialize=1))):
        check(host, FOLD, 2048, state(r1_hi=hi), MIN1, **dict(ZERO, flush=0, hn=0, fold_blocks=8, **want))
    check(host, FOLD, 2048, state(), dict(r1_min_pow=2048), route=FOLD_R1)
    check(host, FOLD, 2048, state(), dict(r1_min_pow=2049), route=FOLD_DENSE, materialize=1)
    check(host, FOLD, 2048, state(r1=0), MIN1, route=FOLD_DENSE, materialize=0)
    check(host, FOLD, 1024, state(), MIN1, route=FOLD_DENSE, materialize=1, fold_blocks=4)              # valid != 2 pow
    check(host, FOLD, 1, state(ell=1, r1_lo=0, r1_hi=1, r1_hi0=1), MIN1, route=FOLD_R1, fold_blocks=1, materialize=1)
    check(host, FOLD, 1 << 27, state(ell=28), route=FOLD_R1, fold_blocks=4096)                           # the cap of the grid-stride folds
    check(host, FOLD, 2048, state(defer_on=1), MIN1, flush=1, route=FOLD_R1)
    check(host, FOLD, 2048, state(defer_on=1), flush=1, route=FOLD_DENSE)


def test_fold_coeffs_rank_one_routes(host):
    # pow = 2048 of 4096, r1_hi = 6: the next round (1024) stays rank-one while MIN_POW <= 1024: hn = 2^4 = 16, grid (1, 16).  One step above
    # the gate this is the last rank-one round: k_sc_r1_fold on 8 blocks, EQ written out, k_sc_coeffs over 1024 pairs on min(8, 4, 256) = 4 blocks.
    # Above 2048 the round is dense from the start: EQ written out first; 1024 pairs <= 2^14 -> split kernel on min(64, 1024 / 64) = 16 workgroups.
    fused = dict(ZERO, route=FC_R1, flush=0, hn=16, grid_x=1, grid_y=16, rows_per_chunk=1, prep_blocks=1)
    last = dict(ZERO, route=FC_LAST_R1, flush=0, hn=0, materialize=1, fold_blocks=8, blocks=4, one_launch=1)
    split = dict(ZERO, route=FC_SPLIT, flush=0, hn=0, materialize=1, blocks=16, one_launch=1)
    check(host, FOLD_COEFFS, 2048, state(), MIN1, **fused)
    check(host, FOLD_COEFFS, 2048, state(), dict(r1_min_pow=1024), **fused)
    check(host, FOLD_COEFFS, 2048, state(), dict(r1_min_pow=1025), **last)
    check(host, FOLD_COEFFS, 2048, state(), dict(r1_min_pow=2048), **last)
    check(host, FOLD_COEFFS, 2048, state(), dict(r1_min_pow=2049), **split)
    # r1_hi: 0 -> dense (EQ is still FH (x) FL with no FH bit: written out), 1 -> last rank-one round, 2 -> fused with one pair row, 3 -> two
    check(host, FOLD_COEFFS, 2048, state(r1_hi=0), MIN1, **split)
    check(host, FOLD_COEFFS, 2048, state(r1_hi=1), MIN1, **last)
    check(host, FOLD_COEFFS, 2048, state(r1_hi=2), MIN1, **dict(fused, hn=1, grid_y=1))
    check(host, FOLD_COEFFS, 2048, state(r1_hi=3), MIN1, **dict(fused, hn=2, grid_y=2))
    check(host, FOLD_COEFFS, 2048, state(r1=0), MIN1, **dict(split, materialize=0))
    # the sum-check identity: the coefficients of the round being folded are still on the device
    check(host, FOLD_COEFFS, 2048, state(r1_prev_pow=2048), MIN1, **dict(fused, ident=1))
    check(host, FOLD_COEFFS, 2048, state(r1_prev_pow=1024), MIN1, **fused)
    check(host, FOLD_COEFFS, 2048, state(r1_prev_pow=2048), dict(r1_min_pow=1, identity=0), **fused)
    check(host, FOLD_COEFFS, 2048, state(r1_prev_pow=2048), dict(r1_min_pow=1025), **last)               # only the fused rank-one routes use it
    # many rows and wide columns: ell = 28, lo = 14 -> gx = 64, at most 1024 / 64 = 16 row groups; hn = 2^12 -> 256 rows each
    check(host, FOLD_COEFFS, 1 << 27, state(ell=28), route=FC_R1, hn=4096, grid_x=64, grid_y=16, rows_per_chunk=256, prep_blocks=16)


def test_fold_coeffs_structured_deferred_and_second(host):
    # A structured table of 4096: H = 64 rows, hn = H / 4 = 16 after the first fold, h8 = 8.  Lists for rows 0 and 1 W and the rest K: a quadruple h is
    # fast unless it holds a W row -> fast = 14, gen = 2 (h = 0, 1); fast8(g) = fast(g) and fast(g + 8): g = 2..7 -> f8 = 6, f8x = 12 (h = 2..7, 10..15),
    # frest = 2 (h = 8, 9), g8 = 2 (g = 0, 1); the deferred rows are K in every source block: d8_bK = 12, d8_bS = 0.
    lists = dict(fast=14, gen=2, f8=6, f8x=12, frest=2, g8=2, d8_0K=12, d8_1K=12, d8_2K=12, d8_3K=12)
    assert {k: v[1] for k, v in row_lists(host, [0, 0] + [3] * 62)[0].items() if v[1] and not k.startswith("sum")} == lists
    st = state(st_ok=1, **lists)
    # defer: DEFER on, r1_hi = 6 >= 3, pow / 4 = 512 >= MIN_POW, f8 not empty.  Grids (gx = 1): gen (1, 2), frest (1, 2); no S rows among the deferred:
    # no k_sc_r1s_rows launch; K rows: ceil(12 / 256) = 1 block x 4 source blocks; no masses: no k_sc_defer_points; kprep / factors: ceil(16 / 256) = 1
    defer = dict(ZERO, route=FC_DEFER, flush=0, hn=16, prep_blocks=1, g_gen_x=1, g_gen_y=2, g_frest_x=1, g_frest_y=2, const_blocks=1, g_fast_x=0, g_f8_x=0,
                 g_d8_0_x=0, g_d8_1_x=0, g_d8_2_x=0, g_d8_3_x=0)
    check(host, FOLD_COEFFS, 2048, st, MIN1, **defer)
    check(host, FOLD_COEFFS, 2048, st, dict(r1_min_pow=512), **defer)
    check(host, FOLD_COEFFS, 2048, dict(st, r1_prev_pow=2048), MIN1, **dict(defer, ident=1))
    check(host, FOLD_COEFFS, 2048, dict(st, r1_nq=200), MIN1, **dict(defer, points_blocks=2))            # ceil(2 * 200 / 256)
    check(host, FOLD_COEFFS, 2048, dict(st, d8_2S=5, d8_2K=7, d8_0K=300), MIN1, **dict(defer, g_d8_2_x=1, g_d8_2_y=5, const_blocks=2))
    # not deferred: the fast rows (1, 14) and the general ones (1, 2)
    plain = dict(ZERO, route=FC_STRUCT, flush=0, hn=16, prep_blocks=1, g_fast_x=1, g_fast_y=14, g_gen_x=1, g_gen_y=2, g_frest_x=0)
    check(host, FOLD_COEFFS, 2048, st, dict(r1_min_pow=513), **plain)                                   # the round after next would be dense
    check(host, FOLD_COEFFS, 2048, st, dict(r1_min_pow=1, defer=0), **plain)
    check(host, FOLD_COEFFS, 2048, dict(st, f8=0), MIN1, **plain)
    # r1_hi = r1_hi0 = 2 (a table with 4 rows): fused with hn = 1, but no third rank-one round to defer to
    check(host, FOLD_COEFFS, 2048, dict(st, r1_hi=2, r1_hi0=2, r1_lo=10), MIN1, route=FC_STRUCT, hn=1, g_fast_x=4, g_fast_y=14)
    check(host, FOLD_COEFFS, 2048, dict(st, r1_hi=3, r1_hi0=3, r1_lo=9), MIN1, route=FC_DEFER, hn=2)
    for other in (dict(st_ok=0), dict(fresh=0), dict(r1_hi=5)):
        check(host, FOLD_COEFFS, 2048, dict(st, **other), MIN1, route=FC_R1)
    check(host, FOLD_COEFFS, 2048, st, dict(r1_min_pow=1, structured=0), route=FC_R1)
    check(host, FOLD_COEFFS, 2048, st, dict(r1_min_pow=1025), route=FC_LAST_R1)
    # the call after a deferred fold: tables of 2048 live entries, r1_hi = 5, defer_pow = 1024, defer_hq = 16.  Its second fold if it is fold_coeffs(1024)
    # and that is fused (512 >= MIN_POW): hn = 8, f8 (1, 6), the others through the general kernel on g8's grid (1, 2), r2_kprep on 1 block
    after = dict(st, valid_t=2048, valid_e=2048, r1_hi=5, fresh=0, defer_on=1, defer_pow=1024, defer_hq=16)
    second = dict(ZERO, route=FC_SECOND, flush=0, hn=8, hq=16, prep_blocks=1, g_f8_x=1, g_f8_y=6, g_gen_x=1, g_gen_y=2)
    check(host, FOLD_COEFFS, 1024, after, MIN1, **second)
    check(host, FOLD_COEFFS, 1024, after, dict(r1_min_pow=512), **second)
    check(host, FOLD_COEFFS, 1024, dict(after, r1_prev_pow=1024), MIN1, **dict(second, ident=1))
    check(host, FOLD_COEFFS, 1024, dict(after, g8=0), MIN1, **dict(second, g_gen_y=1))                   # an empty list's grid is (gx, 1); nothing is launched on it
    # ... and anything else writes the deferred rows out first: the gate moved, another pow, the unfused calls
    check(host, FOLD_COEFFS, 1024, after, dict(r1_min_pow=513), flush=1, route=FC_LAST_R1)
    check(host, FOLD_COEFFS, 1024, after, dict(r1_min_pow=1025), flush=1, route=FC_SPLIT)
    check(host, FOLD_COEFFS, 512, after, MIN1, flush=1, route=FC_SPLIT, materialize=1)
    check(host, FOLD_COEFFS, 1024, dict(after, defer_pow=512), MIN1, flush=1, route=FC_R1)
    check(host, FOLD_COEFFS, 1024, dict(after, defer_on=0), MIN1, flush=0, route=FC_R1, hn=8, grid_y=8)
    check(host, COEFFS, 1024, after, MIN1, flush=1, route=SUMS_R1)
    check(host, FOLD, 1024, after, MIN1, flush=1, route=FOLD_R1)


def test_dense_fused_rounds_split_and_one_launch(host):
    # 2^17 entries given dense (nblocks = min(2048, 2^17 / 512) = 256).  pow = 32768: 16384 pairs = SPLIT_MAX -> split kernel, min(64, 256) workgroups.
    st = state(ell=17, r1=0)
    check(host, FOLD_COEFFS, 32768, st, **dict(ZERO, route=FC_SPLIT, flush=0, hn=0, blocks=64, one_launch=1))
    # 16385 pairs (pow = 32770: pow need be no power of two) -> k_sc_fold_coeffs on min(256, ceil(16385 / 256) = 65, max(256, 9)) = 65 blocks: above
    # ONE_LAUNCH_MAX = 64 -> a second kernel finishes the sums
    check(host, FOLD_COEFFS, 32770, st, **dict(ZERO, route=FC_DENSE, flush=0, hn=0, blocks=65, one_launch=0))
    check(host, FOLD_COEFFS, 32770, st, dict(one_launch_max=65), route=FC_DENSE, blocks=65, one_launch=1)
    # 64 blocks exactly (split off): one launch
    check(host, FOLD_COEFFS, 32768, st, dict(split_max=0), route=FC_DENSE, blocks=64, one_launch=1)
    check(host, FOLD_COEFFS, 32768, st, dict(split_max=16383), route=FC_DENSE, blocks=64)
    check(host, FOLD_COEFFS, 32768, st, dict(one_launch=0), route=FC_DENSE, blocks=64, one_launch=0)    # the split form is a one-launch form
    check(host, FOLD_COEFFS, 32768, st, dict(split_blocks=3), route=FC_SPLIT, blocks=3)
    check(host, FOLD_COEFFS, 2, st, route=FC_SPLIT, blocks=1)
    check(host, COEFFS, 16384, st, route=SUMS_DENSE, blocks=64, one_launch=1)
    check(host, COEFFS, 16385, st, route=SUMS_DENSE, blocks=65, one_launch=0)
    # long threads: 2^20 pairs of a 2^21 table (nblocks 2048): ceil / 256 = 4096, max(256, 2^20 / 2048 = 512) = 512 blocks; one pair each with ITEMS = 1
    # (4096, capped by nblocks); FLOOR = 1024 lifts the 512; BLOCKS = 300 caps them all
    big = state(ell=21, r1=0)
    check(host, COEFFS, 1 << 20, big, blocks=512, one_launch=0)
    check(host, COEFFS, 1 << 20, big, dict(items=1), blocks=2048)
    check(host, COEFFS, 1 << 20, big, dict(floor_blocks=1024), blocks=1024)
    check(host, COEFFS, 1 << 20, dict(big, nblocks=300), blocks=300)
    assert grid_fn(host, "nblocks", 1 << 21, 2048) == 2048 and grid_fn(host, "nblocks", 1 << 21, 300) == 300 and grid_fn(host, "nblocks", 2, 2048) == 1
    assert grid_fn(host, "nblocks", 1 << 28, 8192) == 8192 and grid_fn(host, "nblocks", 4096, 2048) == 8


def test_live_entries_error(host):
    # a round needs 2 pow live entries in both tables; coeffs and fold have written a deferred fold out by then, fold_coeffs has not
    for call in (COEFFS, FOLD, FOLD_COEFFS):
        for st in (state(valid_t=2048), state(valid_e=2048)):
            assert plan(host, call, 2048, st, **MIN1)[0] == 1
            assert plan(host, call, 1024, st, **MIN1)[0] == 0
        rs, p = plan(host, call, 2048, state(valid_t=2048, defer_on=1), **MIN1)
        assert rs == 1 and p["flush"] == (0 if call == FOLD_COEFFS else 1)
        assert all(v == 0 for k, v in p.items() if k != "flush")                  # zero-filled, whatever the caller's memory held


def test_table_predicates_and_the_other_grids(host):
    # which table gets a row structure: RANK1 and STRUCT on, at least 4 rows (hi >= 2), the first round rank-one.  4096: lo = hi = 6 -> 64 rows
    assert grid_fn(host, "struct_rows", 4096, **MIN1) == (64, 6) and grid_fn(host, "struct_rows", 4096, r1_min_pow=2048) == (64, 6)
    assert grid_fn(host, "struct_rows", 4096, r1_min_pow=2049) == (0, 6) and grid_fn(host, "struct_rows", 4096) == (0, 6)
    assert grid_fn(host, "struct_rows", 4096, r1_min_pow=1, rank1=0)[0] == 0 and grid_fn(host, "struct_rows", 4096, r1_min_pow=1, structured=0)[0] == 0
    assert grid_fn(host, "struct_rows", 8192, **MIN1) == (128, 6)                                       # odd ell: the rows take the extra bit
    assert grid_fn(host, "struct_rows", 8, **MIN1) == (4, 1) and grid_fn(host, "struct_rows", 4, **MIN1) == (0, 1)
    assert grid_fn(host, "struct_rows", 1 << 22) == (2048, 11)
    # EQ starts rank-one: RANK1, at least one row bit, len / 2 >= MIN_POW
    assert grid_fn(host, "eq_rank1", 1 << 22) == 1 and grid_fn(host, "eq_rank1", 1 << 21) == 0 and grid_fn(host, "eq_rank1", 1 << 22, rank1=0) == 0
    assert grid_fn(host, "eq_rank1", 2, **MIN1) == 1 and grid_fn(host, "eq_rank1", 1, **MIN1) == 0
    assert grid_fn(host, "eq_rank1", 4096, r1_min_pow=2048) == 1 and grid_fn(host, "eq_rank1", 4096, r1_min_pow=2049) == 0
    # k_sc_set_parts: tiles = len / 128; sub = max(1, min(SET_SUB, tiles / 8192)); ceil(ceil(tiles / sub) / 4) blocks
    assert grid_fn(host, "set_parts", 1 << 26) == (16384, 8) and grid_fn(host, "set_parts", 4096) == (8, 1) and grid_fn(host, "set_parts", 1 << 21) == (2048, 2)
    assert grid_fn(host, "set_parts", 1 << 26, set_sub=1) == (1 << 17, 1) and grid_fn(host, "set_parts", 1 << 26, set_sub=64) == (2048, 64)
    assert grid_fn(host, "set_parts", 1) == (1, 1)
    # k_sc_r1_prep (a = 2 r1_hi + folded): r1_hi = 6 folded: 16 rows of the next sums -> 1 block, or the masses if they are more; unfolded: 32 rows, no masses move
    assert grid_fn(host, "r1_prep_blocks", 13, 0) == 1 and grid_fn(host, "r1_prep_blocks", 13, 1000) == 4 and grid_fn(host, "r1_prep_blocks", 12, 1000) == 1
    assert grid_fn(host, "r1_prep_blocks", 28, 0) == 32 and grid_fn(host, "r1_prep_blocks", 29, 0) == 16 and grid_fn(host, "r1_prep_blocks", 1, 0) == 1
    assert grid_fn(host, "fold_blocks", 1) == 1 and grid_fn(host, "fold_blocks", 257) == 2 and grid_fn(host, "fold_blocks", 1 << 20) == 4096
    assert grid_fn(host, "fold_blocks", (1 << 20) + 1) == 4096 and grid_fn(host, "fold_blocks", 1 << 28) == 4096
    assert grid_fn(host, "split_blocks", 1) == 1 and grid_fn(host, "split_blocks", 65) == 2 and grid_fn(host, "split_blocks", 1 << 14) == 64
    # list grids at 2^28: gx = 64, 16 row groups until a thread would take more than 256 rows: n = 4097 -> 17
    assert grid_fn(host, "list_grid", 14, 8192) == (64, 32) and grid_fn(host, "list_grid", 14, 4096) == (64, 16) and grid_fn(host, "list_grid", 14, 4097) == (64, 17)
    assert grid_fn(host, "list_grid", 14, 5) == (64, 5) and grid_fn(host, "list_grid", 14, 0) == (64, 1) and grid_fn(host, "list_grid", 3, 2000) == (1, 1024)
    assert grid_fn(host, "r1_grid", 14, 8192) == (64, 16, 512) and grid_fn(host, "r1_grid", 14, 1) == (64, 1, 1) and grid_fn(host, "r1_grid", 9, 5000) == (2, 500, 10)


# ---------------------------------------------------------------------------------------------- the switches from their text
def parse(host, **text):
    assert set(text) <= set(SWITCHES)
    arr = (ctypes.c_char_p * len(SWITCHES))(*[None if text.get(k) is None else text[k].encode() for k in SWITCHES])
    out = (ctypes.c_uint64 * len(SWITCHES))()
    host.sc_plan_switches(arr, out)
    return dict(zip(SWITCHES, (int(v) for v in out)))


def test_switch_parsing(host):
    assert parse(host) == SWITCHES                                                                    # every variable unset
    assert parse(host, **{k: "" for k in SWITCHES}) == SWITCHES                                       # set but empty: the default, for the on/off ones too
    for k in ("one_launch", "rank1", "structured", "identity", "defer"):                             # off is a leading '0'
        assert parse(host, **{k: "0"})[k] == 0 and parse(host, **{k: "00"})[k] == 0 and parse(host, **{k: "0x"})[k] == 0
        assert parse(host, **{k: "1"})[k] == 1 and parse(host, **{k: "off"})[k] == 1 and parse(host, **{k: " 0"})[k] == 1
        assert parse(host, **{k: "0"}) == dict(SWITCHES, **{k: 0})
    clamps = dict(floor_blocks=(1, 8192), one_launch_max=(1, 8192), split_blocks=(1, 1024), items=(1, 64), order=(0, 2), set_sub=(1, 64), blocks_cap=(1, 8192))
    for k, (lo, hi) in clamps.items():
        got = [parse(host, **{k: str(v)})[k] for v in (lo - 1, lo, hi, hi + 1, -5, 10 ** 12)]
        assert got == [lo, lo, hi, hi, lo, hi], (k, got)
        assert parse(host, **{k: "x"})[k] == lo                                                       # no number reads as 0, clamped like one
    assert [parse(host, r1_min_pow=v)["r1_min_pow"] for v in ("0", "-3", "1", "4097", str(1 << 40))] == [1, 1, 1, 4097, 1 << 40]
    assert [parse(host, split_max=v)["split_max"] for v in ("-1", "0", "1", "65536", str(1 << 40))] == [0, 0, 1, 65536, 1 << 40]
    assert parse(host, r1_min_pow="1", split_max="0", items="3") == dict(SWITCHES, r1_min_pow=1, split_max=0, items=3)


# ---------------------------------------------------------------------------------------------- the row lists
def row_lists(host, flags):
    """None: no structure; else ({list: rows}, the concatenated array)"""
    H = len(flags)
    fl = (ctypes.c_uint32 * H)(*flags)
    offn = (ctypes.c_uint32 * (2 * len(LISTS)))()
    cap = 20 * H + 1
    words = (ctypes.c_uint32 * cap)()
    n = host.sc_plan_row_lists(fl, H, offn, words, cap)
    assert n >= 0
    if n == 0:
        return None
    words = [int(w) for w in words[:n]]
    return {k: (int(offn[2 * i]), int(offn[2 * i + 1])) for i, k in enumerate(LISTS)}, words


def lists_by_definition(flags):
    """sumcheck_kernels.inc, "a pristine table with structure", transcribed: row classes K (flag bit 1), S (bit 0 alone), W; every list ascending."""
    H = len(flags)
    cls = [2 if f & 2 else 1 if f & 1 else 0 for f in flags]
    if 2 * sum(c != 0 for c in cls) < H:
        return None
    hn, hq = H // 2, H // 4
    h8 = hq // 2

    def fast(h):
        return all(cls[h + b * hq] for b in range(4))

    def fast8(g):
        return h8 > 0 and fast(g) and fast(g + h8)

    out = {}
    for side in (0, 1):
        for k, name in enumerate("WSK"):
            out[f"sum{side}{name}"] = [h for h in range(hn) if cls[h + side * hn] == k]
    out["fast"] = [h for h in range(hq) if fast(h)]
    out["gen"] = [h for h in range(hq) if not fast(h)]
    out["f8"] = [g for g in range(h8) if fast8(g)]
    out["f8x"] = [h for h in range(hq) if h8 and fast8(h % h8)]
    out["frest"] = [h for h in out["fast"] if h not in out["f8x"]]
    out["g8"] = [g for g in range(h8) if not fast8(g)]
    for b in range(4):
        out[f"d8_{b}S"] = [h for h in out["f8x"] if cls[h + b * hq] == 1]
        out[f"d8_{b}K"] = [h for h in out["f8x"] if cls[h + b * hq] == 2]
    return out


def flag_vectors():
    K, S, W = 3, 1, 0                   # k_sc_classify leaves 3 on a constant row (constant and small), 1 on a small one
    rng = random.Random(0x5C)
    out = []
    for H in (4, 8, 16, 64):
        out += [[K] * H, [S] * H, [W] * H, [2] * H]
        out.append([W] * (H // 2) + [K] * (H // 2))                     # exactly half plain: structure
        out.append([W] * (H // 2 + 1) + [S] * (H // 2 - 1))             # one fewer: none
        out.append([K, W] * (H // 2))
        for q in range(4):                                              # one W row in each quarter
            v = [K if i % 3 else S for i in range(H)]
            v[q * (H // 4) + (H // 4) // 2] = W
            out.append(v)
        for e in range(8 if H >= 8 else 0):                             # ... and in each eighth
            v = [K] * H
            v[e * (H // 8)] = W
            out.append(v)
        for _ in range(40):
            p_w = rng.choice((0.02, 0.1, 0.3, 0.5))
            out.append([W if rng.random() < p_w else rng.choice((K, S, 2)) for _ in range(H)])
    return out


def test_row_lists_match_their_definitions(host):
    kept = dropped = 0
    for flags in flag_vectors():
        H = len(flags)
        want = lists_by_definition(flags)
        got = row_lists(host, flags)
        assert (got is None) == (want is None), flags
        if got is None:
            dropped += 1
            continue
        kept += 1
        offn, words = got
        # the lists lie end to end in this order -- the kernels index the one array -- and one spare word follows them
        at = 0
        for k in LISTS:
            off, n = offn[k]
            assert off == at and words[off:off + n] == want[k], (k, flags)
            at += n
        assert len(words) == at + 1 and words[-1] == 0
        hn, hq, h8 = H // 2, H // 4, H // 8
        part = lambda *names: sorted(sum((want[n] for n in names), []))                      # noqa: E731
        assert part("fast", "gen") == part("f8x", "frest", "gen") == list(range(hq)) and part("f8", "g8") == list(range(h8))
        for side in (0, 1):
            assert part(f"sum{side}W", f"sum{side}S", f"sum{side}K") == list(range(hn))
        for b in range(4):
            assert part(f"d8_{b}S", f"d8_{b}K") == want["f8x"]                               # a fast row has no W source
        assert len(want["f8x"]) == 2 * len(want["f8"])
        if H == 4:                                                                         # h8 = 0: nothing can be deferred
            assert all(not want[k] for k in LISTS if "8" in k) and want["frest"] == want["fast"]
    assert kept > 100 and dropped >= 8, (kept, dropped)
    assert row_lists(host, [3, 3, 0, 0]) is not None and row_lists(host, [3, 0, 0, 0]) is None


# ---------------------------------------------------------------------------------------------- whole steps
_LISTS_OF = {}


def step_start(host, ell, nq, flags, sw):
    """The state gen_eq_table and a set table leave (either order), with the row lists of `flags` (None: a table without structure)."""
    n = 1 << ell
    s = dict(SWITCHES, **sw)
    lo = ell // 2
    st = dict(len=n, valid_t=n, valid_e=n, nblocks=grid_fn(host, "nblocks", n, s["blocks_cap"]), r1=grid_fn(host, "eq_rank1", n, **sw), r1_hi=0, r1_hi0=0, r1_lo=0,
              r1_nq=0, r1_prev_pow=0, fresh=1, st_ok=0, defer_on=0, defer_pow=0, defer_hq=0)
    st.update({k: 0 for k in LISTS})
    if st["r1"]:
        st.update(r1_lo=lo, r1_hi=ell - lo, r1_hi0=ell - lo, r1_nq=nq)
    H, lo_bits = grid_fn(host, "struct_rows", n, **sw)
    assert lo_bits == lo
    if H and flags is not None:
        assert H == 1 << (ell - lo)
        if (flags, H) not in _LISTS_OF:
            got = row_lists(host, flags(H))
            _LISTS_OF[flags, H] = got and {k: v[1] for k, v in got[0].items()}
        if _LISTS_OF[flags, H]:
            st.update(st_ok=1, **_LISTS_OF[flags, H])
    return st


def apply(st, call, pow_, p):
    """The state changes of the three entry points, in their words (sumcheck_engine.inc)."""
    hi_before = st["r1_hi"]
    if call != COEFFS:
        st["r1_prev_pow"] = 0
    if p["flush"]:
        st["defer_on"] = 0
    r = p["route"]
    if r in (SUMS_STRUCT, SUMS_R1):
        st["r1_prev_pow"] = pow_
    elif r == SUMS_DENSE:
        st["r1_prev_pow"] = 0
    if r in (FOLD_R1, FC_R1, FC_STRUCT, FC_DEFER, FC_SECOND, FC_LAST_R1):                       # sc_r1_prep with a challenge
        assert hi_before >= 1, "r1_hi underflows"
        st["r1_hi"] -= 1
    if r == FC_DEFER:
        st.update(defer_on=1, defer_pow=pow_ // 2, defer_hq=p["hn"])
    if r == FC_SECOND:
        st["defer_on"] = 0
    if r in (FC_R1, FC_STRUCT, FC_DEFER, FC_SECOND):
        st["r1_prev_pow"] = pow_ // 2
    if p["materialize"]:
        assert st["r1"]
        st["r1"] = 0
    if call != COEFFS:
        st.update(fresh=0, valid_t=pow_, valid_e=pow_)


def rank_one_blocks(st, p):
    """Workgroups that add their limb sums to r1acc in this route (0: not a rank-one sums route)."""
    g = lambda name, n=1: p[f"g_{name}_x"] * p[f"g_{name}_y"] if n else 0                       # noqa: E731
    r = p["route"]
    if r == SUMS_STRUCT:
        return sum(g(f"sum{s}{c}", st[f"sum{s}{c}"]) for s in (0, 1) for c in "WS") + 2 * p["const_blocks"]
    if r in (SUMS_R1, FC_R1):
        return p["grid_x"] * p["grid_y"]
    if r == FC_STRUCT:
        return g("fast", st["fast"]) + g("gen", st["gen"])
    if r == FC_DEFER:
        return sum(g(f"d8_{b}", st[f"d8_{b}S"]) for b in range(4)) + 4 * p["const_blocks"] + g("frest", st["frest"]) + g("gen", st["gen"])
    if r == FC_SECOND:
        return g("f8") + g("gen", st["g8"])
    return 0


def check_plan(st, call, pow_, p):
    r = p["route"]
    gx = ceil_div(1 << st["r1_lo"], 256)
    # a deferred fold is consumed by the very next call, a fold_coeffs at defer_pow, or written out before that call touches the table
    if st["defer_on"]:
        assert p["flush"] or (r == FC_SECOND and call == FOLD_COEFFS and pow_ == st["defer_pow"]), (ROUTE_NAMES[r], st)
    else:
        assert not p["flush"] and r != FC_SECOND
    if r in (SUMS_STRUCT, SUMS_R1):
        assert st["r1_hi"] >= 1 and p["hn"] == 1 << (st["r1_hi"] - 1) and 2 * p["hn"] * (1 << st["r1_lo"]) == 2 * pow_
    if r in (FC_R1, FC_STRUCT, FC_DEFER, FC_SECOND):
        assert st["r1_hi"] >= 2 and p["hn"] == 1 << (st["r1_hi"] - 2) and p["prep_blocks"] == ceil_div(p["hn"], 256) >= 1
    if r == FC_DEFER:
        assert st["r1_hi"] >= 3 and st["f8"] > 0 and 8 * p["hn"] == 2 * (1 << st["r1_hi0"])
    if r == FC_SECOND:
        assert p["hq"] == st["defer_hq"] == 2 * p["hn"]
    if r in (SUMS_R1, FC_R1):                                  # sc_r1_grid: every row in exactly one chunk, at most 1024 blocks
        assert p["grid_x"] == gx and 1 <= p["grid_y"] and p["grid_x"] * p["grid_y"] <= max(1024, gx)
        assert (p["grid_y"] - 1) * p["rows_per_chunk"] < p["hn"] <= p["grid_y"] * p["rows_per_chunk"]
    for name, n in (("sum0W", st["sum0W"]), ("sum0S", st["sum0S"]), ("sum1W", st["sum1W"]), ("sum1S", st["sum1S"]), ("fast", st["fast"]), ("gen", None),
                    ("frest", st["frest"]), ("d8_0", st["d8_0S"]), ("d8_1", st["d8_1S"]), ("d8_2", st["d8_2S"]), ("d8_3", st["d8_3S"]), ("f8", st["f8"])):
        x, y = p[f"g_{name}_x"], p[f"g_{name}_y"]
        if x == 0:
            assert y == 0
            continue
        if n is None:
            n = st["g8"] if r == FC_SECOND else st["gen"]
        # sc_list_grid: at most 2048 blocks, at most 256 rows per thread (a thread walks rows y, y + gridDim.y, ..)
        assert x == gx and 1 <= y <= max(1, n) and x * y <= 2048 and ceil_div(n, y) <= 256, (name, n, x, y)
    if r in (SUMS_DENSE, FC_DENSE, FC_LAST_R1):
        assert 1 <= p["blocks"] <= st["nblocks"]
    if r == FC_SPLIT:
        assert 1 <= p["blocks"] <= 1024 and p["one_launch"] == 1
    if r in (FOLD_R1, FOLD_DENSE, FC_LAST_R1):
        assert 1 <= p["fold_blocks"] <= 4096
    # the limb sums k_sc_r1_final adds up are those of one reduced element per thread and slot, and of the masses: fe_from_limb_sums takes fewer than 2^28
    blocks = rank_one_blocks(st, p)
    if r in (SUMS_STRUCT, SUMS_R1, FC_R1, FC_STRUCT, FC_DEFER, FC_SECOND):
        assert 1 <= blocks and 256 * blocks + 2 * st["r1_nq"] < 1 << 28
        assert st["r1"] and not p["materialize"]


def step_calls(ell, fused, interrupt=None):
    """The calls of one step.  interrupt = (i, kind): the fused call i gets a round_coeffs of its own first (COEFFS), or is made as the unfused pair (FOLD)."""
    n = 1 << ell
    if fused:
        calls = [(COEFFS, n // 2)] + [(FOLD_COEFFS, n >> i) for i in range(1, ell)] + [(FOLD, 1)]
    else:
        calls = [c for i in range(1, ell + 1) for c in ((COEFFS, n >> i), (FOLD, n >> i))]
    if interrupt:
        i, kind = interrupt
        call, pow_ = calls[i]
        assert call == FOLD_COEFFS
        calls[i:i + 1] = [(COEFFS, pow_), (FOLD_COEFFS, pow_)] if kind == COEFFS else [(FOLD, pow_), (COEFFS, pow_ // 2)]
    return calls


def walk(host, ell, sw, nq=0, flags=None, fused=True, interrupt=None):
    """One step, round by round: plan, check, apply.  Returns the routes."""
    st = step_start(host, ell, nq, flags, sw)
    routes = []
    for call, pow_ in step_calls(ell, fused, interrupt):
        rs, p = plan(host, call, pow_, st, **sw)
        assert rs == 0, (call, pow_, st)
        check_plan(st, call, pow_, p)
        apply(st, call, pow_, p)
        routes.append(p["route"])
    assert st["valid_t"] == st["valid_e"] == 1 and not st["defer_on"] and not st["fresh"]
    return routes


def mostly_constant(H):                                         # a document table: S rows, the rest constant, and from 16 rows on a W row in the second eighth (g8 is not empty)
    return [0 if h == 1 and H >= 16 else 1 if h % 5 == 2 else 3 for h in range(H)]


def scattered(H):
    rng = random.Random(H)
    return [0 if rng.random() < 0.2 else rng.choice((1, 3)) for _ in range(H)]


def test_whole_steps_keep_their_invariants(host):
    seen = set()
    for ell in range(2, 29):
        n = 1 << ell
        gates = sorted({1, 4, n // 8 or 1, n // 4 or 1, n // 2, n, 1 << 21})
        for gate in gates:
            for flags in (None, mostly_constant, scattered):
                for extra in ({}, dict(defer=0), dict(identity=0, one_launch=0), dict(structured=0, split_max=0, items=1), dict(rank1=0)):
                    sw = dict(r1_min_pow=gate, **extra)
                    for fused in (True, False):
                        seen |= set(walk(host, ell, sw, nq=(ell * 37) % 300, flags=flags, fused=fused))
    assert seen == set(range(12)), sorted(ROUTE_NAMES[r] for r in set(range(12)) - seen)


def test_a_deferred_fold_is_consumed_or_flushed(host):
    """The call after a deferred fold, in every form: its second fold, the sums alone, the fold alone, and each of them with the gate between the two."""
    for ell in (6, 7, 8, 12, 13, 24, 28):                       # with the shipped gate the third rank-one round exists from 2^24 entries on
        sw = dict(r1_min_pow=1) if ell < 24 else {}
        base = walk(host, ell, sw, flags=mostly_constant)
        assert base[:3] == [SUMS_STRUCT, FC_DEFER, FC_SECOND], [ROUTE_NAMES[r] for r in base]
        # round_coeffs between the two folds: the rows are written out, the next fused call is an ordinary rank-one one
        r = walk(host, ell, sw, flags=mostly_constant, interrupt=(2, COEFFS))
        assert r[:4] == [SUMS_STRUCT, FC_DEFER, SUMS_R1, FC_R1] and FC_SECOND not in r
        # the unfused fold arrives while the fold is deferred
        r = walk(host, ell, sw, flags=mostly_constant, interrupt=(2, FOLD))
        assert r[:3] == [SUMS_STRUCT, FC_DEFER, FOLD_R1] and FC_SECOND not in r
    # ell = 6: lo = hi = 3, eight rows: r1_hi = 3 is the least that defers; ell = 5 (hi = 3) defers too, ell = 4 (hi = 2) cannot
    assert walk(host, 5, dict(r1_min_pow=1), flags=lambda H: [3] * H)[:3] == [SUMS_STRUCT, FC_DEFER, FC_SECOND]
    assert walk(host, 4, dict(r1_min_pow=1), flags=lambda H: [3] * H)[:3] == [SUMS_STRUCT, FC_STRUCT, FC_LAST_R1]


# ---------------------------------------------------------------------------------------------- under the sanitizers
def sanitizer_cases(host):
    """(line for the program, what the library says)"""
    out = []
    rng = random.Random(7)
    for ell in (2, 3, 6, 7, 12, 13, 21, 22, 28):
        for gate in (1, (1 << ell) // 4 or 1, 1 << 21):
            sw = dict(r1_min_pow=gate, split_blocks=rng.choice((1, 3, 64)), items=rng.choice((1, 8)))
            st = step_start(host, ell, 5, mostly_constant, sw)
            n = 1 << ell
            for call, pow_ in [(COEFFS, n // 2)] + [(FOLD_COEFFS, n >> i) for i in range(1, ell)] + [(FOLD, 1), (COEFFS, n)]:
                rs, p = plan(host, call, pow_, st, **sw)
                out.append(("plan " + " ".join(str(v) for v in plan_inputs(call, pow_, st, sw)), [rs] + [p[k] for k in host.out_names]))
                if rs == 0:
                    apply(st, call, pow_, p)
    for flags in flag_vectors():
        got = row_lists(host, flags)
        want = [0] if got is None else [len(got[1])] + [v for k in LISTS for v in got[0][k]] + got[1]
        out.append((f"lists {len(flags)} " + " ".join(str(f) for f in flags), want))
    for text in ({}, {k: "" for k in SWITCHES}, {k: "0" for k in SWITCHES}, {k: "999999999999" for k in SWITCHES}, {k: "-7" for k in SWITCHES},
                 dict(r1_min_pow="1", order="1")):
        words = " ".join("-" if text.get(k) is None else text[k] or '""' for k in SWITCHES)
        out.append(("switch " + words, [0] + list(parse(host, **text).values())))
    return out


def test_everything_under_the_sanitizers(host, tmp_path):
    """The same functions as a stand-alone program built with -fsanitize=address,undefined: plans of whole steps, row lists, switches -- the same numbers."""
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DSC_PLAN_CHECK_MAIN", SRC, "-o", EXE])
    cases = sanitizer_cases(host)
    path = tmp_path / "cases.txt"
    path.write_text("".join(line + "\n" for line, _ in cases))
    r = subprocess.run([EXE, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases) > 300
    for (line, want), got in zip(cases, lines):
        assert [int(v) for v in got.split()] == want, line[:200]
