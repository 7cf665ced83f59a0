"""The launch plan of the bucket pipeline (reef_amd/csrc/msm_plan.h: core_launch_plan -- what engine.inc's run_core launches, decided in one
pure function) on the host, compiled with g++ (csrc/tools/plan_check.cpp).  Runs without a GPU.  Three checks: plans derived BY HAND from the
text of run_core as it stood before the plan was split off (one on each side of every branch; the derivations are in the comments), invariants
over a grid of shapes, and the three argument errors at their exact bounds.  The grid also goes once through the same function built as a
program of its own with -fsanitize=address,undefined."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "reef_amd", "csrc")
LIBDIR = os.path.join(ROOT, "reef_amd", "_lib")
SO = os.path.join(LIBDIR, "libreef_plancheck.so")
EXE = os.path.join(LIBDIR, "plan_check_san")
SRC = os.path.join(CSRC, "tools", "plan_check.cpp")
DEPS = [SRC, os.path.join(CSRC, "msm_plan.h")]
SMALL, WAVE, TILES = 0, 1, 2                    # msm_plan.h: ScanRoute
NONE, COOP, PLAIN = 0, 1, 2                     # msm_plan.h: MergeFirst
SWITCHES = dict(fuse_merge=1, merge1=1, fuse_max_chunks=65536, fuse_recode=1, sort_compact=1, sort_word=1, skip_reduce=0)   # every variable unset


def _stale(path):
    return not os.path.exists(path) or os.path.getmtime(path) < max(os.path.getmtime(d) for d in DEPS)


@pytest.fixture(scope="module")
def host():
    if _stale(SO):
        os.makedirs(LIBDIR, exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", SRC, "-o", SO])
    lib = ctypes.CDLL(SO)
    lib.plan_core.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_char_p)]
    lib.plan_out_names.restype = ctypes.c_char_p
    lib.plan_same.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.plan_constants.argtypes = [ctypes.c_void_p]
    lib.names = lib.plan_out_names().decode().split()
    assert lib.plan_in_count() == 19
    return lib


def windows_for(c):
    return (256 + c - 1) // c


def case(c, G, n, *, W=None, rows=1, n_ctx=None, slice_sort=0, L0=0, coop=1, two_level=-1, lanes=0, group_sums_out=0, **sw):
    """The 19 inputs of one plan.  G as the plan sees it (1: a pre-shifted key); W defaults to the windows of a full-width scalar."""
    s = dict(SWITCHES, **sw)
    assert set(s) == set(SWITCHES)
    return [c, windows_for(c) if W is None else W, G, rows, n, n if n_ctx is None else n_ctx, slice_sort, L0, coop, two_level, lanes, group_sums_out,
            s["fuse_merge"], s["merge1"], s["fuse_max_chunks"], s["fuse_recode"], s["sort_compact"], s["sort_word"], s["skip_reduce"]]


def plan(host, inputs):
    """(status, {field: value}, error text)"""
    a = (ctypes.c_int64 * 19)(*inputs)
    out = (ctypes.c_uint64 * len(host.names))()
    why = ctypes.c_char_p()
    rs = host.plan_core(a, out, ctypes.byref(why))
    return rs, dict(zip(host.names, (int(v) for v in out))), (why.value or b"").decode()


def check(host, inputs, **want):
    rs, p, why = plan(host, inputs)
    assert rs == 0, why
    p["levels"] = [p[f"merge_len{i}"] for i in range(p["merge_nlevels"])]
    got = {k: p[k] for k in want}
    assert got == want, inputs
    return p


# ---------------------------------------------------------------------------------------------- plans derived by hand
# The rules, as run_core, merge_is_fused and launch_partial_merge stated them (NB = 2^(c-1), gt = rows * G, N = rows * row_len, Mmax = N * W):
#   L0 (ctx option 0)  Mmax <= 48 * 65536: max(4, ceil(Mmax / 65536)), else min(128, ceil(Mmax / 131072));  nchunks0 = ceil(Mmax / L0) rounded up to 64
#   row_mode           rows > 1 and not slice_sort
#   two_level          not row_mode, ctx.two_level != 0, NB >= 64 << 8 = 16384 (c >= 15), and (ctx.two_level > 0 or Mmax >= 2^20)
#   compact / shift    two_level and SORT_COMPACT: span = ceil(W / G) * n_ctx <= 2^23: compact, shift 8; <= 2^24: compact, shift 7; else 8-byte, shift 8
#   word_entries       compact and SORT_WORD
#   NBc = NB >> shift, NBTc = gt * NBc, KB = min(NBc, 32768), P = NBc / KB
#   S                  max(1, min(ceil(256 / (gt * P)), ceil(row_len / 1024))), per = ceil(row_len / S), then S = ceil(row_len / per)
#   recode_fused       FUSE_RECODE and gt == 1 and P == 1
#   scan               k_scan_small if not row_mode, NBTc <= 4096, NBTc % 4 == 0 and S <= 64; else the _w kernels if not row_mode and NBTc <= 4096;
#                      else k_slice_totals (not in row mode) / k_scan_tiles / k_scan_finish;  ntiles = ceil(NBTc / 4096)
#   nseg_max, fine     ceil(Mmax / 16384) + NBTc, 2^shift
#   waves = ceil(nchunks0 / 64);  fused: FUSE_MERGE, MERGE1, nchunks0 <= FUSE_MAX_CHUNKS (65536) and not (coop and waves <= 384)
#   first merge        none if fused or MERGE1 = 0; k_merge_chunks<coop> on `waves` workgroups if coop and waves <= 384; else <plain> on ceil(waves / 4)
#   later levels       none if waves <= 1; len = 2 * waves (MERGE1 = 0: 2 * nchunks0, from list 0), then 2 * ceil(len / 64) until a level had len <= 64
#   c2 = ceil((c - 1) / 2), c1 = c - 1 - c2, rc_waves = gt * (2^c1 + 2^c2), direct = no group sums wanted and G == 1
def test_headline_plan_2pow20_points_on_a_preshifted_key(host):
    # c = 17: W = 16, NB = 65536.  Mmax = 2^24 > 48 * 65536 -> L0 = min(128, 2^24 / 2^17 = 128) = 128, nchunks0 = 2^24 / 128 = 131072.
    # NB >= 16384 and Mmax >= 2^20 -> two levels.  span = 16 * 2^20 = 2^24: above 2^23, within 2^24 -> compact with shift 7, one-word entries.
    # NBc = 65536 >> 7 = 512 = NBTc = KB, P = 1.  S = min(ceil(256 / 1), 1024) = 256, per = 4096, S = 256.  gt = 1 and P = 1 -> recode fused.
    # NBTc <= 4096 but S = 256 > 64 -> the _w kernels, one tile.  nseg_max = 2^24 / 16384 + 512 = 1536, fine = 128.
    # waves = 2048: nchunks0 > 65536 -> not fused; waves > 384 -> plain first merge on 2048 / 4 = 512 workgroups, writing 2 * 2048 = 4096 slots;
    # levels 4096 -> 2 * 64 = 128 -> 2 * 2 = 4 (<= 64: the last).  c - 1 = 16 -> c2 = c1 = 8, rc_waves = 256 + 256 = 512.
    p = check(host, case(17, 1, 1 << 20), L0=128, nchunks0=131072, entries_padded=1 << 24, row_mode=0, two_level=1, compact=1, shift=7, word_entries=1,
              NBc=512, NBTc=512, KB=512, P=1, S=256, per=4096, recode_fused=1, scan=WAVE, ntiles=1, nseg_max=1536, fine=128,
              merge_fused=0, merge_first=PLAIN, merge_first_grid=512, merge_cur=1, levels=[4096, 128, 4], c1=8, c2=8, rc_waves=512, direct=1, rowcol_lanes=0)
    assert p["b_dig"] == 4 << 24 and p["b_entries"] == p["b_entries1"] == 8 << 24 and p["b_seg_counts"] == 1536 * 128 * 4
    check(host, case(17, 1, 1 << 20, lanes=32), rowcol_lanes=32, rc_waves=512)          # the form of the row / column sums passes through


def test_one_level_sort_and_k_scan_small(host):
    # c = 13: W = 20, NB = 4096 < 16384 -> one level, shift 0, no entries1.  n = 4096: Mmax = 81920 -> L0 = max(4, 2) = 4, nchunks0 = 20480.
    # NBc = NBTc = KB = 4096, P = 1, S = min(256, 4) = 4, per = 1024.  NBTc <= 4096, a multiple of 4, S <= 64 -> k_scan_small.
    # waves = 320 <= 384 with coop -> not fused, the coop first merge on 320 workgroups; levels 640 -> 2 * 10 = 20.  c - 1 = 12 -> c1 = c2 = 6.
    p = check(host, case(13, 1, 4096), L0=4, nchunks0=20480, two_level=0, compact=0, word_entries=0, shift=0, NBc=4096, NBTc=4096, KB=4096, P=1, S=4, per=1024,
              recode_fused=1, scan=SMALL, ntiles=1, nseg_max=0, fine=0, merge_fused=0, merge_first=COOP, merge_first_grid=320, levels=[640, 20],
              c1=6, c2=6, rc_waves=128, direct=1)
    assert p["b_entries1"] == p["b_bstart1"] == p["b_seg_first"] == p["b_seg_counts"] == 0
    # the same without coop tails: nothing keeps the first level out of k_accum0 (20480 <= 65536)
    check(host, case(13, 1, 4096, coop=0, lanes=64), merge_fused=1, merge_first=NONE, merge_cur=1, levels=[640, 20], b_wsum=0)
    # ctx.two_level = 1 cannot force two levels on a window below c = 15; = 0 keeps one level at any size
    check(host, case(13, 1, 4096, two_level=1), two_level=0)
    check(host, case(17, 1, 1 << 20, two_level=0), two_level=0, shift=0, compact=0, word_entries=0, NBc=65536, KB=32768, P=2, recode_fused=0, scan=TILES, ntiles=16)
    # ... and = 1 takes them below 2^20 digits: c = 15 (W = 18, NB = 16384), 3000 points, Mmax = 54000
    check(host, case(15, 1, 3000, two_level=1), two_level=1, compact=1, shift=8, NBc=64, S=3, per=1000, scan=SMALL, nseg_max=4 + 64, fine=256)
    check(host, case(15, 1, 3000), two_level=0)


def test_two_level_entry_forms(host):
    # 8-byte entries: c = 17, n = n_ctx = 2^21: span = 16 * 2^21 = 2^25 > 2^24 -> not compact, shift 8.  Mmax = 2^25 -> L0 = min(128, 256) = 128,
    # nchunks0 = 2^18.  NBc = 256, S = min(256, 2048) = 256, per = 8192.  nseg_max = 2^25 / 2^14 + 256 = 2304, fine = 256.
    check(host, case(17, 1, 1 << 21), L0=128, nchunks0=1 << 18, two_level=1, compact=0, word_entries=0, shift=8, NBc=256, NBTc=256, KB=256, P=1, S=256, per=8192,
          scan=WAVE, nseg_max=2304, fine=256, recode_fused=1)
    # compact with shift 8: n = n_ctx = 2^19: span = 2^23 exactly.  Mmax = 2^23 -> L0 = min(128, 64) = 64, nchunks0 = 131072.  nseg_max = 512 + 256.
    check(host, case(17, 1, 1 << 19), L0=64, nchunks0=131072, two_level=1, compact=1, word_entries=1, shift=8, NBc=256, S=256, per=2048, nseg_max=768, fine=256)
    # one table point more and the index needs the 24th bit: shift 7 (a prefix MSM of 2^19 points on a key of 2^19 + 1)
    check(host, case(17, 1, 1 << 19, n_ctx=(1 << 19) + 1), compact=1, shift=7, NBc=512, nseg_max=512 + 512, fine=128)
    check(host, case(17, 1, 1 << 19, n_ctx=1 << 20), compact=1, shift=7)                # span = 2^24 exactly
    check(host, case(17, 1, 1 << 19, n_ctx=(1 << 20) + 1), compact=0, shift=8, word_entries=0)
    # a plain key: span counts the tables per group, ceil(W / G) = 4 -> 4 * 2^20 = 2^22 <= 2^23
    check(host, case(17, 4, 1 << 20), compact=1, shift=8, NBc=256, NBTc=1024, P=1, S=min(64, 1024), recode_fused=0, direct=0, rc_waves=4 * 512)
    # the smallest two-level shape of the GPU suite: 65536 points at c = 15 (W = 18, NB = 16384).  Mmax = 1179648 >= 2^20; span = 1179648 <= 2^23 ->
    # compact, shift 8, NBc = 64; S = min(256, 64) = 64, per = 1024 -> S <= 64 and NBTc = 64: k_scan_small.  L0 = max(4, 18) = 18, nchunks0 = 65536:
    # waves = 1024 > 384 and nchunks0 <= 65536 -> fused; levels 2048 -> 64.  nseg_max = 72 + 64.
    check(host, case(15, 1, 65536), L0=18, nchunks0=65536, two_level=1, compact=1, word_entries=1, shift=8, NBc=64, KB=64, S=64, per=1024, scan=SMALL,
          nseg_max=136, fine=256, merge_fused=1, merge_first=NONE, merge_cur=1, levels=[2048, 64], c1=7, c2=7, rc_waves=256)


def test_tiles_route(host):
    # more than 4096 keys: c = 14 (W = 19, NB = 8192), 3000 points.  Mmax = 57000 -> L0 = 4, nchunks0 = 14250 -> 14272.  S = min(256, 3) = 3, per = 1000.
    # NBTc = 8192 -> k_slice_totals / k_scan_tiles / k_scan_finish on 2 tiles.  waves = 223 -> coop first merge; levels 446 -> 14.  c - 1 = 13 -> c2 = 7, c1 = 6.
    check(host, case(14, 1, 3000), L0=4, nchunks0=14272, two_level=0, NBc=8192, NBTc=8192, KB=8192, P=1, S=3, per=1000, recode_fused=1, scan=TILES, ntiles=2,
          merge_first=COOP, merge_first_grid=223, levels=[446, 14], c1=6, c2=7, rc_waves=192)
    # two LDS parts per group and four groups: c = 17 with G = 4, 4096 points (Mmax = 65536 < 2^20: one level).  KB = 32768, P = 2,
    # S = min(ceil(256 / 8) = 32, 4) = 4.  NBTc = 4 * 65536 -> 64 tiles.  L0 = 4, nchunks0 = 16384, waves = 256.  Not direct: four group sums.
    check(host, case(17, 4, 4096), two_level=0, NBc=65536, NBTc=1 << 18, KB=32768, P=2, S=4, per=1024, recode_fused=0, scan=TILES, ntiles=64, L0=4, nchunks0=16384,
          merge_first=COOP, merge_first_grid=256, levels=[512, 16], c1=8, c2=8, rc_waves=2048, direct=0)
    # 4096 keys that are no multiple of 4 do not exist (NBTc = gt * 2^k), but 3 groups of 2 keys do: c = 2, G = 3 -> NBTc = 6 -> the _w kernels
    check(host, case(2, 3, 100), NBc=2, NBTc=6, KB=2, S=1, per=100, scan=WAVE, c1=0, c2=1, rc_waves=9)
    check(host, case(2, 4, 100), NBTc=8, scan=SMALL)


def test_row_mode_and_slice_sort(host):
    # rows sorted whole in LDS: 16 rows of 2048, c = 13 (W = 20).  N = 32768, Mmax = 655360 -> L0 = 10, nchunks0 = 65536.  gt = 16, NBT = 65536.
    # keys_per_row = 4096 -> rows_per_block = min(32768 / 4096 = 8, 65536 / 2048 = 32) = 8; counts hold one word per key.  Never two levels; the scan is
    # k_scan_tiles on NBT / 4096 = 16 tiles without slice totals.  waves = 1024 -> fused; levels 2048 -> 64.  rc_waves = 16 * 128.
    p = check(host, case(13, 1, 2048, rows=16), row_mode=1, two_level=0, N=32768, Mmax=655360, L0=10, nchunks0=65536, groups_total=16, NBT=65536, keys_per_row=4096,
              rows_per_block=8, KB=0, P=0, S=0, per=0, recode_fused=0, scan=TILES, ntiles=16, merge_fused=1, levels=[2048, 64], rc_waves=2048, direct=1)
    assert p["b_counts"] == 65536 * 4
    check(host, case(13, 1, 40000, rows=2), row_mode=1, rows_per_block=1)                 # long rows: 65536 / 40000 = 1
    check(host, case(15, 1, 2048, rows=2, two_level=1), row_mode=1, two_level=0, keys_per_row=16384, rows_per_block=2)     # never two levels in row mode
    # a batch of long rows through the sliced sort: 3 rows of 8209, c = 13.  N = 24627, Mmax = 492540 -> L0 = 8, nchunks0 = 61568 (= 962 * 64).
    # gt = 3: S = min(ceil(256 / 3) = 86, 9) = 9, per = ceil(8209 / 9) = 913, S = 9; the recode stays its own kernel.  NBTc = 12288 -> 3 tiles.
    # waves = 962 -> fused; levels 1924 -> 2 * 31 = 62.
    check(host, case(13, 1, 8209, rows=3, slice_sort=1), row_mode=0, two_level=0, N=24627, Mmax=492540, L0=8, nchunks0=61568, groups_total=3, NBT=12288, NBc=4096,
          NBTc=12288, KB=4096, P=1, S=9, per=913, recode_fused=0, scan=TILES, ntiles=3, merge_fused=1, merge_first=NONE, levels=[1924, 62], rc_waves=384, direct=1)
    # the L / R pair of an IPA round on the headline key: two groups of 512 coarse keys, S = min(128, 1024) = 128
    check(host, case(17, 1, 1 << 19, rows=2, slice_sort=1, n_ctx=1 << 20), row_mode=0, two_level=1, compact=1, shift=7, NBTc=1024, S=128, per=4096, recode_fused=0,
          scan=WAVE, nseg_max=1024 + 1024, rc_waves=1024)


def test_merge_thresholds(host):
    # ctx L0 = 20 with c = 13 (W = 20): nchunks0 = n rounded up to 64
    check(host, case(13, 1, 65536, L0=20), L0=20, nchunks0=65536, merge_fused=1, merge_first=NONE, levels=[2048, 64])
    check(host, case(13, 1, 65600, L0=20), nchunks0=65600, merge_fused=0, merge_first=PLAIN, merge_first_grid=257, levels=[2050, 66, 4])    # 1025 waves
    check(host, case(13, 1, 24576, L0=20), nchunks0=24576, merge_fused=0, merge_first=COOP, merge_first_grid=384, levels=[768, 24])         # 384 waves
    check(host, case(13, 1, 24640, L0=20), nchunks0=24640, merge_fused=1, merge_first=NONE, levels=[770, 26])                               # 385 waves
    check(host, case(13, 1, 24640, L0=20, fuse_merge=0), merge_fused=0, merge_first=PLAIN, merge_first_grid=97, levels=[770, 26])
    check(host, case(13, 1, 24576, L0=20, coop=0, lanes=64), merge_fused=1, merge_first=NONE)
    # one wave of chunks: the first level leaves two slots and nothing to merge; 65 chunks round up to two waves
    check(host, case(13, 1, 64, L0=20), nchunks0=64, merge_first=COOP, merge_first_grid=1, levels=[])
    check(host, case(13, 1, 65, L0=20), nchunks0=128, merge_first=COOP, merge_first_grid=2, levels=[4])


def test_chunk_length_at_48_entries(host):
    # W = 1 (a row of scalars that fit one window): Mmax = n.  48 * 65536 = 3145728 -> L0 = 48 on 65536 chunks; one more digit -> the long-chunk
    # rule: L0 = min(128, ceil(3145729 / 131072) = 25), nchunks0 = ceil(3145729 / 25) = 125830 -> 125888
    check(host, case(13, 1, 3145728, W=1), Mmax=3145728, L0=48, nchunks0=65536, merge_fused=1)
    check(host, case(13, 1, 3145729, W=1), Mmax=3145729, L0=25, nchunks0=125888, merge_fused=0, merge_first=PLAIN, merge_first_grid=492)
    check(host, case(17, 1, 196608), Mmax=3145728, L0=48, nchunks0=65536)                 # the same bound on a key: 16 * 196608
    check(host, case(13, 1, 1, W=1), L0=4, nchunks0=64, entries_padded=256)               # and the floor of 4


def test_each_switch_flipped_once(host):
    mid = dict(c=15, G=1, n=65536)                                                        # fused merge, k_scan_small, two levels (above)
    check(host, case(**mid, fuse_merge=0), merge_fused=0, merge_first=PLAIN, merge_first_grid=256, merge_cur=1, levels=[2048, 64])
    # MERGE1 = 0: no chunk-per-lane level; k_accumN starts on the chunks' own 2 * 65536 slots in list 0
    check(host, case(**mid, merge1=0), merge_fused=0, merge_first=NONE, merge_cur=0, levels=[131072, 4096, 128, 4])
    check(host, case(**mid, fuse_max_chunks=65535), merge_fused=0, merge_first=PLAIN)
    check(host, case(**mid, fuse_max_chunks=65536), merge_fused=1)
    check(host, case(17, 1, 1 << 20, fuse_max_chunks=1 << 17), merge_fused=1, merge_first=NONE, levels=[4096, 128, 4])
    check(host, case(17, 1, 1 << 20, fuse_recode=0), recode_fused=0, S=256)
    check(host, case(17, 1, 1 << 20, sort_compact=0), two_level=1, compact=0, word_entries=0, shift=8, NBc=256, nseg_max=1024 + 256, fine=256)
    check(host, case(17, 1, 1 << 20, sort_word=0), compact=1, shift=7, word_entries=0)
    full = check(host, case(17, 1, 1 << 20), skip_reduce=0)
    assert full["b_wsum"] == 4 * 144
    assert check(host, case(17, 1, 1 << 20, skip_reduce=1), skip_reduce=1)["b_wsum"] == 0
    assert check(host, case(17, 1, 1 << 20, skip_reduce=2), skip_reduce=2)["b_wsum"] == 4 * 144
    assert check(host, case(17, 4, 1 << 12, group_sums_out=1), direct=0)["b_group_sums"] == 4 * 144
    check(host, case(17, 1, 1 << 12, group_sums_out=1), direct=0)


def test_a_captured_chain_is_keyed_on_the_whole_plan(host):
    """run_core_graphed replays a captured chain only for an equal plan: equal inputs give equal bytes (whatever the output struct held before), and
    anything that changes a launch changes them."""
    base = case(17, 1, 1 << 20)

    def same(a, b):
        return host.plan_same((ctypes.c_int64 * 19)(*a), (ctypes.c_int64 * 19)(*b))
    assert same(base, list(base)) == 1
    for other in (case(17, 1, (1 << 20) - 1, n_ctx=1 << 20), case(17, 1, 1 << 20, lanes=32), case(17, 1, 1 << 20, coop=0, lanes=64), case(17, 1, 1 << 20, L0=64),
                  case(17, 1, 1 << 20, two_level=0), case(17, 1, 1 << 20, sort_word=0), case(17, 1, 1 << 20, skip_reduce=2)):
        assert same(base, other) == 0, other


# ---------------------------------------------------------------------------------------------- invariants over a grid
NS = [1, 63, 64, 65, 1023, 1 << 10, (1 << 12) - 1, (1 << 12) + 1, 61439, 61440, 180223, 180224, (1 << 17) + 12345, 1 << 20, 1 << 22]
OPTS = [(0, 0), (7, 0), (7, 1), (9, 3), (12, 1), (13, 0), (16, 0), (4, 2)]        # (window_bits, bucket_groups) of test_plans_vs_c_oracle; (0, g): shipped
ROW_SHAPES = [(64, 512), (3, 8192), (4096, 8192)]


def shipped_window(n, g_opt):
    """engine.inc: choose_window"""
    if g_opt == 1:
        return 13 if n < 61440 else 15 if n < 180224 else 17
    best, best_c = None, 4
    for c in range(3, 21):
        w = windows_for(c)
        g = w if g_opt == 0 else min(g_opt, w)
        cost = (255 // c + (0.5 if 255 % c == 0 else 1.0)) * n + (10.0 if g == 1 else 4.0) * g * (1 << (c - 1))
        if best is None or cost < best:
            best, best_c = cost, c
    return best_c


def grid():
    out = []
    for c_opt, g_opt in OPTS + [(0, 1)]:
        for n in NS:
            c = c_opt or shipped_window(n, g_opt)
            w = windows_for(c)
            g = w if g_opt == 0 else min(g_opt, w)
            for coop, lanes in ((1, 0), (0, 64)):
                out.append(case(c, g, n, coop=coop, lanes=lanes))
            out.append(case(c, g, n, two_level=1, group_sums_out=1))
            out.append(case(c, g, n, merge1=0, sort_word=0, fuse_recode=0))
            out.append(case(c, g, n, L0=7, sort_compact=0, fuse_merge=0, n_ctx=max(n, 1 << 20)))
            for rows, row_len in ROW_SHAPES:
                out.append(case(c, g, row_len, rows=rows, n_ctx=max(n, row_len)))
                out.append(case(c, g, row_len, rows=rows, n_ctx=max(n, row_len), slice_sort=1))
    return out


def ceil_div(a, b):
    return -(-a // b)


def invariants(inp, p):
    c, W, G, rows, row_len, n_ctx, slice_sort, L0, coop = inp[:9]
    merge1 = inp[13]
    gt, NB = rows * G, 1 << (c - 1)
    assert (p["N"], p["Mmax"], p["NB"], p["NBT"], p["groups_total"]) == (rows * row_len, rows * row_len * W, NB, gt * NB, gt)
    assert p["entries_padded"] == p["nchunks0"] * p["L0"] >= p["Mmax"] and p["nchunks0"] % 64 == 0 and p["L0"] >= 1
    assert p["entries_padded"] - p["Mmax"] < 64 * p["L0"]
    assert p["row_mode"] == (rows > 1 and not slice_sort)
    assert p["word_entries"] <= p["compact"] <= p["two_level"] <= 1
    assert p["c1"] + p["c2"] == c - 1 and 0 <= p["c2"] - p["c1"] <= 1 and p["rc_waves"] == gt * ((1 << p["c1"]) + (1 << p["c2"]))
    assert p["NBc"] << p["shift"] == NB and p["NBTc"] == gt * p["NBc"] and p["ntiles"] == ceil_div(p["NBTc"], 4096) <= 1024
    if p["compact"]:                                   # index, low key bits and sign share one word
        assert (ceil_div(W, G) * n_ctx - 1) << p["shift"] < 1 << 31
    if not p["row_mode"]:
        assert p["KB"] * p["P"] == p["NBc"] and p["KB"] <= 32768 and p["S"] * p["per"] >= row_len > (p["S"] - 1) * p["per"]
        assert p["recode_fused"] <= (gt == 1 and p["P"] == 1)
        counts_words = (p["S"] + 1) * p["NBTc"]        # k_count: S slices of NBTc cursors; the slice totals behind them
        if p["scan"] == SMALL:
            assert p["NBTc"] <= 4096 and p["NBTc"] % 4 == 0 and p["S"] <= 64
        elif p["scan"] == WAVE:
            assert p["NBTc"] <= 4096
    else:
        assert p["scan"] == TILES and not p["two_level"] and p["keys_per_row"] == G * NB
        assert 1 <= p["rows_per_block"] and p["rows_per_block"] * p["keys_per_row"] <= 32768    # the LDS histogram of a workgroup
        counts_words = p["NBT"]
    b = {k[2:]: v for k, v in p.items() if k.startswith("b_")}
    assert b["dig"] >= 4 * p["Mmax"] and b["counts"] >= 4 * counts_words and b["tile_sums"] >= 4 * p["ntiles"] and b["bstart"] >= 4 * (p["NBT"] + 1)
    assert b["entries"] >= 8 * p["entries_padded"] and b["bucket_acc"] >= 144 * p["NBT"]
    if p["two_level"]:
        assert p["fine"] == 1 << p["shift"] and p["nseg_max"] >= p["Mmax"] // 16384 + p["NBTc"]     # sum over bins of ceil(count / 16384) <= this
        assert b["bstart1"] >= 4 * (p["NBTc"] + 1) and b["seg_first"] >= 4 * (p["NBTc"] + 1) and b["seg_counts"] >= 4 * p["nseg_max"] * p["fine"]
        assert b["entries1"] >= 8 * p["Mmax"]
    # the partial-sum lists: k_accum0 writes two slots per chunk into list 0, or (fused) two per wave into list 1; every level reads `cur` and writes 2 per 64
    waves = ceil_div(p["nchunks0"], 64)
    need = [0, 0]
    need[1 if p["merge_fused"] else 0] = 2 * waves if p["merge_fused"] else 2 * p["nchunks0"]
    if p["merge_first"] != NONE:
        assert not p["merge_fused"] and merge1
        assert p["merge_first_grid"] == (waves if p["merge_first"] == COOP else ceil_div(waves, 4))
        assert (p["merge_first"] == COOP) == (bool(coop) and waves <= 384)
        need[1] = max(need[1], 2 * waves)
    cur, levels = p["merge_cur"], [p[f"merge_len{i}"] for i in range(p["merge_nlevels"])]
    assert p["merge_nlevels"] <= 8
    if levels:
        assert levels[0] == (2 * waves if merge1 else 2 * p["nchunks0"]) and cur == (1 if merge1 else 0) and levels[-1] <= 64
        for i, ln in enumerate(levels):
            assert ln <= need[cur] and (i == 0 or ln == 2 * ceil_div(levels[i - 1], 64)) and (ln > 64 or i == len(levels) - 1)
            need[cur ^ 1] = max(need[cur ^ 1], 2 * ceil_div(ln, 64))
            cur ^= 1
    else:
        assert waves <= 1 and merge1
    for i in (0, 1):
        assert b[f"lkeys{i}"] >= 4 * need[i] and b[f"lvals{i}"] >= 144 * need[i]
    assert b["rowcol"] >= 144 * p["rc_waves"] and b["group_sums"] >= 144 * gt
    if coop and p["skip_reduce"] != 1:
        assert b["wsum"] >= 144 * 4 * gt               # k_reduce_weighted_coop: grid (gt, 2), two sums each


def test_invariants_over_the_grid(host):
    cases = grid()
    ok = errors = 0
    for inp in cases:
        rs, p, why = plan(host, inp)
        c, W, G, rows, row_len = inp[:5]
        too_many = rows * G << (c - 1) > 1 << 22 or rows * row_len >= 1 << 31 or rows * row_len * W >= 1 << 32
        lds = rows > 1 and not inp[6] and G << (c - 1) > 32768
        assert (rs != 0) == (too_many or lds), (inp, why)
        if rs:
            assert rs == 1 and why                      # REEF_ERR_ARG
            errors += 1
            continue
        invariants(inp, p)
        ok += 1
    assert ok > 1000 and errors > 50, (ok, errors)


def test_the_grid_under_the_sanitizers(host, tmp_path):
    """The same function as a stand-alone program built with -fsanitize=address,undefined: every plan of the grid, and the same numbers."""
    if _stale(EXE):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DPLAN_CHECK_MAIN", SRC, "-o", EXE])
    cases = grid()
    path = tmp_path / "grid.txt"
    path.write_text("".join(" ".join(str(v) for v in inp) + "\n" for inp in cases))
    r = subprocess.run([EXE, str(path)], capture_output=True, text=True)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    for inp, line in zip(cases, lines):
        rs, p, _ = plan(host, inp)
        got = [int(v) for v in line.split()]
        assert got[0] == rs and (rs != 0 or got[1:] == [p[k] for k in host.names]), inp


# ---------------------------------------------------------------------------------------------- the three errors at their bounds
def test_error_returns_at_their_bounds(host):
    def status(inp):
        rs, _, why = plan(host, inp)
        return rs, why
    # 2^22 bucket keys fit the scan: c = 20 (NB = 2^19) with 8 groups; 9 do not.  Rows count as groups.
    assert status(case(20, 8, 1000)) == (0, "")
    assert status(case(20, 9, 1000)) == (1, "too many buckets")
    assert status(case(13, 1, 100, rows=1024, slice_sort=1))[0] == 0 and status(case(13, 1, 100, rows=1025, slice_sort=1)) == (1, "too many buckets")
    # N < 2^31 and N * W < 2^32
    assert status(case(13, 1, (1 << 31) - 1, W=1))[0] == 0 and status(case(13, 1, 1 << 31, W=1)) == (1, "too many digits")
    assert status(case(13, 1, 1 << 30, W=1, rows=2, slice_sort=1)) == (1, "too many digits")
    assert status(case(17, 1, (1 << 28) - 1))[0] == 0 and status(case(17, 1, 1 << 28)) == (1, "too many digits")
    # a row's keys must fit one workgroup's LDS histogram: 32768
    assert status(case(16, 1, 100, rows=2))[0] == 0 and status(case(15, 2, 100, rows=2))[0] == 0
    assert status(case(17, 1, 100, rows=2)) == (1, "row MSM: window too large for the LDS sort")
    assert status(case(15, 3, 100, rows=2)) == (1, "row MSM: window too large for the LDS sort")
    assert status(case(17, 1, 100, rows=2, slice_sort=1))[0] == 0                         # the sliced sort has no such bound
    # the order of the checks is run_core's: buckets before digits before the row sort
    assert status(case(20, 9, 1 << 31, W=1))[1] == "too many buckets" and status(case(17, 1, 1 << 30, rows=2))[1] == "too many digits"
