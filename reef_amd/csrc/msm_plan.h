// The launch plan of the bucket pipeline (engine.inc: run_core): everything one MSM's chain of launches is decided by, as one pure
// function of integers.  Host only, no HIP: engine.inc launches what the plan says, tools/plan_check.cpp compiles this file with g++ and
// tests/test_core_plan_host.py checks the decisions without a GPU.  The constants the decisions rest on are defined here, once;
// msm_kernels.inc and engine.inc use them from here.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/reef_msm.h"

namespace reef {

static constexpr uint32_t SCAN_BLOCK = 1024, SCAN_ITEMS = 4, SCAN_TILE = SCAN_BLOCK * SCAN_ITEMS;   // k_scan_tiles: keys per workgroup
static constexpr uint32_t SCAN_SMALL_SLICES = 64;              // k_scan_small: slices one workgroup keeps in flight
static constexpr uint32_t SORT_SEG = 16384;                    // second sort level: entries per workgroup
static constexpr uint32_t MAX_LDS_KEYS = 32768;                // 128 KiB of LDS counters per workgroup
static constexpr uint32_t MAX_SCAN_KEYS = SCAN_TILE * 1024;
static constexpr uint32_t SORT_SHIFT = 8;                      // two-level sort: 256 buckets per coarse bin
static constexpr uint64_t TWO_LEVEL_MIN_ENTRIES = 1u << 20;    // below this the one-level sort's shorter kernel chain wins
static constexpr uint32_t SCAN_WAVE_MAX_KEYS = 4096;           // up to here a wave per key sums the slices (k_scan_small, k_slice_totals_w / k_scan_finish_w)
static constexpr uint32_t ONE_WAVE_PER_SIMD_CHUNKS = 65536;    // 1024 SIMDs x 64 lanes: the grid of k_accum0 up to 48 entries per chunk, and the most the fused first merge takes
static constexpr uint32_t COOP_MERGE_MAX_WAVES = 384;          // four waves per addition pay while the chip is not full of them
static constexpr uint32_t ROWCOL_SHARED_MIN_BUCKETS = 1u << 16;   // engine.inc: rowcol_lanes
static constexpr int ROWCOL_SHARED_LANES = 32;
static constexpr uint32_t XYZZ_BYTES = 144, ENTRY_BYTES = 8;   // sizeof(xyzz_mem), sizeof(u32x2): engine.inc asserts both
static constexpr int MERGE_MAX_LEVELS = 8;                     // a list of < 2^32 partial sums shrinks 32-fold per level

struct CorePlan {
    uint32_t c, W, G;       // window bits, windows used, bucket groups per result
    uint32_t rows, row_len; // rows == 1: single MSM over N = row_len scalars
    uint32_t n_ctx;         // table stride
    bool slice_sort = false;  // rows > 1 only: long rows, sorted by the sliced K1 sort (a batch of MSMs)
};
// What the ctx and the call add to the shape.
struct CoreCtxOpts {
    uint32_t L0;            // entries per accumulation thread, 0: chosen here
    bool coop;              // tail kernels with four waves per group operation
    int two_level;          // sort: -1 by size, 0 never, 1 whenever the window allows
    int rowcol_lanes;       // engine.inc: rowcol_lanes (it reads a live counter, so it is an input)
    bool group_sums_out;    // the caller finishes the window combine from the group sums
};
// The experiment switches (common.h: exp_env; engine.inc: core_switches reads them once).  The defaults are what an unset variable means.
struct CoreSwitches {
    bool fuse_merge = true;               // REEF_MSM_FUSE_MERGE=0: k_accum0 never runs the first merge level itself
    bool merge1 = true;                   // REEF_MSM_MERGE1=0: slot-per-lane first merge level (k_accumN on the chunks' slots)
    uint32_t fuse_max_chunks = ONE_WAVE_PER_SIMD_CHUNKS;   // REEF_MSM_FUSE_MAX_CHUNKS
    bool fuse_recode = true;              // REEF_MSM_FUSE_RECODE=0: k_recode and k_count stay two kernels
    bool sort_compact = true;             // REEF_MSM_SORT_COMPACT=0: 8-byte entries between the two sort levels
    bool sort_word = true;                // REEF_MSM_SORT_WORD=0: 8-byte sorted entries
    int skip_reduce = 0;                  // REEF_MSM_SKIP_REDUCE (TIMING ONLY): 1 leaves the bucket reduction out, 2 its row / column sums
};

// Partial merge after k_accum0: the two slots per chunk -> bucket sums.  A first level with a chunk per lane (k_merge_chunks, or k_accum0
// itself when fused), then k_accumN levels on the two slots per wave, from list `cur` to list `cur ^ 1` and back, until one wave is left.
enum MergeFirst : uint32_t { MERGE_FIRST_NONE = 0, MERGE_FIRST_COOP, MERGE_FIRST_PLAIN };
struct MergePlan {
    uint32_t fused;         // k_accum0<C, true> writes the level-1 lists itself
    uint32_t first;         // MergeFirst: the k_merge_chunks launch, if any
    uint32_t first_grid;
    uint32_t cur;           // the list the first k_accumN level reads
    uint32_t nlevels;
    uint32_t len[MERGE_MAX_LEVELS];   // list length per k_accumN level
};
enum ScanRoute : uint32_t { SCAN_SMALL = 0, SCAN_WAVE, SCAN_TILES };   // k_scan_small | k_slice_totals_w .. k_scan_finish_w | k_slice_totals .. k_scan_finish

struct CoreBytes {          // the workspace buffers of Ctx, by name; 0: the chain does not touch it
    uint64_t dig, counts, tile_sums, bstart, entries;
    uint64_t bstart1, seg_first, seg_counts, entries1;
    uint64_t bucket_acc, lkeys[2], lvals[2];
    uint64_t rowcol, group_sums, wsum;
};
struct CoreLaunch {
    uint64_t N, Mmax, entries_padded;          // scalars, digits, entry slots of k_accum0's chunks
    uint32_t NB, NBT, groups_total;            // buckets per group, buckets, bucket groups of all rows
    uint32_t L0, nchunks0;
    uint32_t row_mode, two_level, shift, compact, word_entries;
    uint32_t NBc, NBTc, KB, P, S, per;         // (coarse) keys per group and in all, keys per LDS part, parts, slices, scalars per slice
    uint32_t rows_per_block, keys_per_row;     // row mode
    uint32_t recode_fused;
    uint32_t scan, ntiles;                     // ScanRoute
    uint32_t nseg_max, fine;                   // two-level
    MergePlan merge;
    uint32_t c1, c2, rc_waves, direct;
    int32_t rowcol_lanes, skip_reduce;
    CoreBytes bytes;
};
// core_launch_plan zero-fills its output before it sets the fields, so two plans are the same chain of launches exactly when their
// bytes are equal (engine.inc: run_core_graphed keys a captured chain on this).
static inline bool same_plan(const CoreLaunch &a, const CoreLaunch &b) { return memcmp(&a, &b, sizeof a) == 0; }

static inline uint32_t ceil_div(uint64_t a, uint64_t b) { return (uint32_t)((a + b - 1) / b); }
static inline uint64_t round_up(uint64_t a, uint64_t b) { return (a + b - 1) / b * b; }
template <class T> static inline T plan_min(T a, T b) { return a < b ? a : b; }
template <class T> static inline T plan_max(T a, T b) { return a < b ? b : a; }

// Does the accumulation kernel run the first merge level itself (k_accum0<C, true>)?  Mid-size inputs only: one wave per SIMD
// (up to 65536 chunks), where the merged kernel's registers cost no occupancy, and only where the first level would run one
// wave per 64 chunks anyway (beyond 384 waves; below, four waves share each addition).
static inline MergePlan merge_plan(uint32_t nchunks0, bool coop, const CoreSwitches &sw, bool may_fuse) {
    MergePlan m{};
    uint32_t waves = ceil_div(nchunks0, 64);
    const bool coop_first = coop && waves <= COOP_MERGE_MAX_WAVES;
    m.fused = may_fuse && sw.fuse_merge && sw.merge1 && nchunks0 <= sw.fuse_max_chunks && !coop_first;
    uint32_t len = 2 * waves;
    m.cur = 1;
    if (!sw.merge1) { len = 2 * nchunks0; m.cur = 0; waves = 2; }
    else if (m.fused) {}
    else if (coop_first) { m.first = MERGE_FIRST_COOP; m.first_grid = waves; }
    else { m.first = MERGE_FIRST_PLAIN; m.first_grid = ceil_div(waves, 4); }
    if (waves <= 1) return m;
    for (;;) {
        m.len[m.nlevels++] = len;
        if (len <= 64) break;
        len = 2 * ceil_div(len, 64);
    }
    return m;
}

static inline reef_status core_launch_plan(const CorePlan &pl, const CoreCtxOpts &o, const CoreSwitches &sw, CoreLaunch *out, const char **why) {
    memset(out, 0, sizeof *out);
    CoreLaunch &p = *out;
    CoreBytes &by = p.bytes;
    p.N = (uint64_t)pl.rows * pl.row_len;
    p.NB = 1u << (pl.c - 1);
    p.groups_total = pl.rows * pl.G;
    const uint64_t NBT64 = (uint64_t)p.groups_total * p.NB;
    p.Mmax = p.N * pl.W;
    if (NBT64 > MAX_SCAN_KEYS) { *why = "too many buckets"; return REEF_ERR_ARG; }
    if (p.N >= (1ull << 31) || p.Mmax >= (1ull << 32)) { *why = "too many digits"; return REEF_ERR_ARG; }
    p.NBT = (uint32_t)NBT64;
    // entries per accumulation thread: about one bucket's worth (few runs cut by chunk edges), but enough threads to fill the chip
    p.L0 = o.L0;
    if (p.L0 == 0) {
        // k_accum0 is bound by integer issue and a lone wave saturates its SIMD: while the input is too small to keep two
        // waves per SIMD in long chunks, the shortest chain is one wave per SIMD (1024 waves = 65536 chunks) -- more threads
        // would only share the SIMDs and leave more partial sums to merge.  Large inputs: long chunks, two waves per SIMD.
        // The grid is a whole number of waves per SIMD: 65536 chunks (one wave on each of the 1024 SIMDs) up to 48 entries
        // per chunk, 131072 chunks (two waves per SIMD, which hides the table gathers better) beyond.
        if (p.Mmax <= 48ull * ONE_WAVE_PER_SIMD_CHUNKS) p.L0 = (uint32_t)plan_max<uint64_t>(4, ceil_div(p.Mmax, ONE_WAVE_PER_SIMD_CHUNKS));
        else p.L0 = (uint32_t)plan_min<uint64_t>(128, ceil_div(p.Mmax, 2 * ONE_WAVE_PER_SIMD_CHUNKS));
    }
    p.nchunks0 = (uint32_t)round_up(ceil_div(p.Mmax, p.L0), 64);
    p.entries_padded = (uint64_t)p.nchunks0 * p.L0;

    // ---- counting sort by bucket
    p.row_mode = pl.rows > 1 && !pl.slice_sort;
    // large inputs: two-level sort (coarse bins of 2^SORT_SHIFT buckets, then each bin by its low key bits)
    p.two_level = !p.row_mode && o.two_level != 0 && p.NB >= (64u << SORT_SHIFT) && (o.two_level > 0 || p.Mmax >= TWO_LEVEL_MIN_ENTRIES);
    // one-word entries between the two levels when the point index, the low key bits and the sign fit in 32 bits: with
    // SORT_SHIFT low bits, or with one fewer (twice the coarse bins) -- 2^20 points x 16 tables need the latter
    const uint64_t index_span = (uint64_t)ceil_div(pl.W, pl.G) * pl.n_ctx;       // payloads are j * n_ctx + i, j < tables per group
    p.shift = p.two_level ? SORT_SHIFT : 0u;
    if (p.two_level && sw.sort_compact) {
        if (index_span <= (1ull << (31 - SORT_SHIFT))) p.compact = 1;
        else if (index_span <= (1ull << (32 - SORT_SHIFT))) { p.compact = 1; p.shift = SORT_SHIFT - 1; }
    }
    p.word_entries = p.compact && sw.sort_word;        // one-word sorted entries: k_accum0 takes its keys from bucket_start[]
    p.NBc = p.NB >> p.shift;                           // keys per group seen by the (coarse) histogram
    p.NBTc = p.groups_total * p.NBc;
    if (!p.row_mode) {
        p.KB = plan_min(p.NBc, MAX_LDS_KEYS);
        p.P = p.NBc / p.KB;
        p.S = plan_max<uint32_t>(1, plan_min<uint32_t>(ceil_div(256, (uint64_t)p.groups_total * p.P), ceil_div(pl.row_len, 1024)));   // one workgroup per CU
        p.per = ceil_div(pl.row_len, p.S);
        p.S = ceil_div(pl.row_len, p.per);
        // a single MSM with one bucket group whose (coarse) histogram fits one LDS part: the thread that recodes a scalar counts
        // its digits too (k_recode_count); the grid is the slices
        p.recode_fused = sw.fuse_recode && p.groups_total == 1 && p.P == 1;
        by.counts = ((uint64_t)p.S + 1) * p.NBTc * sizeof(uint32_t);
    } else {
        p.keys_per_row = pl.G * p.NB;
        if (p.keys_per_row > MAX_LDS_KEYS) { *why = "row MSM: window too large for the LDS sort"; return REEF_ERR_ARG; }
        // whole rows per workgroup: bounded by LDS keys and ~64Ki digits of work
        p.rows_per_block = plan_max<uint32_t>(1, MAX_LDS_KEYS / p.keys_per_row);
        p.rows_per_block = plan_min<uint32_t>(p.rows_per_block, plan_max<uint32_t>(1, 65536 / plan_max<uint32_t>(1, pl.row_len)));
        by.counts = (uint64_t)p.NBT * sizeof(uint32_t);
    }
    p.ntiles = ceil_div(p.NBTc, SCAN_TILE);
    // few keys: slice totals + scan + cursors in one workgroup; else three phases, a wave or a thread per key
    if (!p.row_mode && p.NBTc <= SCAN_WAVE_MAX_KEYS && (p.NBTc & 3u) == 0 && p.S <= SCAN_SMALL_SLICES) p.scan = SCAN_SMALL;
    else p.scan = !p.row_mode && p.NBTc <= SCAN_WAVE_MAX_KEYS ? SCAN_WAVE : SCAN_TILES;
    if (p.two_level) {
        p.nseg_max = (uint32_t)ceil_div(p.Mmax, SORT_SEG) + p.NBTc;
        p.fine = 1u << p.shift;
        by.bstart1 = ((uint64_t)p.NBTc + 1) * sizeof(uint32_t);
        by.entries1 = p.entries_padded * ENTRY_BYTES;
        by.seg_first = ((uint64_t)p.NBTc + 1) * sizeof(uint32_t);
        by.seg_counts = (uint64_t)p.nseg_max * p.fine * sizeof(uint32_t);
    }
    by.dig = p.Mmax * sizeof(uint32_t);
    by.bstart = ((uint64_t)p.NBT + 1) * sizeof(uint32_t);
    by.tile_sums = 1024 * sizeof(uint32_t);
    by.entries = p.entries_padded * ENTRY_BYTES;

    // ---- bucket accumulation and partial merge
    p.merge = merge_plan(p.nchunks0, o.coop, sw, true);
    const uint32_t len1 = 2 * p.nchunks0, len2 = 2 * ceil_div(len1, 64);
    by.bucket_acc = (uint64_t)p.NBT * XYZZ_BYTES;
    by.lkeys[0] = (uint64_t)len1 * sizeof(uint32_t);
    by.lvals[0] = (uint64_t)len1 * XYZZ_BYTES;
    by.lkeys[1] = (uint64_t)len2 * sizeof(uint32_t);
    by.lvals[1] = (uint64_t)len2 * XYZZ_BYTES;

    // ---- bucket reduction (row/column sums, two short weighted sums), final Horner over groups
    const uint32_t lg = pl.c - 1;                      // NB = 2^lg
    p.c2 = (lg + 1) / 2;
    p.c1 = lg - p.c2;
    p.rc_waves = p.groups_total * ((1u << p.c1) + (1u << p.c2));
    p.direct = !o.group_sums_out && pl.G == 1;         // one group per result: no Horner, no separate conversion kernel
    p.rowcol_lanes = o.rowcol_lanes;                   // rc_waves sums: on four waves each (0), or that many lanes each
    p.skip_reduce = sw.skip_reduce;
    by.rowcol = (uint64_t)p.rc_waves * XYZZ_BYTES;
    by.group_sums = (uint64_t)p.groups_total * XYZZ_BYTES;
    if (o.coop && sw.skip_reduce != 1) by.wsum = (uint64_t)p.groups_total * 4 * XYZZ_BYTES;
    return REEF_OK;
}

}  // namespace reef
