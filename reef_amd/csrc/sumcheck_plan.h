// The decisions of the sum-check engine (row N2, sumcheck_engine.inc), as pure functions of integers: the switches from their text,
// the grid of every launch, the row lists of a structured table from its row flags, and the route one round takes from the state
// the calls before it left.  Host only, no HIP: sumcheck_engine.inc launches what the plan says and changes the state,
// tools/sc_plan_check.cpp compiles this file with g++ and tests/test_sc_plan_host.py checks the decisions without a GPU.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "msm_plan.h"     // ceil_div, plan_min, plan_max

namespace reef {

// ---- the tuning switches.  The defaults are what an unset variable means.
struct ScSwitches {
    bool one_launch = true;              // REEF_SC_ONE_LAUNCH=0: the sums of a round are finished by a second kernel and copied back (rounds 1-2 form), for A/B runs
    bool rank1 = true;                   // REEF_SC_RANK1=0: gen_eq_table writes the EQ table out, as rounds 1-2 did
    bool structured = true;              // REEF_SC_STRUCT=0: the first round of a step reads the pristine table as dense field elements whatever it holds
    bool identity = true;                // REEF_SC_IDENTITY=0: all three sums of a fused rank-one round are accumulated
    bool defer = true;                   // REEF_SC_DEFER=0: the first fold of a structured table is written out at once (round 3 form)
    // REEF_SC_RANK1_MIN_POW: rounds below this many entries per half are launch-latency-bound; there the dense fused kernel (one launch and
    // the final sums) is shorter than the rank-one round (row factors, pass, final sums), so EQ is written out once the tables have shrunk
    // to it (measured: 2^21-entry tables 1.18 ms dense, 1.27 ms rank-one; 2^24: 2.31 / 2.02; 2^26: 5.67 / 3.68).
    uint64_t r1_min_pow = (uint64_t)1 << 21;
    uint32_t floor_blocks = 256;         // REEF_SC_FLOOR: a dense round of long threads is spread over at least this many blocks
    uint32_t one_launch_max = 64;        // REEF_SC_ONE_LAUNCH_MAX: a round of at most this many blocks finishes its sums itself (the last block to arrive)
    uint64_t split_max = (uint64_t)1 << 14;   // REEF_SC_SPLIT_MAX: rounds of at most this many pairs spread an item over four waves (0: never)
    uint32_t split_blocks = 64;          // REEF_SC_SPLIT_BLOCKS: the most workgroups of such a round (every one adds 27 words to the shared sums: 256 of them cost the 2^14-pair round 7 us)
    uint32_t items = 8;                  // REEF_SC_ITEMS: pairs a thread of a dense round takes at least (its three lazy reductions and the block's sums are per thread)
    uint32_t order = 2;                  // REEF_SC_FENCE: how a multi-block one-launch round orders its additions before the ticket (sumcheck_kernels.inc: SC_ORDER_*)
    uint32_t set_sub = 8;                // REEF_SC_SET_SUB: the most 128-entry tiles a wave of k_sc_set_parts takes (two entries per lane and tile)
    uint32_t blocks_cap = 2048;          // REEF_SC_BLOCKS: the most blocks a round is spread over (A/B runs)
};
// The text of each variable, null where it is unset (sumcheck_engine.inc: sc_read_switches is the one reader of the environment).
struct ScSwitchText {
    const char *one_launch, *rank1, *structured, *identity, *defer, *r1_min_pow, *floor_blocks, *one_launch_max, *split_max, *split_blocks, *items, *order,
        *set_sub, *blocks_cap;
};
static inline ScSwitches sc_parse_switches(const ScSwitchText &t) {
    ScSwitches s;
    auto off = [](const char *e) { return e && e[0] == '0'; };
    // unset or empty: the default; else the number, clamped
    auto num = [](const char *e, long long lo, long long hi, uint64_t unset) { return (e && *e) ? (uint64_t)plan_min(hi, plan_max(lo, atoll(e))) : unset; };
    const long long NO_CAP = INT64_MAX;
    s.one_launch = !off(t.one_launch);
    s.rank1 = !off(t.rank1);
    s.structured = !off(t.structured);
    s.identity = !off(t.identity);
    s.defer = !off(t.defer);
    s.r1_min_pow = num(t.r1_min_pow, 1, NO_CAP, s.r1_min_pow);
    s.floor_blocks = (uint32_t)num(t.floor_blocks, 1, 8192, s.floor_blocks);
    s.one_launch_max = (uint32_t)num(t.one_launch_max, 1, 8192, s.one_launch_max);
    s.split_max = num(t.split_max, 0, NO_CAP, s.split_max);
    s.split_blocks = (uint32_t)num(t.split_blocks, 1, 1024, s.split_blocks);
    s.items = (uint32_t)num(t.items, 1, 64, s.items);
    s.order = (uint32_t)num(t.order, 0, 2, s.order);   // 2 (default since round 6): acq_rel ticket; 1: __threadfence before the ticket; 0: returning atomics + s_waitcnt only
    s.set_sub = (uint32_t)num(t.set_sub, 1, 64, s.set_sub);
    s.blocks_cap = (uint32_t)num(t.blocks_cap, 1, 8192, s.blocks_cap);
    return s;
}

// ---- grids
struct ScGrid { uint32_t x, y; };
// the most blocks a dense round of this ctx is spread over: a pair per thread, up to the cap
static inline uint32_t sc_nblocks(uint64_t len, uint32_t cap) { return (uint32_t)plan_min<uint64_t>(cap, plan_max<uint64_t>(1, len / 2 / 256)); }
// Blocks of a dense round over `work` pairs: a thread pays ~7 products of fixed work (three lazy reductions, the wave's sums)
// against ~5 per pair, so a mid-sized round is spread over fewer, longer threads (2^20 pairs: 109 -> 74 us with 8 pairs each).
static inline uint32_t sc_dense_blocks(uint64_t work, uint32_t nblocks, const ScSwitches &sw) {
    const uint64_t one_each = plan_max<uint64_t>(1, ceil_div(work, 256));      // a pair per thread: the shortest chain
    const uint64_t longer = plan_max<uint64_t>(sw.floor_blocks, ceil_div(work, (uint64_t)256 * sw.items));   // never fewer blocks than CUs for it
    return (uint32_t)plan_min<uint64_t>(nblocks, plan_min(one_each, longer));
}
// One-launch rounds only for rounds of a few blocks: 2048 blocks adding 27 limbs each to the same 27 words serialise (2^20-entry
// round: 58 -> 103 us), a small round saves its second kernel and its copy (46 -> 37 us per round, 16 of the 21 rounds of a 2^21 step).
static inline bool sc_one_launch(uint32_t blocks, const ScSwitches &sw) { return sw.one_launch && blocks <= sw.one_launch_max; }
// a small fused round (k_sc_fold_coeffs_split): an item over four waves, 64 pairs per workgroup and pass
static inline uint32_t sc_split_blocks(uint64_t pairs, const ScSwitches &sw) { return (uint32_t)plan_min<uint64_t>(sw.split_blocks, plan_max<uint64_t>(1, ceil_div(pairs, 64))); }
// the grid-stride kernels with an entry per thread (k_sc_fold, k_sc_r1_fold, k_sc_eq_table) over n entries
static inline uint32_t sc_fold_blocks(uint64_t n) { return (uint32_t)plan_min<uint64_t>(4096, plan_max<uint64_t>(1, ceil_div(n, 256))); }
// k_sc_r1_prep: a thread per pair row of the next sums and per mass that moves; r1_hi = FH bits before, folded: with a challenge
static inline uint32_t sc_r1_prep_blocks(uint32_t r1_hi, bool folded, uint32_t nq) {
    const uint32_t hc = 1u << r1_hi, hn_next = (folded ? hc >> 1 : hc) >> 1;
    return ceil_div(plan_max<uint32_t>(plan_max<uint32_t>(hn_next, folded ? nq : 0u), 1u), 256);
}
// grid of the column kernels for `hn` pair rows: blocks over the columns x row groups, at most 1024 blocks (every block
// leaves 36 limb sums for k_sc_r1_final to add up: 2048 of them cost it 25 us)
static inline ScGrid sc_r1_grid(uint32_t r1_lo, uint32_t hn, uint32_t *rows_per_chunk) {
    const uint32_t gx = ceil_div((uint64_t)1 << r1_lo, 256);
    const uint32_t chunks = plan_max<uint32_t>(1u, plan_min<uint32_t>(hn, plan_max<uint32_t>(1u, 1024u / gx)));
    *rows_per_chunk = ceil_div(hn, chunks);
    return ScGrid{gx, ceil_div(hn, *rows_per_chunk)};
}
// grid of a list-driven column kernel: blocks over the columns x row groups (at most 2048 blocks, at most 256 rows per thread)
static inline ScGrid sc_list_grid(uint32_t r1_lo, uint32_t nlist) {
    const uint32_t gx = ceil_div((uint64_t)1 << r1_lo, 256);
    return ScGrid{gx, plan_max<uint32_t>(1u, plan_min<uint32_t>(nlist, plan_max<uint32_t>(plan_max<uint32_t>(1u, 1024u / gx), ceil_div(nlist, 256))))};
}
// k_sc_set_parts: tiles per wave: 8 (16 entries per lane) where that still leaves 8192 waves -- by measurement at 2^26 entries, where the
// kernel alone takes a quarter less time with 4 tiles than with 1 (the sweep: profiles/r12_sc_set_parts_timing.txt); four waves a block
static inline uint32_t sc_set_parts_blocks(uint64_t len, const ScSwitches &sw, uint32_t *sub) {
    const uint32_t tiles = ceil_div(len, 128);
    *sub = plan_max<uint32_t>(1u, plan_min<uint32_t>(sw.set_sub, tiles / 8192u));
    return ceil_div(ceil_div(tiles, *sub), 4);
}

// ---- which tables get what
// gen_eq_table's split of the ell index bits: the low ell / 2 are columns, the others rows
static inline uint32_t sc_lo_bits(uint64_t len) {
    uint32_t ell = 0;
    while (((uint64_t)1 << ell) < len) ++ell;
    return ell / 2;
}
static inline uint32_t sc_hi_bits(uint64_t len) {
    uint32_t ell = 0;
    while (((uint64_t)1 << ell) < len) ++ell;
    return ell - ell / 2;
}
// Does a table of `len` entries get a row structure?  Only tables the rank-one rounds serve.  Returns its rows, 0: none.
static inline uint32_t sc_struct_rows(uint64_t len, const ScSwitches &sw) {
    const uint32_t hi = sc_hi_bits(len);
    return (!sw.rank1 || !sw.structured || hi < 2 || len / 2 < sw.r1_min_pow) ? 0u : 1u << hi;
}
// Does EQ start a step as FH (x) FL + masses, nothing of its 2^ell entries written?
static inline bool sc_eq_rank1(uint64_t len, const ScSwitches &sw) { return sc_hi_bits(len) >= 1 && sw.rank1 && len / 2 >= sw.r1_min_pow; }

// ---- the row lists of a structured table (sumcheck_kernels.inc, "a pristine table with structure"), for H rows: one array of row
// numbers, each list a stretch of it
struct ScList { uint32_t off = 0, n = 0; };
struct ScRowLists {
    ScList sum[2][3];                    // round-one sums: [side][class W, S, K] -> pair rows h < H/2
    ScList fast, gen;                    // first fold: h < H/4 whose four sources are all K or S / the others
    // first fold deferred by one round (sumcheck_kernels.inc): g < H/8 with both quadruples g, g + H/8 fast (f8), the same rows
    // as a list of quadruples (f8x), the fast quadruples that are not among them (frest), the g that are not in f8 (g8)
    ScList f8, f8x, frest, g8;
    ScList d8[4][2];                     // the rows of f8x by source block b (row h + b * H/4) and class: [b][0] S rows, [b][1] K rows
};
// flags: bit 1 set: a K row (constant), else bit 0 set: an S row (small entries), else W.  False, and nothing written: fewer than half
// the rows are K or S, the table gets no structure.  `lists` ends with one word more than the lists hold (no kernel is handed a
// pointer past the array when the last list is empty).
static inline bool sc_build_row_lists(const uint32_t *flags, uint32_t H, ScRowLists *out, std::vector<uint32_t> *lists) {
    auto cls = [&](uint32_t row) { return (flags[row] & 2u) ? 2u : (flags[row] & 1u) ? 1u : 0u; };   // K, S, W
    uint64_t plain = 0;
    for (uint32_t r = 0; r < H; ++r) plain += cls(r) != 0;
    if (2 * plain < H) return false;
    lists->clear();
    const uint32_t hn = H / 2, hq = H / 4, h8 = hq / 2;
    auto collect = [&](ScList *l, uint32_t rows, auto &&member) {
        l->off = (uint32_t)lists->size();
        for (uint32_t h = 0; h < rows; ++h)
            if (member(h)) lists->push_back(h);
        l->n = (uint32_t)lists->size() - l->off;
    };
    auto fast = [&](uint32_t h) { return cls(h) && cls(h + hq) && cls(h + 2 * hq) && cls(h + 3 * hq); };
    auto fast8 = [&](uint32_t g) { return h8 && fast(g) && fast(g + h8); };
    auto in_f8x = [&](uint32_t h) { return h8 && fast8(h % h8); };
    for (uint32_t side = 0; side < 2; ++side)
        for (uint32_t k = 0; k < 3; ++k) collect(&out->sum[side][k], hn, [&](uint32_t h) { return cls(h + side * hn) == k; });
    collect(&out->fast, hq, fast);
    collect(&out->gen, hq, [&](uint32_t h) { return !fast(h); });
    collect(&out->f8, h8, fast8);
    collect(&out->f8x, hq, in_f8x);
    collect(&out->frest, hq, [&](uint32_t h) { return fast(h) && !in_f8x(h); });
    collect(&out->g8, h8, [&](uint32_t g) { return !fast8(g); });
    for (uint32_t b = 0; b < 4; ++b)
        for (uint32_t k = 0; k < 2; ++k)                   // cls: 1 = S, 2 = K
            collect(&out->d8[b][k], hq, [&](uint32_t h) { return in_f8x(h) && cls(h + b * hq) == k + 1; });
    lists->push_back(0);
    return true;
}

// ---- one round
// What the decisions read of the ctx (sumcheck_engine.inc: ScCtx has the meaning of each).
struct ScState {
    uint64_t len, valid_t, valid_e;
    uint32_t nblocks;
    bool r1;
    uint32_t r1_hi, r1_hi0, r1_lo, r1_nq;
    uint64_t r1_prev_pow;
    bool fresh, st_ok, defer_on;
    uint64_t defer_pow;
    uint32_t defer_hq;
    ScRowLists st;                       // the sizes are read
};
enum ScCall : uint32_t { SC_COEFFS = 0, SC_FOLD, SC_FOLD_COEFFS };
enum ScRoute : uint32_t {
    // reef_sc_round_coeffs
    SC_SUMS_STRUCT = 0,   // the first round of a step on a structured table: per side the S rows, the W rows, and the K rows of both in one launch
    SC_SUMS_R1,           // EQ rank-one: k_sc_r1_coeffs
    SC_SUMS_DENSE,        // k_sc_coeffs (EQ written out first if it was rank-one)
    // reef_sc_fold
    SC_FOLD_R1,           // FH and T folded apart; EQ written out after it if that was the last FH bit
    SC_FOLD_DENSE,        // k_sc_fold (EQ written out first if it was rank-one)
    // reef_sc_fold_coeffs
    SC_FC_R1,             // the next round stays rank-one: fold and its sums in one pass over T
    SC_FC_STRUCT,         // ... of a structured table: fast rows from their 4-byte sources, the others through the general kernel
    SC_FC_DEFER,          // ... and the next round will be of this kind too: the rows of f8x are not written
    SC_FC_SECOND,         // the call after that one: the second fold of those rows, straight from the sources
    SC_FC_LAST_R1,        // last rank-one round (FH bits used up, or the tables are small now): fold T, write EQ out, dense sums
    SC_FC_SPLIT,          // a small round: an item over four waves, always one launch
    SC_FC_DENSE,          // k_sc_fold_coeffs
};
struct ScRoundPlan {
    uint32_t flush;           // a deferred first fold is written out before anything else: this call is not its second fold
    uint32_t route;           // ScRoute
    uint32_t ident;           // the sum-check identity spares the sum t1 e1: the coefficients of this round are still on the device
    uint32_t materialize;     // EQ is written out: before the dense routes, after SC_FOLD_R1 (SC_FC_LAST_R1 always does)
    uint32_t one_launch;      // the dense sums finish in their own kernel
    uint32_t hn, hq;          // pair rows of the sums the route takes; SC_FC_SECOND: the rows of the deferred fold
    uint32_t blocks;          // the dense sums kernel (k_sc_coeffs, k_sc_fold_coeffs, k_sc_fold_coeffs_split)
    uint32_t fold_blocks;     // k_sc_fold, k_sc_r1_fold
    ScGrid grid;              // SC_SUMS_R1, SC_FC_R1: the column kernel over all rows, rows_per_chunk each
    uint32_t rows_per_chunk;
    uint32_t prep_blocks;     // k_sc_r1_kprep, k_sc_r2_kprep, k_sc_r2s_factors: a thread per row of hn
    ScGrid g_sum[2][2];       // SC_SUMS_STRUCT: [side][W, S]; a list's grid counts only where the list has rows
    ScGrid g_fast, g_gen;     // SC_FC_STRUCT; SC_FC_DEFER and SC_FC_SECOND: g_gen is the general kernel's (gen / g8)
    ScGrid g_frest, g_d8[4];  // SC_FC_DEFER: the fast rows that are written, the S rows of the deferred ones by source block
    ScGrid g_f8;              // SC_FC_SECOND
    uint32_t const_blocks;    // k_sc_r1s_const: x 2 sides (SC_SUMS_STRUCT) / x 4 source blocks (SC_FC_DEFER); 0: no K rows, no launch
    uint32_t points_blocks;   // SC_FC_DEFER: k_sc_defer_points; 0: no masses, no launch
};

// a round with `pow` can stay rank-one: both tables have exactly 2*pow live entries and the bit it folds is an FH bit
static inline bool sc_r1_round(const ScState &s, uint64_t pow, const ScSwitches &sw) {
    return s.r1 && s.r1_hi >= 1 && s.valid_e == 2 * pow && s.valid_t == 2 * pow && pow >= sw.r1_min_pow;
}
// the first round of a step on a structured table: tables are whole (2*pow = len), T is pristine, EQ is rank-one with all its FH bits
static inline bool sc_struct_round(const ScState &s, uint64_t pow, const ScSwitches &sw) {
    return s.st_ok && s.fresh && 2 * pow == s.len && s.r1_hi == s.r1_hi0 && sw.structured;
}

// REEF_ERR_ARG: the tables do not have the 2 * pow live entries the round needs.  `flush` is set even then where the engine writes a
// deferred fold out before it looks (coeffs and fold do, fold_coeffs does not).
static inline reef_status sc_round_plan(ScCall call, uint64_t pow, const ScState &s, const ScSwitches &sw, ScRoundPlan *out) {
    memset(out, 0, sizeof *out);
    ScRoundPlan &p = *out;
    const bool live = 2 * pow <= plan_min(s.valid_t, s.valid_e);
    if (call != SC_FOLD_COEFFS) p.flush = s.defer_on;          // neither is the second fold of a deferred one
    if (!live) return REEF_ERR_ARG;
    const bool r1 = sc_r1_round(s, pow, sw);
    auto dense_sums = [&](uint64_t pairs) {
        p.blocks = sc_dense_blocks(pairs, s.nblocks, sw);
        p.one_launch = sc_one_launch(p.blocks, sw);
    };
    if (call == SC_COEFFS) {
        if (r1 && sc_struct_round(s, pow, sw)) {
            p.route = SC_SUMS_STRUCT;
            p.hn = 1u << (s.r1_hi - 1);
            for (uint32_t side = 0; side < 2; ++side) {
                for (uint32_t k = 0; k < 2; ++k)
                    if (s.st.sum[side][k].n) p.g_sum[side][k] = sc_list_grid(s.r1_lo, s.st.sum[side][k].n);
                p.const_blocks = plan_max(p.const_blocks, ceil_div(s.st.sum[side][2].n, 256));   // one launch for both sides: the larger set's blocks, per side
            }
        } else if (r1) {
            p.route = SC_SUMS_R1;
            p.hn = 1u << (s.r1_hi - 1);
            p.grid = sc_r1_grid(s.r1_lo, p.hn, &p.rows_per_chunk);
        } else {
            p.route = SC_SUMS_DENSE;
            p.materialize = s.r1;
            dense_sums(pow);
        }
        return REEF_OK;
    }
    if (call == SC_FOLD) {
        p.fold_blocks = sc_fold_blocks(pow);
        p.route = r1 ? SC_FOLD_R1 : SC_FOLD_DENSE;
        p.materialize = r1 ? s.r1_hi == 1 : s.r1;              // the FH bits are used up: 2^lo entries, dense from here
        return REEF_OK;
    }
    // the next round stays rank-one too: fold and its sums in one pass over T
    const bool fused_r1 = r1 && s.r1_hi >= 2 && pow / 2 >= sw.r1_min_pow;
    const bool second = s.defer_on && pow == s.defer_pow && fused_r1;
    p.flush = s.defer_on && !second;
    if (fused_r1) {
        p.hn = 1u << (s.r1_hi - 2);
        p.ident = s.r1_prev_pow == pow && sw.identity;
        p.prep_blocks = ceil_div(p.hn, 256);
        if (sc_struct_round(s, pow, sw)) {
            // it is the first fold of a structured table and the next round will be of this kind too: defer what can be
            const bool defer = sw.defer && s.r1_hi >= 3 && pow / 4 >= sw.r1_min_pow && s.st.f8.n > 0;
            p.route = defer ? SC_FC_DEFER : SC_FC_STRUCT;
            p.g_gen = sc_list_grid(s.r1_lo, s.st.gen.n);
            if (!defer) {
                p.g_fast = sc_list_grid(s.r1_lo, s.st.fast.n);
                return REEF_OK;
            }
            p.g_frest = sc_list_grid(s.r1_lo, s.st.frest.n);
            for (uint32_t b = 0; b < 4; ++b) {
                if (s.st.d8[b][0].n) p.g_d8[b] = sc_list_grid(s.r1_lo, s.st.d8[b][0].n);
                p.const_blocks = plan_max(p.const_blocks, ceil_div(s.st.d8[b][1].n, 256));
            }
            p.points_blocks = ceil_div(2 * (uint64_t)s.r1_nq, 256);
        } else if (second) {
            p.route = SC_FC_SECOND;          // hn = an eighth of the pristine rows = half of defer_hq
            p.hq = s.defer_hq;
            p.g_f8 = sc_list_grid(s.r1_lo, s.st.f8.n);
            p.g_gen = sc_list_grid(s.r1_lo, s.st.g8.n);
        } else {
            p.route = SC_FC_R1;
            p.grid = sc_r1_grid(s.r1_lo, p.hn, &p.rows_per_chunk);
        }
        return REEF_OK;
    }
    if (r1) {
        p.route = SC_FC_LAST_R1;
        p.materialize = 1;
        p.fold_blocks = sc_fold_blocks(pow);
        dense_sums(pow / 2);
        return REEF_OK;
    }
    p.materialize = s.r1;
    if (sw.one_launch && pow / 2 <= sw.split_max) {
        p.route = SC_FC_SPLIT;
        p.blocks = sc_split_blocks(pow / 2, sw);
        p.one_launch = 1;
    } else {
        p.route = SC_FC_DENSE;
        dense_sums(pow / 2);
    }
    return REEF_OK;
}

}  // namespace reef
