// The launch plan of the bucket pipeline (msm_plan.h: core_launch_plan) behind a C interface, compiled with g++ -- no HIP, no GPU.
//   g++ -O2 -std=c++17 -shared -fPIC plan_check.cpp -o libreef_plancheck.so       what tests/test_core_plan_host.py loads
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DPLAN_CHECK_MAIN plan_check.cpp -o plan_check
//       the same function as a program of its own: `plan_check FILE` reads one case per line (the PLAN_IN numbers) and prints the
//       status and the PLAN_OUT numbers of each, so a sanitizer sees every plan of the test's grid and the test compares the lines.
#include <stdio.h>
#include <stdlib.h>

#include "../msm_plan.h"

using namespace reef;

enum { PLAN_IN = 19, PLAN_OUT = 62 };
static const char *const OUT_NAMES =
    "N Mmax entries_padded NB NBT groups_total L0 nchunks0 row_mode two_level shift compact word_entries NBc NBTc KB P S per rows_per_block "
    "keys_per_row recode_fused scan ntiles nseg_max fine merge_fused merge_first merge_first_grid merge_cur merge_nlevels merge_len0 merge_len1 "
    "merge_len2 merge_len3 merge_len4 merge_len5 merge_len6 merge_len7 c1 c2 rc_waves direct rowcol_lanes skip_reduce "
    "b_dig b_counts b_tile_sums b_bstart b_entries b_bstart1 b_seg_first b_seg_counts b_entries1 b_bucket_acc b_lkeys0 b_lkeys1 b_lvals0 b_lvals1 "
    "b_rowcol b_group_sums b_wsum";

// in: c W G rows row_len n_ctx slice_sort | L0 coop two_level rowcol_lanes group_sums_out | fuse_merge merge1 fuse_max_chunks fuse_recode
// sort_compact sort_word skip_reduce.  Returns the status; *why is the error's text or null.
static reef_status fill(const int64_t *in, CoreLaunch *p, const char **why) {
    CorePlan pl{(uint32_t)in[0], (uint32_t)in[1], (uint32_t)in[2], (uint32_t)in[3], (uint32_t)in[4], (uint32_t)in[5], in[6] != 0};
    CoreCtxOpts o{(uint32_t)in[7], in[8] != 0, (int)in[9], (int)in[10], in[11] != 0};
    CoreSwitches sw;
    sw.fuse_merge = in[12] != 0; sw.merge1 = in[13] != 0; sw.fuse_max_chunks = (uint32_t)in[14]; sw.fuse_recode = in[15] != 0;
    sw.sort_compact = in[16] != 0; sw.sort_word = in[17] != 0; sw.skip_reduce = (int)in[18];
    memset(p, 0xA5, sizeof *p);                       // whatever the caller's stack held
    *why = nullptr;
    return core_launch_plan(pl, o, sw, p, why);
}
static int plan(const int64_t *in, uint64_t *out, const char **why) {
    CoreLaunch p;
    const reef_status rs = fill(in, &p, why);
    const MergePlan &m = p.merge;
    const CoreBytes &b = p.bytes;
    const uint64_t v[] = {p.N, p.Mmax, p.entries_padded, p.NB, p.NBT, p.groups_total, p.L0, p.nchunks0, p.row_mode, p.two_level, p.shift, p.compact, p.word_entries,
                          p.NBc, p.NBTc, p.KB, p.P, p.S, p.per, p.rows_per_block, p.keys_per_row, p.recode_fused, p.scan, p.ntiles, p.nseg_max, p.fine,
                          m.fused, m.first, m.first_grid, m.cur, m.nlevels, m.len[0], m.len[1], m.len[2], m.len[3], m.len[4], m.len[5], m.len[6], m.len[7],
                          p.c1, p.c2, p.rc_waves, p.direct, (uint64_t)(int64_t)p.rowcol_lanes, (uint64_t)(int64_t)p.skip_reduce,
                          b.dig, b.counts, b.tile_sums, b.bstart, b.entries, b.bstart1, b.seg_first, b.seg_counts, b.entries1, b.bucket_acc, b.lkeys[0], b.lkeys[1],
                          b.lvals[0], b.lvals[1], b.rowcol, b.group_sums, b.wsum};
    static_assert(sizeof v / sizeof v[0] == PLAN_OUT, "OUT_NAMES lists these");
    static_assert(MERGE_MAX_LEVELS == 8, "merge_len0 .. merge_len7");
    for (int i = 0; i < PLAN_OUT; ++i) out[i] = v[i];
    return (int)rs;
}

extern "C" {
int plan_core(const int64_t *in, uint64_t *out, const char **why) { return plan(in, out, why); }
const char *plan_out_names() { return OUT_NAMES; }
int plan_in_count() { return PLAN_IN; }
// the constants of msm_plan.h, for the test's own arithmetic
void plan_constants(uint64_t *out) {
    const uint64_t v[] = {SCAN_TILE, SCAN_SMALL_SLICES, SORT_SEG, MAX_LDS_KEYS, MAX_SCAN_KEYS, SORT_SHIFT, TWO_LEVEL_MIN_ENTRIES, XYZZ_BYTES, ENTRY_BYTES,
                          ROWCOL_SHARED_MIN_BUCKETS, (uint64_t)ROWCOL_SHARED_LANES};
    for (size_t i = 0; i < sizeof v / sizeof v[0]; ++i) out[i] = v[i];
}
// are two plans the same chain (what run_core_graphed keys a captured graph on)?
int plan_same(const int64_t *a, const int64_t *b) {
    CoreLaunch pa, pb;
    const char *why;
    if (fill(a, &pa, &why) != REEF_OK || fill(b, &pb, &why) != REEF_OK) return -1;
    return same_plan(pa, pb) ? 1 : 0;
}
}

#ifdef PLAN_CHECK_MAIN
int main(int argc, char **argv) {
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) { fprintf(stderr, "usage: plan_check FILE   (one case per line: %d integers)\n", PLAN_IN); return 2; }
    long cases = 0;
    for (;;) {
        int64_t in[PLAN_IN];
        int got = 0;
        for (; got < PLAN_IN; ++got) {
            long long x;
            if (fscanf(f, "%lld", &x) != 1) break;
            in[got] = x;
        }
        if (got == 0) break;
        if (got != PLAN_IN) { fprintf(stderr, "case %ld: %d of %d numbers\n", cases, got, PLAN_IN); return 2; }
        uint64_t out[PLAN_OUT];
        const char *why;
        const int rs = plan(in, out, &why);
        printf("%d", rs);
        if (rs == 0) for (int i = 0; i < PLAN_OUT; ++i) printf(" %llu", (unsigned long long)out[i]);
        printf("\n");
        ++cases;
    }
    fclose(f);
    fprintf(stderr, "plan_check: %ld cases\n", cases);
    return 0;
}
#endif
