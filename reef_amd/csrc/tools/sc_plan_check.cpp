// The decisions of the sum-check engine (sumcheck_plan.h) behind a C interface, compiled with g++ -- no HIP, no GPU.
//   g++ -O2 -std=c++17 -shared -fPIC sc_plan_check.cpp -o libreef_scplancheck.so       what tests/test_sc_plan_host.py loads
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -DSC_PLAN_CHECK_MAIN sc_plan_check.cpp -o sc_plan_check
//       the same functions as a program of its own: `sc_plan_check FILE` reads one case per line -- `plan` and the PLAN_IN numbers, `lists`,
//       H and H row flags, `switch` and SW_COUNT words (`-`: unset, `""`: empty) -- and prints what the library's entry points return, so a
//       sanitizer sees every case of the test's grid and the test compares the lines.
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "../sumcheck_plan.h"

using namespace reef;

enum { SW_COUNT = 14, STATE_COUNT = 15, LIST_COUNT = 20, PLAN_IN = 2 + STATE_COUNT + LIST_COUNT + SW_COUNT, PLAN_OUT = 39 };
static const char *const SW_NAMES = "one_launch rank1 structured identity defer r1_min_pow floor_blocks one_launch_max split_max split_blocks items order set_sub blocks_cap";
static const char *const IN_NAMES =
    "call pow len valid_t valid_e nblocks r1 r1_hi r1_hi0 r1_lo r1_nq r1_prev_pow fresh st_ok defer_on defer_pow defer_hq "
    "sum0W sum0S sum0K sum1W sum1S sum1K fast gen f8 f8x frest g8 d8_0S d8_0K d8_1S d8_1K d8_2S d8_2K d8_3S d8_3K";     // then SW_NAMES
static const char *const OUT_NAMES =
    "flush route ident materialize one_launch hn hq blocks fold_blocks grid_x grid_y rows_per_chunk prep_blocks "
    "g_sum0W_x g_sum0W_y g_sum0S_x g_sum0S_y g_sum1W_x g_sum1W_y g_sum1S_x g_sum1S_y g_fast_x g_fast_y g_gen_x g_gen_y g_frest_x g_frest_y "
    "g_d8_0_x g_d8_0_y g_d8_1_x g_d8_1_y g_d8_2_x g_d8_2_y g_d8_3_x g_d8_3_y g_f8_x g_f8_y const_blocks points_blocks";

static ScSwitches switches_from(const int64_t *v) {
    ScSwitches s;
    s.one_launch = v[0] != 0; s.rank1 = v[1] != 0; s.structured = v[2] != 0; s.identity = v[3] != 0; s.defer = v[4] != 0;
    s.r1_min_pow = (uint64_t)v[5]; s.floor_blocks = (uint32_t)v[6]; s.one_launch_max = (uint32_t)v[7]; s.split_max = (uint64_t)v[8];
    s.split_blocks = (uint32_t)v[9]; s.items = (uint32_t)v[10]; s.order = (uint32_t)v[11]; s.set_sub = (uint32_t)v[12]; s.blocks_cap = (uint32_t)v[13];
    return s;
}
static void switches_to(const ScSwitches &s, uint64_t *v) {
    const uint64_t w[] = {s.one_launch, s.rank1, s.structured, s.identity, s.defer, s.r1_min_pow, s.floor_blocks, s.one_launch_max, s.split_max, s.split_blocks,
                          s.items, s.order, s.set_sub, s.blocks_cap};
    static_assert(sizeof w / sizeof w[0] == SW_COUNT, "SW_NAMES lists these");
    for (int i = 0; i < SW_COUNT; ++i) v[i] = w[i];
}
static ScList *list_at(ScRowLists *l, int i) {      // the lists in IN_NAMES order
    ScList *const all[] = {&l->sum[0][0], &l->sum[0][1], &l->sum[0][2], &l->sum[1][0], &l->sum[1][1], &l->sum[1][2], &l->fast, &l->gen, &l->f8, &l->f8x, &l->frest, &l->g8,
                           &l->d8[0][0], &l->d8[0][1], &l->d8[1][0], &l->d8[1][1], &l->d8[2][0], &l->d8[2][1], &l->d8[3][0], &l->d8[3][1]};
    static_assert(sizeof all / sizeof all[0] == LIST_COUNT, "IN_NAMES lists these");
    return all[i];
}

extern "C" {
const char *sc_plan_in_names() { return IN_NAMES; }
const char *sc_plan_switch_names() { return SW_NAMES; }
const char *sc_plan_out_names() { return OUT_NAMES; }
int sc_plan_round(const int64_t *in, uint64_t *out) {
    ScState s;
    const int64_t *v = in + 2;
    s.len = (uint64_t)v[0]; s.valid_t = (uint64_t)v[1]; s.valid_e = (uint64_t)v[2]; s.nblocks = (uint32_t)v[3]; s.r1 = v[4] != 0; s.r1_hi = (uint32_t)v[5];
    s.r1_hi0 = (uint32_t)v[6]; s.r1_lo = (uint32_t)v[7]; s.r1_nq = (uint32_t)v[8]; s.r1_prev_pow = (uint64_t)v[9]; s.fresh = v[10] != 0; s.st_ok = v[11] != 0;
    s.defer_on = v[12] != 0; s.defer_pow = (uint64_t)v[13]; s.defer_hq = (uint32_t)v[14];
    for (int i = 0; i < LIST_COUNT; ++i) list_at(&s.st, i)->n = (uint32_t)v[STATE_COUNT + i];
    ScRoundPlan p;
    memset(&p, 0xA5, sizeof p);                       // whatever the caller's stack held
    const reef_status rs = sc_round_plan((ScCall)in[0], (uint64_t)in[1], s, switches_from(in + 2 + STATE_COUNT + LIST_COUNT), &p);
    const uint64_t w[] = {p.flush, p.route, p.ident, p.materialize, p.one_launch, p.hn, p.hq, p.blocks, p.fold_blocks, p.grid.x, p.grid.y, p.rows_per_chunk, p.prep_blocks,
                          p.g_sum[0][0].x, p.g_sum[0][0].y, p.g_sum[0][1].x, p.g_sum[0][1].y, p.g_sum[1][0].x, p.g_sum[1][0].y, p.g_sum[1][1].x, p.g_sum[1][1].y,
                          p.g_fast.x, p.g_fast.y, p.g_gen.x, p.g_gen.y, p.g_frest.x, p.g_frest.y, p.g_d8[0].x, p.g_d8[0].y, p.g_d8[1].x, p.g_d8[1].y, p.g_d8[2].x, p.g_d8[2].y,
                          p.g_d8[3].x, p.g_d8[3].y, p.g_f8.x, p.g_f8.y, p.const_blocks, p.points_blocks};
    static_assert(sizeof w / sizeof w[0] == PLAN_OUT, "OUT_NAMES lists these");
    for (int i = 0; i < PLAN_OUT; ++i) out[i] = w[i];
    return (int)rs;
}
// text[i]: the variable's value, null: unset -> the switches, in SW_NAMES order
void sc_plan_switches(const char *const *text, uint64_t *out) {
    const ScSwitchText t = {text[0], text[1], text[2], text[3], text[4], text[5], text[6], text[7], text[8], text[9], text[10], text[11], text[12], text[13]};
    switches_to(sc_parse_switches(t), out);
}
// the grid functions and the two table predicates, by name; sw: SW_COUNT numbers.  out: up to three numbers; returns how many
int sc_plan_grid(const char *fn, uint64_t a, uint64_t b, const int64_t *sw_in, uint64_t *out) {
    const std::string f = fn;
    const ScSwitches sw = switches_from(sw_in);
    uint32_t extra = 0;
    if (f == "nblocks") { out[0] = sc_nblocks(a, (uint32_t)b); return 1; }
    if (f == "dense_blocks") { out[0] = sc_dense_blocks(a, (uint32_t)b, sw); return 1; }
    if (f == "one_launch") { out[0] = sc_one_launch((uint32_t)a, sw); return 1; }
    if (f == "split_blocks") { out[0] = sc_split_blocks(a, sw); return 1; }
    if (f == "fold_blocks") { out[0] = sc_fold_blocks(a); return 1; }
    if (f == "r1_prep_blocks") { out[0] = sc_r1_prep_blocks((uint32_t)(a >> 1), a & 1, (uint32_t)b); return 1; }       // a = 2 * r1_hi + folded
    if (f == "r1_grid") { const ScGrid g = sc_r1_grid((uint32_t)a, (uint32_t)b, &extra); out[0] = g.x; out[1] = g.y; out[2] = extra; return 3; }
    if (f == "list_grid") { const ScGrid g = sc_list_grid((uint32_t)a, (uint32_t)b); out[0] = g.x; out[1] = g.y; return 2; }
    if (f == "set_parts") { out[0] = sc_set_parts_blocks(a, sw, &extra); out[1] = extra; return 2; }
    if (f == "struct_rows") { out[0] = sc_struct_rows(a, sw); out[1] = sc_lo_bits(a); return 2; }
    if (f == "eq_rank1") { out[0] = sc_eq_rank1(a, sw); return 1; }
    return 0;
}
// offn: (off, n) of the 20 lists in IN_NAMES order; lists: room for cap words.  Returns the words of the concatenated array (the
// sentinel included), 0: the table gets no structure, -1: cap is too small
long sc_plan_row_lists(const uint32_t *flags, uint32_t H, uint32_t *offn, uint32_t *lists, long cap) {
    ScRowLists l;
    std::vector<uint32_t> words;
    if (!sc_build_row_lists(flags, H, &l, &words)) return 0;
    if ((long)words.size() > cap) return -1;
    for (int i = 0; i < LIST_COUNT; ++i) { offn[2 * i] = list_at(&l, i)->off; offn[2 * i + 1] = list_at(&l, i)->n; }
    for (size_t i = 0; i < words.size(); ++i) lists[i] = words[i];
    return (long)words.size();
}
}

#ifdef SC_PLAN_CHECK_MAIN
static bool read_ints(FILE *f, int64_t *v, int n) {
    for (int i = 0; i < n; ++i) {
        long long x;
        if (fscanf(f, "%lld", &x) != 1) return false;
        v[i] = x;
    }
    return true;
}
int main(int argc, char **argv) {
    FILE *f = argc > 1 ? fopen(argv[1], "r") : nullptr;
    if (!f) { fprintf(stderr, "usage: sc_plan_check FILE   (lines: plan + %d integers | lists H + H flags | switch + %d words)\n", PLAN_IN, SW_COUNT); return 2; }
    long cases = 0;
    char kind[16];
    while (fscanf(f, "%15s", kind) == 1) {
        const std::string k = kind;
        if (k == "plan") {
            int64_t in[PLAN_IN];
            uint64_t out[PLAN_OUT];
            if (!read_ints(f, in, PLAN_IN)) { fprintf(stderr, "case %ld: short plan line\n", cases); return 2; }
            printf("%d", sc_plan_round(in, out));
            for (int i = 0; i < PLAN_OUT; ++i) printf(" %llu", (unsigned long long)out[i]);
        } else if (k == "lists") {
            int64_t H;
            if (!read_ints(f, &H, 1) || H < 0 || H > (1 << 20)) { fprintf(stderr, "case %ld: bad H\n", cases); return 2; }
            std::vector<int64_t> fl((size_t)H);
            if (!read_ints(f, fl.data(), (int)H)) { fprintf(stderr, "case %ld: short lists line\n", cases); return 2; }
            std::vector<uint32_t> flags(fl.begin(), fl.end()), words(20 * (size_t)H + 1);
            uint32_t offn[40] = {};
            const long n = sc_plan_row_lists(flags.data(), (uint32_t)H, offn, words.data(), (long)words.size());
            printf("%ld", n);
            if (n > 0) {
                for (int i = 0; i < 40; ++i) printf(" %u", offn[i]);
                for (long i = 0; i < n; ++i) printf(" %u", words[(size_t)i]);
            }
        } else if (k == "switch") {
            std::string word[SW_COUNT];
            const char *text[SW_COUNT];
            char buf[64];
            for (int i = 0; i < SW_COUNT; ++i) {
                if (fscanf(f, "%63s", buf) != 1) { fprintf(stderr, "case %ld: short switch line\n", cases); return 2; }
                word[i] = buf;
                text[i] = word[i] == "-" ? nullptr : word[i] == "\"\"" ? "" : word[i].c_str();
            }
            uint64_t out[SW_COUNT];
            sc_plan_switches(text, out);
            printf("0");
            for (int i = 0; i < SW_COUNT; ++i) printf(" %llu", (unsigned long long)out[i]);
        } else { fprintf(stderr, "case %ld: unknown kind %s\n", cases, kind); return 2; }
        printf("\n");
        ++cases;
    }
    fclose(f);
    fprintf(stderr, "sc_plan_check: %ld cases\n", cases);
    return 0;
}
#endif
