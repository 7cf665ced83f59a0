// proof_order_selftest -- the call order of the resident proof contexts (../proof_order.h) against a table written out here: every
// phase of the Spartan sum-checks with the opening, and of the Hyrax argument, against every call name of the family; with the round
// counter at 0, at the last round that still expects a ..._round and one past it; at the smallest sizes with rounds (ell_x 2, ell_y 3,
// n 4, right 2) and at the degenerate ones (ell_x 1, ell_y 1, n 2, right 1), where the first ..._claims or finish follows begin at once;
// each with and without a stale generation, and with no state at all.  Compared: accept or refuse, the full text (it names the next
// call) and the phase-reset flag.  One line; exit 1 on the first mismatch.  Plain g++, no HIP, no library (host/Makefile).
#include <string>

#include "../proof_order.h"

using namespace reef;

#define SP(x) "reef_spartan_" x
#define HY(x) "reef_hyrax_" x

struct Name { const char *name; bool opening; };
static const Name SP_NAMES[] = {{SP("begin"), false},         {SP("outer_round"), false},   {SP("outer_claims"), false}, {SP("inner_begin"), false},
                                {SP("inner_round"), false},   {SP("inner_claims"), false},  {SP("open_begin"), true},    {SP("open_fold"), true},
                                {SP("open_ipa_begin"), true}, {SP("open_ipa_round"), true}, {SP("open_finish"), true},   {SP("open_read"), true}};
static const char *HY_NAMES[] = {HY("eval_begin"), HY("eval_comm"), HY("eval_comm_compressed"), HY("eval_comm_own"), HY("ipa_begin"), HY("ipa_round"), HY("finish"), HY("read")};

// the next call of a prove at {phase, rounds, ell_x, ell_y, log2 n}: for a call of N5, for a call of the opening
struct SpCase { SpOrder s; const char *next, *next_open; };
static const SpCase SP_CASES[] = {
    {{SP_NONE, 0, 2, 3, 2}, SP("begin"), SP("begin")},
    {{SP_OUTER, 0, 2, 3, 2}, SP("outer_round"), SP("outer_round")},
    {{SP_OUTER, 1, 2, 3, 2}, SP("outer_claims"), SP("outer_claims")},
    {{SP_OUTER_DONE, 0, 2, 3, 2}, SP("inner_begin"), SP("inner_begin")},
    {{SP_INNER, 0, 2, 3, 2}, SP("inner_round"), SP("inner_round")},
    {{SP_INNER, 1, 2, 3, 2}, SP("inner_round"), SP("inner_round")},
    {{SP_INNER, 2, 2, 3, 2}, SP("inner_claims"), SP("inner_claims")},
    {{SP_DONE, 2, 2, 3, 2}, SP("begin"), SP("open_begin")},
    {{SP_DONE, 2, 2, 3, 0}, SP("begin"), SP("open_begin")},           // before the first opening: no n yet
    {{SP_OPEN_BEGUN, 0, 2, 3, 2}, SP("open_fold"), SP("open_fold")},
    {{SP_OPEN_FOLDED, 0, 2, 3, 2}, SP("open_ipa_begin"), SP("open_ipa_begin")},
    {{SP_OPEN_IPA, 0, 2, 3, 2}, SP("open_ipa_round"), SP("open_ipa_round")},
    {{SP_OPEN_IPA, 1, 2, 3, 2}, SP("open_finish"), SP("open_finish")},
    {{SP_OPEN_DONE, 1, 2, 3, 2}, SP("begin"), SP("begin")},
    // degenerate: one outer, one inner and one IPA challenge
    {{SP_OUTER, 0, 1, 1, 1}, SP("outer_claims"), SP("outer_claims")},
    {{SP_OUTER, 1, 1, 1, 1}, SP("outer_claims"), SP("outer_claims")},
    {{SP_OUTER_DONE, 0, 1, 1, 1}, SP("inner_begin"), SP("inner_begin")},
    {{SP_INNER, 0, 1, 1, 1}, SP("inner_claims"), SP("inner_claims")},
    {{SP_INNER, 1, 1, 1, 1}, SP("inner_claims"), SP("inner_claims")},
    {{SP_DONE, 0, 1, 1, 1}, SP("begin"), SP("open_begin")},
    {{SP_OPEN_BEGUN, 0, 1, 1, 1}, SP("open_fold"), SP("open_fold")},
    {{SP_OPEN_FOLDED, 0, 1, 1, 1}, SP("open_ipa_begin"), SP("open_ipa_begin")},
    {{SP_OPEN_IPA, 0, 1, 1, 1}, SP("open_finish"), SP("open_finish")},
    {{SP_OPEN_IPA, 1, 1, 1, 1}, SP("open_finish"), SP("open_finish")},
    {{SP_OPEN_DONE, 0, 1, 1, 1}, SP("begin"), SP("begin")},
};
struct HyCase { int phase; uint32_t rounds, right; const char *next; };
static const HyCase HY_CASES[] = {
    {HY_NONE, 0, 2, HY("eval_begin")}, {HY_EVAL, 0, 2, HY("ipa_begin")}, {HY_IPA, 0, 2, HY("ipa_round")}, {HY_IPA, 1, 2, HY("finish")},
    {HY_IPA, 2, 2, HY("finish")},      {HY_DONE, 1, 2, HY("eval_begin")}, {HY_NONE, 0, 1, HY("eval_begin")}, {HY_EVAL, 0, 1, HY("ipa_begin")},
    {HY_IPA, 0, 1, HY("finish")},      {HY_IPA, 1, 1, HY("finish")},     {HY_DONE, 0, 1, HY("eval_begin")},
};

struct Expect { bool ok, reset; std::string text; };
static Expect accept() { return {true, false, ""}; }
static Expect refuse(const std::string &text, bool reset = false) { return {false, reset, text}; }

// the rules of N5 and the opening; k == nullptr: no prove state on the ctx
static Expect sp_rule(const Name &n, const SpCase *k, bool stale) {
    const std::string name = n.name, begin = SP("begin");
    if (name == begin) return accept();
    if (name == SP("open_read")) {
        if (k && !stale && k->s.phase >= SP_OPEN_FOLDED) return accept();
        return refuse(name + ": a and b exist from reef_spartan_open_fold on; the next call is " + (k && !stale ? k->next_open : begin));
    }
    if (k && stale && k->s.phase != SP_NONE)
        return refuse(name + ": the matrices or the running instance changed (set_matrix, set_running, commit_T or fold) since "
                             "reef_spartan_begin: the next call is reef_spartan_begin", true);
    if (name == SP("open_begin") && k && k->s.phase >= SP_DONE) return accept();
    const std::string want = !k ? begin : n.opening ? k->next_open : k->next;
    return want == name ? accept() : refuse(name + ": out of order, the next call is " + want);
}
static Expect hy_rule(const std::string &name, const HyCase &k) {
    if (name == HY("eval_begin")) return accept();
    if (name == HY("eval_comm") || name == HY("eval_comm_compressed") || name == HY("eval_comm_own"))
        return k.phase != HY_NONE ? accept() : refuse(name + ": the point is set by reef_hyrax_eval_begin, the next call");
    if (name == HY("read")) return k.phase != HY_NONE ? accept() : refuse(name + ": a and b exist from reef_hyrax_eval_begin on, the next call");
    return name == k.next ? accept() : refuse(name + ": out of order, the next call is " + k.next);
}

static int checked = 0;
static bool same(const char *what, const OrderVerdict &got, const Expect &want, int phase, unsigned rounds, unsigned ell, int stale) {
    ++checked;
    if (got.ok == want.ok && got.reset == want.reset && want.text == got.text) return true;
    printf("proof_order_selftest: MISMATCH %s at phase %d, rounds %u, size %u, stale %d: got ok %d reset %d \"%s\", want ok %d reset %d \"%s\"\n", what, phase,
           rounds, ell, stale, (int)got.ok, (int)got.reset, got.text, (int)want.ok, (int)want.reset, want.text.c_str());
    return false;
}

int main() {
    for (const Name &n : SP_NAMES) {
        for (int stale = 0; stale < 2; ++stale) {
            if (!same(n.name, sp_check(n.name, nullptr, stale), sp_rule(n, nullptr, stale), -1, 0, 0, stale)) return 1;
            for (const SpCase &k : SP_CASES) {
                if (strcmp(sp_next(k.s, false), k.next) != 0 || strcmp(sp_next(k.s, true), k.next_open) != 0) {
                    printf("proof_order_selftest: MISMATCH sp_next at phase %d, rounds %u: %s / %s, want %s / %s\n", k.s.phase, k.s.rounds, sp_next(k.s, false),
                           sp_next(k.s, true), k.next, k.next_open);
                    return 1;
                }
                if (!same(n.name, sp_check(n.name, &k.s, stale), sp_rule(n, &k, stale), k.s.phase, k.s.rounds, k.s.ell_x, stale)) return 1;
            }
        }
    }
    for (const char *name : HY_NAMES)
        for (const HyCase &k : HY_CASES) {
            if (strcmp(hy_next(k.phase, k.rounds, k.right), k.next) != 0) {
                printf("proof_order_selftest: MISMATCH hy_next at phase %d, rounds %u, right %u: %s, want %s\n", k.phase, k.rounds, k.right,
                       hy_next(k.phase, k.rounds, k.right), k.next);
                return 1;
            }
            if (!same(name, hy_check(name, k.phase, k.rounds, k.right), hy_rule(name, k), k.phase, k.rounds, k.right, 0)) return 1;
        }
    printf("proof_order_selftest: ok, %d calls checked\n", checked);
    return 0;
}
