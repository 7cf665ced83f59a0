// hyrax_batch_order_selftest -- the call order of a batch of Hyrax arguments in lock-step (../proof_order.h: hyb_check, hyb_next)
// against a table written out here: every phase against every call of the family, with the round counter at 0, at the last round that
// still expects a ..._round and one past it, at right 3 and 2 and at the degenerate right 1, where finish follows ipa_begin at once.
// Compared: accept or refuse, the full text (it names the next call) and the reset flag (never set).  One line; exit 1 on the first
// mismatch.  With the argument "dump": one line "phase rounds right name -> ok | the text" for every phase, rounds 0 .. 3 and right
// 1 .. 3, for a table kept elsewhere (tests/test_hyrax_batch_host.py).  Plain g++, no HIP, no library (host/Makefile).
#include <string>

#include "../proof_order.h"

using namespace reef;

#define HB(x) "reef_hyrax_batch_" x

static const char *NAMES[] = {HB("eval_begin"), HB("ipa_begin"), HB("ipa_round"), HB("finish"), HB("read")};

struct Case { int phase; uint32_t rounds, right; const char *next; };
static const Case CASES[] = {
    {HY_NONE, 0, 3, HB("eval_begin")}, {HY_EVAL, 0, 3, HB("ipa_begin")},  {HY_IPA, 0, 3, HB("ipa_round")},  {HY_IPA, 1, 3, HB("ipa_round")},
    {HY_IPA, 2, 3, HB("finish")},      {HY_IPA, 3, 3, HB("finish")},      {HY_DONE, 2, 3, HB("eval_begin")}, {HY_NONE, 0, 2, HB("eval_begin")},
    {HY_EVAL, 0, 2, HB("ipa_begin")},  {HY_IPA, 0, 2, HB("ipa_round")},   {HY_IPA, 1, 2, HB("finish")},      {HY_IPA, 2, 2, HB("finish")},
    {HY_DONE, 1, 2, HB("eval_begin")}, {HY_NONE, 0, 1, HB("eval_begin")}, {HY_EVAL, 0, 1, HB("ipa_begin")},  {HY_IPA, 0, 1, HB("finish")},
    {HY_IPA, 1, 1, HB("finish")},      {HY_DONE, 0, 1, HB("eval_begin")},
};

struct Expect { bool ok; std::string text; };
static Expect rule(const std::string &name, const Case &k) {
    if (name == HB("eval_begin")) return {true, ""};
    if (name == HB("read")) {
        if (k.phase != HY_NONE) return {true, ""};
        return {false, name + ": a and b exist from reef_hyrax_batch_eval_begin on, the next call"};
    }
    if (name == k.next) return {true, ""};
    return {false, name + ": out of order, the next call is " + k.next};
}

int main(int argc, char **argv) {
    if (argc > 1 && strcmp(argv[1], "dump") == 0) {
        for (int phase = HY_NONE; phase <= HY_DONE; ++phase)
            for (uint32_t rounds = 0; rounds <= 3; ++rounds)
                for (uint32_t right = 1; right <= 3; ++right)
                    for (const char *name : NAMES) {
                        const OrderVerdict v = hyb_check(name, phase, rounds, right);
                        printf("%d %u %u %s -> %s\n", phase, rounds, right, name, v.ok ? "ok" : v.text);
                    }
        return 0;
    }
    if (argc > 1) {
        printf("usage: hyrax_batch_order_selftest [dump]\n");
        return 2;
    }
    int checked = 0;
    for (const char *name : NAMES)
        for (const Case &k : CASES) {
            if (strcmp(hyb_next(k.phase, k.rounds, k.right), k.next) != 0) {
                printf("hyrax_batch_order_selftest: MISMATCH hyb_next at phase %d, rounds %u, right %u: %s, want %s\n", k.phase, k.rounds, k.right,
                       hyb_next(k.phase, k.rounds, k.right), k.next);
                return 1;
            }
            const OrderVerdict got = hyb_check(name, k.phase, k.rounds, k.right);
            const Expect want = rule(name, k);
            ++checked;
            if (got.ok != want.ok || got.reset || want.text != got.text) {
                printf("hyrax_batch_order_selftest: MISMATCH %s at phase %d, rounds %u, right %u: got ok %d reset %d \"%s\", want ok %d \"%s\"\n", name,
                       k.phase, k.rounds, k.right, (int)got.ok, (int)got.reset, got.text, (int)want.ok, want.text.c_str());
                return 1;
            }
        }
    printf("hyrax_batch_order_selftest: ok, %d calls checked\n", checked);
    return 0;
}
