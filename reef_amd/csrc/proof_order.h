// The call order of the resident proof contexts: which call comes next in the Spartan sum-checks and the batched opening (N5, 3h:
// spartan_engine.inc, open_engine.inc) and in the Hyrax argument (3i: hyrax_engine.inc), and what a call out of order is told.  Host
// code that knows nothing of HIP or common.h: host/proof_order_selftest.cpp walks every phase against every call with plain g++.
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

namespace reef {

enum { SP_NONE = 0, SP_OUTER, SP_OUTER_DONE, SP_INNER, SP_DONE, SP_OPEN_BEGUN, SP_OPEN_FOLDED, SP_OPEN_IPA, SP_OPEN_DONE };
enum { HY_NONE = 0, HY_EVAL, HY_IPA, HY_DONE };

// What a call is told: go on, or REEF_ERR_ARG with `text`; reset: the caller puts the phase back to NONE.  Nothing is formatted for a
// call that is accepted.
struct OrderVerdict {
    bool ok = true, reset = false;
    char text[256];
    OrderVerdict() { text[0] = 0; }
    OrderVerdict &refuse(const char *fmt, ...) __attribute__((format(printf, 2, 3))) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof text, fmt, ap);
        va_end(ap);
        ok = false;
        return *this;
    }
};

// What the order of N5 and 3h depends on; rounds: challenges taken in the current sum-check or IPA, ell_n: log2 of the opening's n
struct SpOrder {
    int phase;
    uint32_t rounds, ell_x, ell_y, ell_n;
};
// The next call of a prove that stands at s.  After inner_claims a prover may open (what an opening call is told) or start over.
inline const char *sp_next(const SpOrder &s, bool opening) {
    switch (s.phase) {
    case SP_OUTER: return s.rounds + 1 < s.ell_x ? "reef_spartan_outer_round" : "reef_spartan_outer_claims";
    case SP_OUTER_DONE: return "reef_spartan_inner_begin";
    case SP_INNER: return s.rounds + 1 < s.ell_y ? "reef_spartan_inner_round" : "reef_spartan_inner_claims";
    case SP_DONE: return opening ? "reef_spartan_open_begin" : "reef_spartan_begin";
    case SP_OPEN_BEGUN: return "reef_spartan_open_fold";
    case SP_OPEN_FOLDED: return "reef_spartan_open_ipa_begin";
    case SP_OPEN_IPA: return s.rounds + 1 < s.ell_n ? "reef_spartan_open_ipa_round" : "reef_spartan_open_finish";
    default: return "reef_spartan_begin";
    }
}
// The call `name` on a ctx whose prove state is s (nullptr: none yet); stale: the matrices or the running instance changed since
// reef_spartan_begin, which voids the prove.  reef_spartan_begin may always come, reef_spartan_open_begin from SP_DONE on (it starts the
// opening over), reef_spartan_open_read from SP_OPEN_FOLDED on and in no order; every other call must be the next one.
inline OrderVerdict sp_check(const char *name, const SpOrder *s, bool stale) {
    OrderVerdict v;
    if (strcmp(name, "reef_spartan_begin") == 0) return v;
    const bool opening = strncmp(name, "reef_spartan_open_", 18) == 0;
    if (strcmp(name, "reef_spartan_open_read") == 0) {
        if (s && !stale && s->phase >= SP_OPEN_FOLDED) return v;
        return v.refuse("reef_spartan_open_read: a and b exist from reef_spartan_open_fold on; the next call is %s",
                        s && !stale ? sp_next(*s, true) : "reef_spartan_begin");
    }
    if (s && s->phase != SP_NONE && stale) {
        v.reset = true;
        return v.refuse("%s: the matrices or the running instance changed (set_matrix, set_running, commit_T or fold) since "
                        "reef_spartan_begin: the next call is reef_spartan_begin", name);
    }
    if (s && s->phase >= SP_DONE && strcmp(name, "reef_spartan_open_begin") == 0) return v;
    const char *want = s ? sp_next(*s, opening) : "reef_spartan_begin";
    return strcmp(want, name) == 0 ? v : v.refuse("%s: out of order, the next call is %s", name, want);
}

// The same for 3i.  reef_hyrax_eval_begin may always come and starts the argument over; eval_comm, eval_comm_compressed, eval_comm_own
// and read need the point it set and nothing else; the IPA calls go in order.  reef_hyrax_commit is in no order and is not asked here.
inline const char *hy_next(int phase, uint32_t rounds, uint32_t right) {
    switch (phase) {
    case HY_EVAL: return "reef_hyrax_ipa_begin";
    case HY_IPA: return rounds + 1 < right ? "reef_hyrax_ipa_round" : "reef_hyrax_finish";
    default: return "reef_hyrax_eval_begin";
    }
}
inline OrderVerdict hy_check(const char *name, int phase, uint32_t rounds, uint32_t right) {
    OrderVerdict v;
    if (strcmp(name, "reef_hyrax_eval_begin") == 0) return v;
    const bool read = strcmp(name, "reef_hyrax_read") == 0;
    if (read || strncmp(name, "reef_hyrax_eval_comm", 20) == 0) {
        if (phase != HY_NONE) return v;
        return read ? v.refuse("%s: a and b exist from reef_hyrax_eval_begin on, the next call", name)
                    : v.refuse("%s: the point is set by reef_hyrax_eval_begin, the next call", name);
    }
    const char *want = hy_next(phase, rounds, right);
    return strcmp(want, name) == 0 ? v : v.refuse("%s: out of order, the next call is %s", name, want);
}

// The same for a batch of arguments in lock-step (3p: hyrax_batch_engine.inc), whose phases are 3i's and whose rounds are the
// challenges the whole batch has taken.  reef_hyrax_batch_eval_begin may always come and starts the batch over; reef_hyrax_batch_read
// needs the vectors it set and nothing else; the IPA calls go in order.
inline const char *hyb_next(int phase, uint32_t rounds, uint32_t right) {
    switch (phase) {
    case HY_EVAL: return "reef_hyrax_batch_ipa_begin";
    case HY_IPA: return rounds + 1 < right ? "reef_hyrax_batch_ipa_round" : "reef_hyrax_batch_finish";
    default: return "reef_hyrax_batch_eval_begin";
    }
}
inline OrderVerdict hyb_check(const char *name, int phase, uint32_t rounds, uint32_t right) {
    OrderVerdict v;
    if (strcmp(name, "reef_hyrax_batch_eval_begin") == 0) return v;
    if (strcmp(name, "reef_hyrax_batch_read") == 0) {
        if (phase != HY_NONE) return v;
        return v.refuse("%s: a and b exist from reef_hyrax_batch_eval_begin on, the next call", name);
    }
    const char *want = hyb_next(phase, rounds, right);
    return strcmp(want, name) == 0 ? v : v.refuse("%s: out of order, the next call is %s", name, want);
}

}  // namespace reef
