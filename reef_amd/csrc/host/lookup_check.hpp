// lookup_check.hpp -- the verifier of the replay's lookup leg (`reef_replay cfgN lookup`, replay_lookup.hpp): the nlookup sum-check a
// folding step runs (wit_nlookup_gadget, r1cs.rs:2177-2393), the running claim from step to step, and the claim it hands to the
// consistency argument (framework.rs:629-639, 708-721; commitment.rs:241-244, 305-345).  Host only, on proof_check.hpp's Mod, eq_evals
// and StandinTranscript: lookup_check_selftest.cpp builds from it with plain g++ and no library.
//
// Conventions, the reference's: a point is written most significant variable first -- sc_rs in round order (round i folds index bit
// ell - i, linear_mle_product r1cs_helper.rs:441-506), prev_running_q as the step before left it, T~(r) = sum_i T[i] prod_m
// [bit_{ell-m}(i) ? r_m : 1 - r_m] (prover_mle_partial_eval / verifier_mle_eval, r1cs_helper.rs:551-641; the KAT at r1cs.rs:2701-2723).
// gen_eq_table (r1cs_helper.rs:508-544) is handed prev_running_q REVERSED (r1cs.rs:2319), which makes its weight of index i the same
// product over p = prev_running_q.  Values are reef_fe in Montgomery form throughout, as in proof_check.hpp.
#pragma once
#include "proof_check.hpp"

static reef_fe from_m(const Mod &m, const reef_fe &a) { return fmul(m, a, reef_fe{{1, 0, 0, 0}}); }
static std::string fe_hex(const Mod &m, const reef_fe &a) {      // the canonical integer, for the JSON lines
    const reef_fe c = from_m(m, a);
    char b[80];
    snprintf(b, sizeof b, "\"0x%016llx%016llx%016llx%016llx\"", (unsigned long long)c.l[3], (unsigned long long)c.l[2], (unsigned long long)c.l[1], (unsigned long long)c.l[0]);
    return b;
}
// prod_m [bit_{k-1-m}(i) ? t_m : 1 - t_m], m = 0 .. k-1: eq_evals(t, k)[i] without the table
static reef_fe eq_index(const Mod &m, const reef_fe *t, size_t k, uint64_t i) {
    reef_fe w = m.one;
    for (size_t j = 0; j < k; ++j) w = fmul(m, w, ((i >> (k - 1 - j)) & 1) ? t[j] : fsub(m, m.one, t[j]));
    return w;
}

// What the harness knows T to be -- "nldoc": the document's symbols, zero beyond them; "nlhybrid": [pub, fill x (half - |pub|)] in the
// lower half, the document's symbols in the upper -- and its own restatement of the symbols where the table is small enough to hold them.
struct LookupTable {
    size_t ell = 0;
    bool hybrid = false;
    std::vector<reef_fe> pub;                 // hybrid: the transition table
    reef_fe fill = {};
    bool have_doc = false;                    // doc holds the host's restatement of the document part's symbols (zero beyond them)
    bool eval_on_host = false;                // ... and T~ is evaluated from it (the "host" route); else the step's doc_eval is taken (the "n3" route)
    std::vector<uint32_t> doc;
    size_t doc_vars() const { return hybrid ? ell - 1 : ell; }
};
struct LookupStep {
    std::vector<uint64_t> qs;
    std::vector<reef_fe> vs, prev_q, sc_rs;
    reef_fe prev_v = {}, claim_r = {}, next_v = {};
    std::vector<std::array<reef_fe, 3>> g;    // per round (xsq, x, con)
    reef_fe doc_eval = {};                    // the "n3" route: doc~ at the step's point from reef_mle_bound_rows (unused on the host route)
};
struct LookupRecord {
    LookupTable tbl;
    reef_fe doc_hash = {};                    // stands in for self.doc_hash, the first element a step absorbs (r1cs.rs:2287-2288)
    std::vector<LookupStep> steps;
};
struct LookupCounts { size_t rounds = 0, values = 0; };

// T[i] from the host's restatement (have_doc)
static reef_fe table_entry(const Mod &m, const LookupTable &t, uint64_t i) {
    const uint64_t half = (uint64_t)1 << (t.ell - 1);
    if (t.hybrid && i < half) return i < t.pub.size() ? t.pub[i] : t.fill;
    const uint64_t d = t.hybrid ? i - half : i;
    return d < t.doc.size() ? fsmall(m, t.doc[d]) : reef_fe{};
}
// the public half at a point over its own ell - 1 variables, closed form: sum_{i < |pub|} pub[i] eq_i + fill (1 - sum_{i < |pub|} eq_i)
// (the eq-mass of a whole half is one)
static reef_fe pub_eval(const Mod &m, const LookupTable &t, const reef_fe *point) {
    reef_fe s = {}, mass = {};
    for (size_t i = 0; i < t.pub.size(); ++i) {
        const reef_fe w = eq_index(m, point, t.ell - 1, i);
        s = fadd(m, s, fmul(m, t.pub[i], w));
        mass = fadd(m, mass, w);
    }
    return fadd(m, s, fmul(m, t.fill, fsub(m, m.one, mass)));
}
static reef_fe doc_eval_host(const Mod &m, const LookupTable &t, const reef_fe *point) {
    const std::vector<reef_fe> e = eq_evals(m, point, t.doc_vars());
    reef_fe s = {};
    for (size_t i = 0; i < t.doc.size(); ++i)
        if (t.doc[i]) s = fadd(m, s, fmul(m, fsmall(m, t.doc[i]), e[i]));
    return s;
}
// T~(r), r over all ell variables; doc_at: the document part at its own point (the last doc_vars entries of r)
static reef_fe table_eval(const Mod &m, const LookupTable &t, const reef_fe *r, const reef_fe &doc_at) {
    if (!t.hybrid) return doc_at;
    return fadd(m, fmul(m, fsub(m, m.one, r[0]), pub_eval(m, t, r + 1)), fmul(m, r[0], doc_at));
}

// What a step absorbs before claim_r, in the reference's order (r1cs.rs:2285-2306): doc_hash, the combined q's, the v's, prev_running_q,
// prev_running_v.  The q's go in as the 64-bit indices (the reference packs their bits into field elements: the same information).
static const uint64_t LOOKUP_DOMAIN = 0x4C4F4F4B;
static reef_fe lookup_claim_r(StandinTranscript &T, const reef_fe &doc_hash, const LookupStep &st) {
    T.absorb("doc_hash", &doc_hash, sizeof doc_hash);
    T.absorb("combined_q", st.qs.data(), st.qs.size() * sizeof(uint64_t));
    T.absorb("v", st.vs.data(), st.vs.size() * sizeof(reef_fe));
    T.absorb("running_q", st.prev_q.data(), st.prev_q.size() * sizeof(reef_fe));
    T.absorb("running_v", &st.prev_v, sizeof st.prev_v);
    return T.squeeze();
}
static reef_fe lookup_round_r(StandinTranscript &T, const std::array<reef_fe, 3> &g) {      // absorb (con, x, xsq): r1cs_helper.rs:478-482
    const reef_fe q[3] = {g[2], g[1], g[0]};
    T.absorb("g", q, sizeof q);
    return T.squeeze();
}
static std::vector<reef_fe> lookup_rs(const Mod &m, const reef_fe &claim_r, size_t nq) {   // rs[i] = claim_r^(i+1), nq + 1 of them
    std::vector<reef_fe> rs(1, claim_r);
    for (size_t i = 1; i <= nq; ++i) rs.push_back(fmul(m, rs.back(), claim_r));
    return rs;
}

// Phase `lookup`: every step's sum-check with the verifier's equations, its challenges re-derived, T~(r) recomputed without reef_sc_*, the
// looked-up values against the host's restatement, and the running claim from step to step.
static LookupCounts check_lookup(const Mod &m, const LookupRecord &rec) {
    const char *ph = "lookup";
    const LookupTable &t = rec.tbl;
    const size_t ell = t.ell;
    LookupCounts n;
    for (size_t s = 0; s < rec.steps.size(); ++s) {
        const LookupStep &st = rec.steps[s];
        const std::string sn = "step " + std::to_string(s);
        const size_t nq = st.qs.size();
        EXPECT(ph, st.vs.size() == nq && st.prev_q.size() == ell && st.sc_rs.size() == ell && st.g.size() == ell, sn + ": sizes of the recorded step");
        if (s == 0) {
            for (const reef_fe &p : st.prev_q) EXPECT(ph, feq(p, reef_fe{}), sn + ": the first running q is not 0..0 (r1cs.rs:2194-2197)");
            if (t.have_doc || t.hybrid) EXPECT(ph, feq(st.prev_v, table_entry(m, t, 0)), sn + ": the first running v is not T[0] (r1cs.rs:2198-2201)");
        } else {
            const LookupStep &b = rec.steps[s - 1];
            EXPECT(ph, memcmp(st.prev_q.data(), b.sc_rs.data(), ell * sizeof(reef_fe)) == 0 && feq(st.prev_v, b.next_v),
                   sn + ": its previous running claim is not the next running claim of the step before");
        }
        for (size_t k = 0; k < nq; ++k) {
            EXPECT(ph, st.qs[k] >> ell == 0, sn + ": lookup index past the table");
            if (t.have_doc) {
                EXPECT(ph, feq(st.vs[k], table_entry(m, t, st.qs[k])), sn + ": v_" + std::to_string(k) + " differs from the host's T[" + std::to_string(st.qs[k]) + "]");
                ++n.values;
            }
        }
        StandinTranscript T(m, LOOKUP_DOMAIN + s);
        EXPECT(ph, feq(lookup_claim_r(T, rec.doc_hash, st), st.claim_r), sn + ": claim_r is not the transcript's challenge for what was absorbed");
        const std::vector<reef_fe> rs = lookup_rs(m, st.claim_r, nq);
        reef_fe c = fmul(m, rs[nq], st.prev_v);
        for (size_t k = 0; k < nq; ++k) c = fadd(m, c, fmul(m, rs[k], st.vs[k]));
        for (size_t i = 0; i < ell; ++i) {
            const reef_fe &xsq = st.g[i][0], &x = st.g[i][1], &con = st.g[i][2];
            const std::string rn = sn + " round " + std::to_string(i + 1);
            EXPECT(ph, feq(fadd(m, fadd(m, con, con), fadd(m, x, xsq)), c), rn + ": 2 con + x + xsq differs from the claim");
            const reef_fe r = lookup_round_r(T, st.g[i]);
            EXPECT(ph, feq(r, st.sc_rs[i]), rn + ": sc_r is not the transcript's challenge for (con, x, xsq)");
            c = fadd(m, fmul(m, fadd(m, fmul(m, xsq, r), x), r), con);
            ++n.rounds;
        }
        const reef_fe *r = st.sc_rs.data();
        const reef_fe doc_at = t.have_doc && t.eval_on_host ? doc_eval_host(m, t, r + (ell - t.doc_vars())) : st.doc_eval;
        EXPECT(ph, feq(st.next_v, table_eval(m, t, r, doc_at)), sn + ": next_running_v differs from T~(sc_rs) evaluated outside the sum-check rows");
        reef_fe e = fmul(m, rs[nq], eq_at(m, st.sc_rs, st.prev_q));
        for (size_t k = 0; k < nq; ++k) e = fadd(m, e, fmul(m, rs[k], eq_index(m, r, ell, st.qs[k])));
        EXPECT(ph, feq(c, fmul(m, st.next_v, e)), sn + ": the last claim differs from next_running_v * eq~(sc_rs)");
    }
    return n;
}

// Phase `claim`: the evaluation the consistency argument proves is the last running claim.  q = the last sc_rs.  doc / proj: eval itself;
// hybrid: (1 - q0) t + q0 eval with t the public half at q[1..] (commitment.rs:237-244).
static void check_claim(const Mod &m, const LookupRecord &rec, const reef_fe &eval) {
    const char *ph = "claim";
    EXPECT(ph, !rec.steps.empty(), "no step recorded");
    const LookupStep &last = rec.steps.back();
    if (!rec.tbl.hybrid) {
        EXPECT(ph, feq(eval, last.next_v), "the evaluation handed to the consistency argument differs from the last next_running_v");
        return;
    }
    const reef_fe q0 = last.sc_rs[0], t = pub_eval(m, rec.tbl, last.sc_rs.data() + 1);
    EXPECT(ph, feq(fadd(m, fmul(m, fsub(m, m.one, q0), t), fmul(m, q0, eval)), last.next_v), "(1 - q0) t + q0 v' differs from the last next_running_v");
}

static const char *const LOOKUP_TAMPER_PHASES[] = {"lookup", "claim", "hyrax"};
static void check_lookup_tamper_name(const std::string &t) {
    if (t.empty()) return;
    for (const char *p : LOOKUP_TAMPER_PHASES)
        if (t == p) return;
    fail("tamper=" + t + ": one of lookup, claim, hyrax");
}
// one recorded value per phase: a round coefficient, the value handed over, a_hat
template <class Hf> static void apply_lookup_tamper(const Mod &m, const std::string &t, LookupRecord &rec, reef_fe &handed, Hf &hf) {
    if (t == "lookup") rec.steps[rec.steps.size() / 2].g[1][1] = fadd(m, rec.steps[rec.steps.size() / 2].g[1][1], m.one);
    else if (t == "claim") handed = fadd(m, handed, m.one);
    else if (t == "hyrax") hf.a_hat = fadd(m, hf.a_hat, m.one);
}

// ---- the host-only self-test: a tiny honest transcript made with plain loops, printed, and run through the checks ----------------------
// one honest step on the written-out table: the reference's loops (gen_eq_table, linear_mle_product) on Montgomery values
static void lookup_honest_step(const Mod &m, const std::vector<reef_fe> &table, const reef_fe &doc_hash, size_t s, LookupStep &st) {
    size_t ell = 0;
    while (((size_t)1 << ell) < table.size()) ++ell;
    const size_t nq = st.qs.size();
    st.vs.clear();
    for (uint64_t q : st.qs) st.vs.push_back(table[q]);
    StandinTranscript T(m, LOOKUP_DOMAIN + s);
    st.claim_r = lookup_claim_r(T, doc_hash, st);
    const std::vector<reef_fe> rs = lookup_rs(m, st.claim_r, nq);
    std::vector<reef_fe> t = table, e(table.size());
    for (size_t i = 0; i < table.size(); ++i) {              // last_q = prev_q reversed: last_q[j] pairs with index bit j
        reef_fe term = rs[nq];
        for (size_t j = 0; j < ell; ++j) {
            const reef_fe &lq = st.prev_q[ell - 1 - j];
            term = fmul(m, term, ((i >> j) & 1) ? lq : fsub(m, m.one, lq));
        }
        e[i] = term;
    }
    for (size_t k = 0; k < nq; ++k) e[st.qs[k]] = fadd(m, e[st.qs[k]], rs[k]);
    st.g.clear();
    st.sc_rs.clear();
    for (size_t i = 1; i <= ell; ++i) {
        const size_t pow = (size_t)1 << (ell - i);
        reef_fe xsq = {}, x = {}, con = {};
        for (size_t b = 0; b < pow; ++b) {
            const reef_fe ts = fsub(m, t[b + pow], t[b]), es = fsub(m, e[b + pow], e[b]);
            xsq = fadd(m, xsq, fmul(m, ts, es));
            x = fadd(m, x, fadd(m, fmul(m, es, t[b]), fmul(m, ts, e[b])));
            con = fadd(m, con, fmul(m, t[b], e[b]));
        }
        st.g.push_back({xsq, x, con});
        const reef_fe r = lookup_round_r(T, st.g.back());
        st.sc_rs.push_back(r);
        for (size_t b = 0; b < pow; ++b) {
            t[b] = fadd(m, t[b], fmul(m, r, fsub(m, t[b + pow], t[b])));
            e[b] = fadd(m, e[b], fmul(m, r, fsub(m, e[b + pow], e[b])));
        }
    }
    st.next_v = t[0];
}
// the honest Hyrax argument over `doc` (8-bit symbols, zero-padded to 2^num_vars) at `point`, in discrete-logarithm form
template <class Hf> static void hyrax_honest(const Mod &m, const std::vector<uint8_t> &doc, size_t num_vars, size_t left, const std::vector<reef_fe> &point,
                                             const std::vector<reef_fe> &g, const std::vector<reef_fe> &blinds, const reef_fe &hd, const reef_fe &g1,
                                             const reef_provider::Transcript &tr, Hf &hf) {
    const size_t cols = (size_t)1 << (num_vars - left);
    const std::vector<reef_fe> L = eq_evals(m, point.data(), left), Rv = eq_evals(m, point.data() + left, num_vars - left);
    const std::vector<reef_fe> lz = host_lz(m, doc, cols, L);
    hf.eval = dot(m, lz.data(), Rv.data(), cols);
    hf.lz_blind = dot(m, L.data(), blinds.data(), L.size());
    const reef_fe u[2] = {fadd(m, dot(m, lz.data(), g.data(), cols), fmul(m, hf.lz_blind, hd)), hf.eval};
    hf.r_q = tr("r", u, sizeof u);
    const IpaTrace t = ipa_honest(m, lz, Rv, g, fmul(m, g1, hf.r_q), [&](size_t, const reef_fe &l, const reef_fe &r) {
        const reef_fe lr[2] = {l, r};
        return tr("challenge_r", lr, sizeof lr);
    });
    hf.r_rounds = t.rs;
    hf.a_hat = t.a_hat;
    hf.b_hat = t.b_hat;
}
static std::string json_list(const Mod &m, const std::vector<reef_fe> &v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + fe_hex(m, v[i]);
    return s + "]";
}

// ell = 4, 3 steps, 3 lookups; mode doc (13 symbols, zero beyond) and mode hybrid (public half [3 values, fill x 5], 6 symbols in the
// document half).  Returns the JSON line: both transcripts in full, canonical integers as hex strings, for a reader to recompute.
static std::string lookup_selftest(const std::string &tamper) {
    using Hf = reef_provider::HyraxEval<REEF_PALLAS>::Proof;
    check_lookup_tamper_name(tamper);
    const Mod m(ORDER[0]);
    const size_t ell = 4, n = (size_t)1 << ell, steps = 3;
    std::string line = "{\"selftest\": \"accepted\", \"ell\": 4, \"steps\": 3, \"lookups\": 3, \"tamper\": \"" + tamper + "\", \"modes\": {";
    size_t rounds = 0, values = 0;
    for (int hybrid = 0; hybrid < 2; ++hybrid) {
        LookupRecord rec;
        LookupTable &t = rec.tbl;
        t.ell = ell;
        t.hybrid = hybrid != 0;
        t.have_doc = t.eval_on_host = true;
        Rng rng{0x100Cu + (uint64_t)hybrid};
        const size_t ndoc = hybrid ? 6 : 13;
        for (size_t i = 0; i < ndoc; ++i) t.doc.push_back((uint32_t)((i * 37 + 11) % 131));
        if (hybrid) {
            for (int i = 0; i < 3; ++i) t.pub.push_back(rng.full(m));
            t.fill = rng.full(m);
        }
        rec.doc_hash = fsmall(m, 0xD0C);
        std::vector<reef_fe> table(n);
        for (size_t i = 0; i < n; ++i) table[i] = table_entry(m, t, i);
        // index 0, the last live entry, the zero padding, both sides of every part boundary, a repeated index
        const std::vector<std::vector<uint64_t>> qs = hybrid ? std::vector<std::vector<uint64_t>>{{0, 2, 3}, {7, 8, 13}, {14, 8, 8}}
                                                             : std::vector<std::vector<uint64_t>>{{0, 12, 13}, {15, 5, 5}, {12, 1, 0}};
        for (size_t s = 0; s < steps; ++s) {
            LookupStep st;
            st.qs = qs[s];
            st.prev_q = s ? rec.steps[s - 1].sc_rs : std::vector<reef_fe>(ell);
            st.prev_v = s ? rec.steps[s - 1].next_v : table[0];
            lookup_honest_step(m, table, rec.doc_hash, s, st);
            rec.steps.push_back(st);
        }
        // the hand-over (commitment.rs:305-316): doc: q; hybrid: the last q_len entries, t on the public half
        const std::vector<reef_fe> &q = rec.steps.back().sc_rs;
        const size_t hv = t.doc_vars(), left = hv / 2;
        const std::vector<reef_fe> point(q.end() - hv, q.end());
        std::vector<uint8_t> doc8(t.doc.begin(), t.doc.end());
        std::vector<reef_fe> hg((size_t)1 << (hv - left)), blinds((size_t)1 << left);
        for (size_t i = 0; i < hg.size(); ++i) hg[i] = fsmall(m, 0xFEED + 3 * i);
        for (size_t i = 0; i < blinds.size(); ++i) blinds[i] = fsmall(m, 1000003 * (i + 1));
        const reef_fe hd = fsmall(m, 0xB11D), g1 = fsmall(m, 0x6E1);
        StandinTranscript HT(m, 2);
        Hf hf;
        hyrax_honest(m, doc8, hv, left, point, hg, blinds, hd, g1, HT.fn(), hf);
        reef_fe handed = hf.eval;
        if (!hybrid) apply_lookup_tamper(m, tamper, rec, handed, hf);      // the tampered value sits in mode doc: mode hybrid then is not reached
        const LookupCounts c = check_lookup(m, rec);
        check_claim(m, rec, handed);
        check_hyrax(m, doc8, hv, left, point, hf, hg, blinds, hd, g1, PointCheck());
        rounds += c.rounds;
        values += c.values;
        line += std::string(hybrid ? ", \"hybrid\": {" : "\"doc\": {") + "\"table\": " + json_list(m, table) + ", \"steps\": [";
        for (size_t s = 0; s < steps; ++s) {
            const LookupStep &st = rec.steps[s];
            line += std::string(s ? ", " : "") + "{\"qs\": [";
            for (size_t k = 0; k < st.qs.size(); ++k) line += (k ? ", " : "") + std::to_string(st.qs[k]);
            line += "], \"vs\": " + json_list(m, st.vs) + ", \"prev_q\": " + json_list(m, st.prev_q) + ", \"prev_v\": " + fe_hex(m, st.prev_v) +
                    ", \"claim_r\": " + fe_hex(m, st.claim_r) + ", \"g\": [";
            for (size_t i = 0; i < ell; ++i) line += (i ? ", " : "") + json_list(m, {st.g[i][0], st.g[i][1], st.g[i][2]});
            line += "], \"sc_rs\": " + json_list(m, st.sc_rs) + ", \"next_v\": " + fe_hex(m, st.next_v) + "}";
        }
        line += "], \"eval\": " + fe_hex(m, hf.eval);
        if (hybrid) line += ", \"q0\": " + fe_hex(m, q[0]) + ", \"t\": " + fe_hex(m, pub_eval(m, t, q.data() + 1)) + ", \"public\": " + std::to_string(t.pub.size());
        line += "}";
    }
    return line + "}, \"rounds_checked\": " + std::to_string(rounds) + ", \"values_checked\": " + std::to_string(values) + "}";
}
