// replay_lookup.hpp -- the lookup leg of the replay (reef_replay_run_lookup, `reef_replay cfgN lookup`): the lookup argument a folding
// step runs (wit_nlookup_gadget, r1cs.rs:2177-2393) from the document's bytes to the claim the consistency argument proves
// (framework.rs:629-639, 708-721), as ONE chain of device rows through the C ABI and reef_provider.hpp only:
//   bytes -> reef_doc_transform (2n) -> device symbols -> reef_hyrax_create / _commit (2m)  and  reef_sc_set_table_parts (2b)
//   per step: v = reef_sc_lookup(qs); claim_r; reset, gen_eq_table(prev_running_q reversed), ell x linear_mle_product, read
//   the last (sc_rs, next_running_v) -> running_q as proof_dot_prod_prover forms it -> reef_hyrax_eval_begin / _eval_comm_own / IPA (2i)
//   the verifier's half of that argument on the device: reef_hyrax_vk_create over the rows commit produced, reef_hyrax_vk_comm_lz (2o),
//   reef_ipa_check_eq (2k)
// After the device symbols exist the host's own copy of them goes into no device call: it serves the checks (lookup_check.hpp) only.
#pragma once
#include "lookup_check.hpp"
#include "replay_prove.hpp"   // Curve, is_dlog_point, one_point_key, g_checked, g_small_key

struct LookupFlags {
    std::string mode, tamper;     // mode: "" (from the shape), "doc", "hybrid"
    int proj = 0, width = 1;
};
static LookupFlags parse_lookup_flags(const char *flags) {
    LookupFlags o;
    const std::string f = flags ? flags : "";
    for (size_t p = 0; p < f.size();) {
        const size_t e = std::min(f.find(' ', p), f.size());
        const std::string w = f.substr(p, e - p);
        if (w.rfind("tamper=", 0) == 0) o.tamper = w.substr(7);
        else if (w.rfind("mode=", 0) == 0) o.mode = w.substr(5);
        else if (w.rfind("proj=", 0) == 0) o.proj = atoi(w.c_str() + 5);
        else if (w.rfind("width=", 0) == 0) o.width = atoi(w.c_str() + 6);
        else if (!w.empty()) fail("reef_replay_run_lookup: unknown flag '" + w + "'");
        p = e + 1;
    }
    check_lookup_tamper_name(o.tamper);
    if (!o.mode.empty() && o.mode != "doc" && o.mode != "hybrid") fail("mode=" + o.mode + ": doc or hybrid");
    if (o.width != 1 && o.width != 2 && o.width != 4) fail("width: 1, 2 or 4");
    if (o.proj < 0) fail("proj: a non-negative number of chunk bits");
    return o;
}

static std::string lookup_body(const Shape &shape, const LookupFlags &fl) {
    const Shape *sh = &shape;
    if (sh->merkle_log > 0) fail("reef_replay lookup: " + sh->name + " commits with a Merkle tree; the lookup leg covers the Hyrax route only");
    if (!sh->doc_log || !sh->table_log || sh->lookups < 1) fail("reef_replay lookup: " + sh->name + " has no document or no lookup table");
    const bool hybrid = fl.mode.empty() ? sh->table_log == sh->doc_log + 1 : fl.mode == "hybrid";
    if (hybrid && fl.proj) fail("reef_replay lookup: proj with mode=hybrid is not replayed");
    if (fl.proj >= sh->doc_log) fail("proj: fewer chunk bits than the document has variables");
    if (sh->symbol_bits < 2) fail("reef_replay lookup: symbols of at least 2 bits (one character, EPSILON, EOF)");
    const Mod m(ORDER[REEF_PALLAS]);
    const size_t doc_log = (size_t)sh->doc_log, n_doc = (size_t)1 << doc_log;
    const size_t ell = hybrid ? doc_log + 1 : doc_log - (size_t)fl.proj, len = (size_t)1 << ell;
    const size_t chunk_len = n_doc >> fl.proj, chunk = fl.proj ? ((size_t)1 << fl.proj) - 2 : 0;   // proj: the last chunk but one, index bits 1..10
    const size_t steps = (size_t)sh->steps, nq = (size_t)sh->lookups;
    const uint32_t eb = (uint32_t)fl.width;
    int dev = 0;
    CK(reef_get_device(&dev));

    // ---- 1. seeded text over the shape's alphabet -> device symbols (the measuring call, then the writing call)
    const size_t alpha = std::min<size_t>(((size_t)1 << std::min(sh->symbol_bits, 16)) - 3, 90);
    std::vector<uint32_t> map(0x20 + alpha, REEF_DOC_BAD);
    for (size_t k = 0; k < alpha; ++k) map[0x20 + k] = (uint32_t)k;
    map[0x1A] = (uint32_t)alpha + 2;
    const size_t nbytes = n_doc - 2 - std::max<size_t>(1, n_doc / 16);                          // EOF, EPSILON and some zero padding fill up 2^doc_log
    std::vector<uint8_t> text(nbytes);
    {
        Rng rng{0xD0C0 + doc_log};
        for (uint8_t &b : text) b = (uint8_t)(0x20 + rng.next() % alpha);
    }
    const dev_ptr<uint8_t> d_text = device_alloc<uint8_t>(nbytes);
    CK(reef_memcpy(d_text.get(), text.data(), nbytes, REEF_DEVICE, REEF_HOST));
    auto t0 = clk::now();
    const reef_doc_info measured = reef_provider::doc_transform(d_text.get(), nbytes, REEF_DEVICE, REEF_DOC_BYTES, map, alpha, nullptr, eb, 0, REEF_DEVICE);
    if (measured.padded != n_doc) fail("reef_doc_transform measured " + std::to_string(measured.padded) + " symbols for a document of 2^" + std::to_string(doc_log));
    const dev_ptr<uint8_t> d_sym = device_alloc<uint8_t>(n_doc * eb);
    const reef_doc_info info = reef_provider::doc_transform(d_text.get(), nbytes, REEF_DEVICE, REEF_DOC_BYTES, map, alpha, d_sym.get(), eb, n_doc, REEF_DEVICE);
    const double transform_ms = ms_since(t0);
    const size_t live = (size_t)info.kept + 2;
    // the host's restatement of the map on the bytes it generated: for the checks only
    std::vector<uint8_t> doc8(n_doc, 0);
    for (size_t i = 0; i < nbytes; ++i) doc8[i] = (uint8_t)(text[i] - 0x20);
    doc8[nbytes] = (uint8_t)(alpha + 2);
    doc8[nbytes + 1] = (uint8_t)(alpha + 1);

    // ---- 2. the resident document and its commitment on a gens_v key made as the prove leg makes its keys
    const size_t left = doc_log / 2, right = doc_log - left, rows = (size_t)1 << left, cols = (size_t)1 << right;
    const dev_ptr<reef_affine> d_row_gens = device_alloc<reef_affine>(cols);
    CK(reef_gen_bases(REEF_PALLAS, 0xFEED, 3, cols, d_row_gens.get(), REEF_DEVICE));
    reef_msm_ctx *row_key = nullptr;
    const reef_msm_opts ko = fixed_key_opts(false, -1);
    CK(reef_msm_ctx_create(&row_key, REEF_PALLAS, d_row_gens.get(), cols, REEF_DEVICE, &ko));
    const ctx_ptr row_key_owner(row_key);
    Curve pc_curve;
    pc_curve.id = REEF_PALLAS;
    pc_curve.one = one_point_key(REEF_PALLAS);
    const ctx_ptr one_owner(pc_curve.one);
    std::vector<reef_fe> hg(cols), blinds(rows);
    for (size_t j = 0; j < cols; ++j) hg[j] = fsmall(m, 0xFEED + 3 * j);
    {
        Rng rng{0xB1D5};
        for (reef_fe &b : blinds) b = rng.full(m);
    }
    const reef_fe hd = fsmall(m, 0xB11D), g1 = fsmall(m, 0x6E1);
    reef_affine h;
    CK(reef_gen_bases(REEF_PALLAS, 0xB11D, 0, 1, &h, REEF_HOST));
    using HyraxP = reef_provider::HyraxEval<REEF_PALLAS>;
    t0 = clk::now();
    HyraxP hyrax(d_sym.get(), n_doc, (int)eb, REEF_DEVICE, doc_log, left, blinds.data(), dev);
    const std::vector<reef_provider::Compressed> comm = hyrax.commit(row_key, &h);
    const double commit_ms = ms_since(t0);

    // ---- 3. the table from parts
    LookupRecord rec;
    LookupTable &tb = rec.tbl;
    tb.ell = ell;
    tb.hybrid = hybrid;
    tb.have_doc = true;
    tb.eval_on_host = ell <= 16;                                         // above that T~ of the document part comes from row N3
    tb.doc.assign(doc8.begin() + chunk * chunk_len, doc8.begin() + (chunk + 1) * chunk_len);
    memcpy(&rec.doc_hash, comm[0].data(), sizeof(reef_fe));
    rec.doc_hash.l[3] &= 0x0fffffffffffffffULL;
    rec.doc_hash = to_m(m, rec.doc_hash);
    std::vector<reef_fe> pub_canon;
    const reef_fe fill_canon = {{0x123456789abcdef1ULL, 0x0fedcba987654321ULL, 0x1111111122222222ULL, 0x0333333344444444ULL}};
    std::vector<reef_sc_part> parts;
    const uint8_t *d_chunk = d_sym.get() + chunk * chunk_len * eb;
    if (hybrid) {
        const size_t half = len / 2, trans = std::min<size_t>(256, half / 2);
        pub_canon.resize(trans);
        CK(reef_gen_scalars(REEF_PALLAS, 0x7AB1E, 0, 0, trans, false, pub_canon.data(), REEF_HOST));
        for (const reef_fe &v : pub_canon) tb.pub.push_back(to_m(m, v));
        tb.fill = to_m(m, fill_canon);
        parts.push_back({REEF_SC_PART_FE, 0, pub_canon.data(), trans, REEF_HOST});
        parts.push_back({REEF_SC_PART_FILL, 0, &fill_canon, half - trans, REEF_HOST});
    }
    parts.push_back({REEF_SC_PART_SYMBOLS, eb, d_chunk, chunk_len, REEF_DEVICE});
    reef_provider::SumCheck sc(ell);
    t0 = clk::now();
    sc.set_table_parts(parts);
    const double set_table_ms = ms_since(t0);

    // the seeded lookups: index 0, the last live entry, the zero padding where there is some, both sides of every part boundary, the last
    // entry; the last lookup of a step repeats its first
    std::vector<uint64_t> special = {0, len - 1};
    const size_t doc_at = hybrid ? len / 2 : 0;
    if (hybrid) for (uint64_t q : {(uint64_t)tb.pub.size() - 1, (uint64_t)tb.pub.size(), (uint64_t)doc_at - 1, (uint64_t)doc_at}) special.push_back(q);
    if (!fl.proj) for (uint64_t q : {(uint64_t)(doc_at + live - 1), (uint64_t)(doc_at + live)}) special.push_back(q);
    Rng qrng{0x100C + ell};
    size_t next_special = 0;

    // ---- 4. the folding steps
    double lookup_ms = 0, sumcheck_ms = 0;
    std::vector<reef_fe> prev_q(ell), next_q;
    reef_fe prev_v = {};
    for (size_t s = 0; s < steps; ++s) {
        LookupStep st;
        for (size_t k = 0; k < nq; ++k) {
            if (k && k + 1 == nq) st.qs.push_back(st.qs[0]);
            else if (next_special < special.size()) st.qs.push_back(special[next_special++]);
            else st.qs.push_back(qrng.next() & (len - 1));
        }
        t0 = clk::now();
        const std::vector<reef_fe> v = sc.lookup(st.qs);
        if (s == 0) prev_v = to_m(m, sc.lookup({0})[0]);                 // prev_running_v = T[0] (r1cs.rs:2198-2201)
        lookup_ms += ms_since(t0);
        for (const reef_fe &x : v) st.vs.push_back(to_m(m, x));
        st.prev_q = prev_q;
        st.prev_v = prev_v;
        t0 = clk::now();
        StandinTranscript T(m, LOOKUP_DOMAIN + s);
        st.claim_r = lookup_claim_r(T, rec.doc_hash, st);
        std::vector<reef_fe> rs_canon, last_q;
        for (const reef_fe &r : lookup_rs(m, st.claim_r, nq)) rs_canon.push_back(from_m(m, r));
        for (size_t j = 0; j < ell; ++j) last_q.push_back(from_m(m, prev_q[ell - 1 - j]));      // reversed (r1cs.rs:2319)
        const std::vector<uint32_t> qs32(st.qs.begin(), st.qs.end());
        sc.start_step();
        sc.gen_eq_table(rs_canon, qs32, last_q);
        for (size_t i = 1; i <= ell; ++i) {
            sc.linear_mle_product(i, [&](const std::array<reef_fe, 3> &query) {              // {con, x, xsq}, canonical
                st.g.push_back({to_m(m, query[2]), to_m(m, query[1]), to_m(m, query[0])});
                st.sc_rs.push_back(lookup_round_r(T, st.g.back()));
                return from_m(m, st.sc_rs.back());
            });
        }
        st.next_v = to_m(m, sc.final_value());
        sumcheck_ms += ms_since(t0);
        if (!tb.eval_on_host) {                                            // the "n3" route: the document part at the step's point by row N3's kernels
            const size_t dv = tb.doc_vars(), dl = dv / 2;
            std::vector<reef_fe> lz((size_t)1 << (dv - dl));
            CK(reef_mle_bound_rows(REEF_PALLAS, d_chunk, chunk_len, (int)eb, REEF_DEVICE, true, st.sc_rs.data() + (ell - dv), dv, dl, lz.data(), REEF_HOST, &st.doc_eval));
        }
        prev_q = st.sc_rs;
        prev_v = st.next_v;
        rec.steps.push_back(std::move(st));
    }

    // ---- 5. the hand-over, as proof_dot_prod_prover forms running_q (commitment.rs:305-345)
    const std::vector<reef_fe> &q = rec.steps.back().sc_rs;
    std::vector<reef_fe> point;
    for (int b = fl.proj - 1; b >= 0; --b) point.push_back(((chunk >> b) & 1) ? m.one : reef_fe{});   // the chunk index bits, most significant first
    point.insert(point.end(), q.end() - (doc_log - (size_t)fl.proj), q.end());
    HyraxP::Proof hpf;
    StandinTranscript ht(m, 0xD0C);
    const auto q_of = [&](const reef_fe &r) {
        const reef_fe d = fmul(m, g1, r);
        reef_jacobian j;
        CK(reef_msm(pc_curve.one, &d, 1, REEF_HOST, true, &j, REEF_HOST));
        reef_affine a;
        CK(reef_normalize(REEF_PALLAS, &j, 1, REEF_HOST, &a, nullptr));
        return a;
    };
    t0 = clk::now();
    hyrax.prove_own(row_key, point.data(), ht.fn(), q_of, hpf, g_small_key);
    const double consistency_ms = ms_since(t0);

    // ---- the checks
    t0 = clk::now();
    reef_fe handed = hpf.eval;
    apply_lookup_tamper(m, fl.tamper, rec, handed, hpf);
    const LookupCounts counts = check_lookup(m, rec);
    check_claim(m, rec, handed);
    Curve *cp = &pc_curve;
    const PointCheck pcp = [cp](const char *phase, const reef_jacobian &pt, const reef_fe &dlog, const std::string &what) {
        if (!is_dlog_point(*cp, pt, dlog, true)) reject(phase, what + " differs from its discrete-logarithm closed form");
    };
    check_hyrax(m, doc8, doc_log, left, point, hpf, hg, blinds, hd, g1, pcp);
    const double check_ms = ms_since(t0);

    // ---- the verifier's half on the device, from what a verifier holds: the compressed rows, the point, the proof.  comm_LZ through a vk
    // must be the point reef_hyrax_eval_comm_own gave the prover, and reef_ipa_check_eq must accept the proof against it (the row blinds
    // leave lz_blind h in comm_LZ; the rounds carry no blinds of their own)
    t0 = clk::now();
    const reef_provider::HyraxVk<REEF_PALLAS> vk(comm.data(), left, dev);
    const double verify_vk_create_ms = ms_since(t0);
    t0 = clk::now();
    std::vector<reef_provider::Compressed> vk_lz32;
    const std::vector<reef_jacobian> vk_lz = vk.comm_lz(point.data(), 1, &vk_lz32);
    const double verify_comm_lz_ms = ms_since(t0);
    if (vk_lz32[0] != reef_provider::compress<REEF_PALLAS>(hpf.comm_lz) || vk_lz32[0] != reef_provider::compress<REEF_PALLAS>(vk_lz[0]))
        reject("verify", "comm_LZ through reef_hyrax_vk_comm_lz differs from reef_hyrax_eval_comm_own's");
    t0 = clk::now();
    reef_provider::InnerProductArgument<REEF_PALLAS> ipa;
    ipa.L = hpf.L;
    ipa.R = hpf.R;
    ipa.a_hat = hpf.a_hat;
    const bool device_verified = ipa.verify(row_key, cols, vk_lz[0], hpf.eval, q_of(hpf.r_q), hpf.r_rounds,
                                            {std::vector<reef_fe>(point.begin() + left, point.end())}, {m.one}, &h, &hpf.lz_blind);
    const double verify_ipa_ms = ms_since(t0);
    if (!device_verified) reject("verify", "reef_ipa_check_eq rejects the consistency argument against the vk's comm_LZ");

    const double ns = (double)steps;
    std::vector<char> line(4096);
    snprintf(line.data(), line.size(),
             "{\"replay\": \"%s\", \"leg\": \"lookup\", \"note\": \"the lookup argument of every folding step from the document's bytes to the consistency argument, "
             "one chain of device rows through the C ABI (reef_doc_transform, reef_hyrax_create / _commit, reef_sc_set_table_parts, reef_sc_lookup, the N2 rounds, "
             "reef_hyrax_eval_begin / _eval_comm_own / IPA), checked on the host\", \"transcript\": \"stand-in hash for neptune's sponge: binds every challenge to what "
             "preceded it, parity unpinned\", \"mode\": \"%s\", \"proj\": %d, \"width\": %u, \"doc_log\": %zu, \"table_log\": %zu, \"steps\": %zu, \"lookups\": %zu, "
             "\"text_bytes\": %zu, \"live_symbols\": %zu, \"table_eval\": \"%s\", \"transform_ms\": %.3f, \"commit_ms\": %.3f, \"set_table_ms\": %.3f, "
             "\"lookup_ms_per_step\": %.3f, \"sumcheck_ms_per_step\": %.3f, \"ms_per_step\": %.3f, \"consistency_ms\": %.3f, \"consistency_rounds\": %zu, \"check_ms\": %.3f, "
             "\"timed\": \"sumcheck_ms_per_step: claim_r, reset, gen_eq_table, ell rounds with the stand-in transcript on the host, the read of next_running_v; "
             "lookup_ms_per_step: reef_sc_lookup host to host\", \"rounds_checked\": %zu, \"values_checked\": %zu, \"points_checked\": %d, \"proof_checked\": true, "
             "\"verify_vk_create_ms\": %.3f, \"verify_comm_lz_ms\": %.3f, \"verify_ipa_ms\": %.3f, \"device_verified\": %s}",
             sh->name.c_str(), hybrid ? "hybrid" : "doc", fl.proj, eb, doc_log, ell, steps, nq, nbytes, live, tb.eval_on_host ? "host" : "n3", transform_ms, commit_ms,
             set_table_ms, lookup_ms / ns, sumcheck_ms / ns, (lookup_ms + sumcheck_ms) / ns, consistency_ms, hpf.r_rounds.size(), check_ms, counts.rounds,
             counts.values, g_checked, verify_vk_create_ms, verify_comm_lz_ms, verify_ipa_ms, device_verified ? "true" : "false");
    return std::string(line.data());
}
