// replay_prove.hpp -- the device run of the prove leg (reef_replay_run_prove); its checks are proof_check.hpp.
#pragma once
#include "replay_msm.hpp"   // Curve, g_checked, the sum-check and document helpers

// ==== the prove leg (`reef_replay cfgN prove`) =========================================================================================
// Every device row of one proof, through the C ABI and the provider mirror (reef_provider.hpp), in the order `reef --prove` runs
// them (framework.rs:642-754): per folding step the N2 sum-check step and, per curve, comm_W, NIFS commit_T, a challenge and the
// fold (3f; with `paired` the two commitments are one reef_nifs_commit_step, and the folded instance's comm_W, comm_E come from the ctx); the last fold; per curve the Spartan sum-checks (3g) and the batched IPA opening (3h) on the instance the folds left
// on the device; the Hyrax consistency argument over the committed document (3i).  The R1CS matrices are SYNTHETIC (layered,
// satisfiable, of the shape's sizes), the transcript is a stand-in hash, and the point operations the Rust host does on
// commitments (comm_W, comm_E of a folded instance, comm_a) are tracked as discrete logarithms, which every generator here has.
// After the timed region the proof is checked with the verifier's equations on the host, and every point the device returned
// against its discrete logarithm; `tamper=<phase>` alters one recorded value first, to show that the checks can fail.

// ---- the device run ----------------------------------------------------------------------------------------------------------------
template <int CURVE> struct ProveSide {
    using Snark = reef_provider::RelaxedR1CSSnark<CURVE>;
    const Mod &m;
    const char *name;
    size_t num_cons, num_vars, ncp = 0, nvp = 0, n = 0;
    Curve c;                                        // c.key: the commitment key, exactly n = max(ncp, nvp) points; c.one: [G]
    dev_ptr<reef_affine> gens;
    ctx_ptr key_owner, one_owner;
    R1cs S;
    std::vector<reef_fe> g;                         // the generators' discrete logarithms
    reef_fe gs = {};                                // gens_s's (the opening's q = gens_s.scale(r_ipa))
    std::unique_ptr<reef_provider::Nifs<CURVE>> nifs;
    StandinTranscript tr;
    NifsRecord rec;
    typename Snark::Proof pf;
    Inst fin;                                       // the running instance, read back after the timed region
    uint64_t violations = 0;
    double init_ms = 0, spartan_ms = 0, open_ms = 0;
    reef_fe comm_a_dlog = {};                       // the opening's comm_a = comm_E + r comm_W and q, as the callbacks produced them
    reef_affine q_open = {};
    double verify_ipa_ms = 0;                       // 3j on the opening, after the host checks
    double verify_evals_ms = 0, verify_evals_host_ms = 0;   // 3k on the device (warm: the second call) against the host loop of proof_check.hpp alone
    bool paired = false;                            // `paired`: comm_W and comm_T of a step from one reef_nifs_commit_step, the running instance's points from the ctx
    ProveSide(const Mod &mod, const char *nm, size_t cons, size_t vars, uint64_t domain) : m(mod), name(nm), num_cons(cons), num_vars(vars), tr(mod, domain) {}
    Inst fresh(uint64_t seed) const { return fresh_instance(m, S, seed); }
};

// key, one-point key, synthetic shape and the NIFS context (PublicParams::setup: not timed)
template <int CURVE> static void prove_setup(ProveSide<CURVE> &s, bool tables) {
    s.ncp = next_pow2(s.num_cons);
    s.nvp = next_pow2(s.num_vars);
    s.n = std::max(s.ncp, s.nvp);
    s.c.id = CURVE;
    s.c.n = s.n;
    s.c.k0 = 0xC0FFEE + CURVE;
    s.c.d = 7;
    s.gens = device_alloc<reef_affine>(s.n);
    s.c.d_gens = s.gens.get();
    CK(reef_gen_bases(CURVE, s.c.k0, s.c.d, s.n, s.c.d_gens, REEF_DEVICE));
    s.c.one = one_point_key(CURVE);
    s.one_owner.reset(s.c.one);
    const reef_msm_opts o = fixed_key_opts(tables, -1);
    CK(reef_msm_ctx_create(&s.c.key, CURVE, s.c.d_gens, s.n, REEF_DEVICE, &o));
    s.key_owner.reset(s.c.key);
    CK(reef_msm_ctx_sync(s.c.key));
    s.g.resize(s.n);
    const reef_fe step = fsmall(s.m, s.c.d);
    s.g[0] = fsmall(s.m, s.c.k0);
    for (size_t i = 1; i < s.n; ++i) s.g[i] = fadd(s.m, s.g[i - 1], step);
    s.gs = fsmall(s.m, 0x5EED + CURVE);
    s.S = layered_r1cs(s.m, s.num_cons, s.num_vars, 0x51A7 + CURVE);
    int dev = 0;
    CK(reef_get_device(&dev));
    s.nifs.reset(new reef_provider::Nifs<CURVE>(s.num_cons, s.num_vars, s.S.num_io, dev));
    for (int k = 0; k < 3; ++k) s.nifs->set_matrix(k, s.S.row[k].data(), s.S.col[k].data(), s.S.val[k].data(), s.S.row[k].size(), true);
}
// dl * G through the one-point key, affine: the host's point operation gens.scale(r) when gens has a known discrete logarithm
template <int CURVE> static reef_affine scaled_G(ProveSide<CURVE> &s, const reef_fe &dl) {
    reef_jacobian j;
    CK(reef_msm(s.c.one, &dl, 1, REEF_HOST, true, &j, REEF_HOST));
    reef_affine a;
    CK(reef_normalize(CURVE, &j, 1, REEF_HOST, &a, nullptr));
    return a;
}
template <int CURVE> static PointCheck point_check(ProveSide<CURVE> &s) {
    Curve *c = &s.c;
    return [c](const char *phase, const reef_jacobian &pt, const reef_fe &dlog, const std::string &what) {
        if (!is_dlog_point(*c, pt, dlog, true)) reject(phase, what + " differs from its discrete-logarithm closed form");
    };
}

// the first running instance (u = 1, E = 0) and its comm_W
template <int CURVE> static void nifs_init(ProveSide<CURVE> &s, const Inst &f0) {
    const auto t0 = clk::now();
    s.nifs->set_running(f0.W.data(), nullptr, f0.u, f0.X.data(), REEF_HOST, true);
    reef_jacobian cw;
    if (s.paired) s.nifs->commit_running(s.c.key, &cw, nullptr);      // the ctx holds W already: no second upload
    else CK(reef_msm(s.c.key, f0.W.data(), s.num_vars, REEF_HOST, true, &cw, REEF_HOST));
    s.tr.absorb("U1", &cw, sizeof cw);
    s.init_ms = ms_since(t0);
    s.rec.dW = dot(s.m, f0.W.data(), s.g.data(), s.num_vars);
    s.rec.u = f0.u;
    s.rec.X = f0.X;
    s.rec.points.push_back({cw, s.rec.dW, "comm_W of the first instance"});
}
// one NIFS::prove of a folding step: comm_W of the fresh witness (scalars from host memory), commit_T, the challenge, the fold;
// `paired`: both commitments from one reef_nifs_commit_step (one upload of W, counted under nifs_ms)
struct StepOut { reef_jacobian comm_W, comm_T; reef_fe r; double commit_w_ms, nifs_ms; };
template <int CURVE> static StepOut step_fold(ProveSide<CURVE> &s, const Inst &f) {
    StepOut o;
    const auto t0 = clk::now();
    if (!s.paired) CK(reef_msm(s.c.key, f.W.data(), s.num_vars, REEF_HOST, true, &o.comm_W, REEF_HOST));
    const auto t1 = clk::now();
    o.commit_w_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    if (s.paired) {
        const auto both = s.nifs->commit_step(s.c.key, f.W.data(), f.X.data(), REEF_HOST, true);
        o.comm_W = both.comm_W2;
        o.comm_T = both.comm_T;
    } else o.comm_T = s.nifs->commit_T(s.c.key, f.W.data(), f.X.data(), REEF_HOST, true);
    const reef_jacobian both[2] = {o.comm_W, o.comm_T};
    s.tr.absorb("fold", both, sizeof both);
    o.r = s.tr.squeeze();
    s.nifs->fold(o.r, true);
    o.nifs_ms = ms_since(t1);
    return o;
}
// outside the timing: T back from the device, the discrete logs of comm_W and comm_T, the tracked fold of comm_W, comm_E, u, X
template <int CURVE> static void step_record(ProveSide<CURVE> &s, const Inst &f, const StepOut &o, const std::string &what) {
    const std::vector<reef_fe> T = s.nifs->read(2, s.num_cons, true);
    const reef_fe dW2 = dot(s.m, f.W.data(), s.g.data(), s.num_vars), dT = dot(s.m, T.data(), s.g.data(), s.num_cons);
    s.rec.points.push_back({o.comm_W, dW2, "comm_W of " + what});
    s.rec.points.push_back({o.comm_T, dT, "comm_T of " + what});
    s.rec.dW = fadd(s.m, s.rec.dW, fmul(s.m, o.r, dW2));
    s.rec.dE = fadd(s.m, s.rec.dE, fmul(s.m, o.r, dT));
    s.rec.u = fadd(s.m, s.rec.u, o.r);
    s.rec.X = lin(s.m, s.rec.X, o.r, f.X);
}
// "small_key=N" of the prove leg: the openings and the Hyrax argument move their late rounds to a folded key of N points (0: never)
static size_t g_small_key = 0;
// RelaxedR1CSSNARK::prove on the folded instance: 3g, then 3h with the same key as commit_T
template <int CURVE> static void final_snark(ProveSide<CURVE> &s) {
    const typename ProveSide<CURVE>::Snark snark(*s.nifs, s.ncp, s.nvp);
    if (snark.opening_len() != s.c.n) fail("the opening needs a key of exactly " + std::to_string(snark.opening_len()) + " points");
    const reef_provider::Transcript tr = s.tr.fn();
    auto t0 = clk::now();
    snark.prove_sumchecks(tr, s.pf);
    s.spartan_ms = ms_since(t0);
    t0 = clk::now();
    snark.prove_opening(
        s.c.key, tr,
        [&](const reef_fe &r) {   // comm_a = comm_E + r comm_W, as its discrete logarithm
            const reef_fe d = fadd(s.m, s.rec.dE, fmul(s.m, r, s.rec.dW));
            s.comm_a_dlog = d;
            return std::vector<uint8_t>((const uint8_t *)&d, (const uint8_t *)&d + sizeof d);
        },
        [&](const reef_fe &r) { return s.q_open = scaled_G(s, fmul(s.m, s.gs, r)); }, s.pf, g_small_key);
    s.open_ms = ms_since(t0);
}
// After the host checks: the verifier's matrix evaluations on the device (3k) at the recorded (r_x, r_y), on the ctx the prove ran on.
// A~ + r B~ + r^2 C~ must equal the recorded claims_inner[0] and the host's own value.  Both sides build their eq tables on the clock.
template <int CURVE> static void device_matrix_evals(ProveSide<CURVE> &s) {
    const typename ProveSide<CURVE>::Snark snark(*s.nifs, s.ncp, s.nvp);
    snark.eval_matrices(s.pf.r_x, s.pf.r_y);                  // the first call makes the workspace
    auto t0 = clk::now();
    const std::array<reef_fe, 3> dev = snark.eval_matrices(s.pf.r_x, s.pf.r_y);
    s.verify_evals_ms = ms_since(t0);
    t0 = clk::now();
    const std::vector<reef_fe> erx = eq_evals(s.m, s.pf.r_x.data(), s.pf.r_x.size()), ery = eq_evals(s.m, s.pf.r_y.data(), s.pf.r_y.size());
    const std::array<reef_fe, 3> host = host_matrix_evals(s.m, s.S, s.nvp, erx, ery);
    s.verify_evals_host_ms = ms_since(t0);
    const reef_fe r = s.pf.r_joint, r2 = fmul(s.m, r, r);
    const reef_fe abc_dev = fadd(s.m, fadd(s.m, dev[0], fmul(s.m, r, dev[1])), fmul(s.m, r2, dev[2]));
    const reef_fe abc_host = fadd(s.m, fadd(s.m, host[0], fmul(s.m, r, host[1])), fmul(s.m, r2, host[2]));
    const std::string cn(s.name);
    for (int k = 0; k < 3; ++k) EXPECT("spartan", feq(dev[k], host[k]), cn + ": the device's matrix evaluation " + "ABC"[k] + "~(r_x, r_y) differs from the host's");
    EXPECT("spartan", feq(abc_dev, abc_host), cn + ": the device's A~ + r B~ + r^2 C~ differs from the host's");
    EXPECT("spartan", feq(abc_dev, s.pf.claims_inner[0]), cn + ": the device's A~ + r B~ + r^2 C~ differs from the recorded claims_inner[0]");
}
// and the opening through InnerProductArgument::verify (3j): comm_a as the point of its tracked discrete logarithm, c, q, the recorded
// L, R, round challenges and a_hat, b = eq(r_x) + r_fold eq(r_y[1..]) built on the device
template <int CURVE> static void device_ipa_verify(ProveSide<CURVE> &s) {
    reef_jacobian comm;
    CK(reef_msm(s.c.one, &s.comm_a_dlog, 1, REEF_HOST, true, &comm, REEF_HOST));
    reef_provider::InnerProductArgument<CURVE> ipa;
    ipa.L = s.pf.L;
    ipa.R = s.pf.R;
    ipa.a_hat = s.pf.a_hat;
    const std::vector<std::vector<reef_fe>> points = {s.pf.r_x, std::vector<reef_fe>(s.pf.r_y.begin() + 1, s.pf.r_y.end())};
    const std::vector<reef_fe> weights = {s.m.one, s.pf.r_fold};
    const auto t0 = clk::now();
    const bool ok = ipa.verify(s.c.key, s.n, comm, s.pf.c, s.q_open, s.pf.r_rounds, points, weights);
    s.verify_ipa_ms = ms_since(t0);
    EXPECT("open", ok, std::string(s.name) + ": the device's IPA check rejects the recorded opening");
}
template <int CURVE> static void read_back(ProveSide<CURVE> &s) {
    s.fin.W = s.nifs->read(0, s.num_vars, true);
    s.fin.E = s.nifs->read(1, s.num_cons, true);
    s.fin.u = s.nifs->read(3, 1, true)[0];
    s.fin.X = s.nifs->read(4, s.S.num_io, true);
    s.violations = s.nifs->check_relaxed();
    if (s.paired) {   // the device's comm_W and comm_E of the folded instance against the host's tracked point operations
        reef_jacobian cw, ce;
        s.nifs->commit_running(s.c.key, &cw, &ce);
        s.rec.points.push_back({cw, s.rec.dW, "comm_W of the folded instance (reef_nifs_commit_running)"});
        s.rec.points.push_back({ce, s.rec.dE, "comm_E of the folded instance (reef_nifs_commit_running)"});
    }
}

static std::string prove_body(const Shape &shape, const std::string &tamper, bool tables, bool paired = false) {
    const Shape *sh = &shape;
    check_tamper_name(tamper);
    if (tamper == "hyrax" && !sh->doc_log) fail("tamper=hyrax: " + sh->name + " has no Hyrax consistency argument");
    const Mod mp(ORDER[REEF_PALLAS]), mv(ORDER[REEF_VESTA]);
    ProveSide<REEF_PALLAS> P(mp, "pallas", sh->c1, sh->w1, 0xA11A5);
    ProveSide<REEF_VESTA> V(mv, "vesta", sh->c2, sh->w2, 0x7E57A);
    P.paired = V.paired = paired;
    prove_setup(P, tables);
    prove_setup(V, tables);
    sc_ptr sc;
    if (sh->table_log) sc = sumcheck_ctx(sh);

    // ---- the document (--commit, before the proof): Hyrax rows with blinds, and the document resident for the consistency argument
    using HyraxP = reef_provider::HyraxEval<REEF_PALLAS>;
    std::unique_ptr<HyraxP> hyrax;
    HyraxP::Proof hpf;
    std::vector<uint8_t> doc;
    std::vector<reef_fe> hg, blinds, point;
    std::vector<reef_affine> row_aff;
    std::vector<PointRec> row_points;
    dev_ptr<uint8_t> d_doc;
    dev_ptr<reef_affine> d_row_gens;
    ctx_ptr row_key_owner;
    reef_msm_ctx *row_key = nullptr;
    const size_t left = (size_t)sh->doc_log / 2, right = (size_t)sh->doc_log - left;
    const reef_fe hd = fsmall(mp, 0xB11D), g1 = fsmall(mp, 0x6E1);    // discrete logs of h and of gens_1 (the argument's q)
    double commit_hyrax_ms = 0, hyrax_create_ms = 0, consistency_ms = 0;
    if (sh->doc_log) {
        const size_t n_doc = (size_t)1 << sh->doc_log, rows = (size_t)1 << left, cols = (size_t)1 << right;
        doc = host_symbols(n_doc, sh->symbol_bits, 0xD0C);
        d_doc = device_alloc<uint8_t>(n_doc);
        CK(reef_memcpy(d_doc.get(), doc.data(), n_doc, REEF_DEVICE, REEF_HOST));
        d_row_gens = device_alloc<reef_affine>(cols);
        CK(reef_gen_bases(REEF_PALLAS, 0xFEED, 3, cols, d_row_gens.get(), REEF_DEVICE));
        const reef_msm_opts o = fixed_key_opts(tables, -1);
        CK(reef_msm_ctx_create(&row_key, REEF_PALLAS, d_row_gens.get(), cols, REEF_DEVICE, &o));
        row_key_owner.reset(row_key);
        hg.resize(cols);
        for (size_t j = 0; j < cols; ++j) hg[j] = fsmall(mp, 0xFEED + 3 * j);
        Rng rng{0xB1D5};
        blinds.resize(rows);
        for (reef_fe &b : blinds) b = rng.full(mp);
        reef_affine h;
        CK(reef_gen_bases(REEF_PALLAS, 0xB11D, 0, 1, &h, REEF_HOST));
        const dev_ptr<reef_fe> d_blinds = device_alloc<reef_fe>(rows);
        const dev_ptr<reef_affine> d_h = device_alloc<reef_affine>(1);
        CK(reef_memcpy(d_blinds.get(), blinds.data(), rows * sizeof(reef_fe), REEF_DEVICE, REEF_HOST));
        CK(reef_memcpy(d_h.get(), &h, sizeof h, REEF_DEVICE, REEF_HOST));
        std::vector<reef_jacobian> row_comms(rows);
        auto t0 = clk::now();
        CK(reef_msm_rows_symbols(row_key, d_doc.get(), rows, cols, REEF_DEVICE, (uint32_t)sh->symbol_bits, d_blinds.get(), d_h.get(), true,
                                 row_comms.data(), REEF_HOST));
        commit_hyrax_ms = ms_since(t0);
        row_aff.resize(rows);
        CK(reef_normalize(REEF_PALLAS, row_comms.data(), rows, REEF_HOST, row_aff.data(), nullptr));
        for (size_t i : {(size_t)0, rows - 1}) {   // two rows against <Z_i, G> + blind_i h
            reef_fe d = fmul(mp, blinds[i], hd);
            for (size_t j = 0; j < cols; ++j) d = fadd(mp, d, fmul(mp, fsmall(mp, doc[i * cols + j]), hg[j]));
            row_points.push_back({row_comms[i], d, "row commitment " + std::to_string(i)});
        }
        int dev = 0;
        CK(reef_get_device(&dev));
        t0 = clk::now();
        hyrax.reset(new HyraxP(d_doc.get(), n_doc, 1, REEF_DEVICE, (size_t)sh->doc_log, left, blinds.data(), dev));
        hyrax_create_ms = ms_since(t0);
    }

    // ---- the timed region: every folding step, the last fold, the final SNARK on both curves, the consistency argument
    int seed = 1;
    const Inst f0p = P.fresh(seed++), f0v = V.fresh(seed++);
    {   // the keys' first MSM (workspaces), as the MSM replay warms up
        reef_jacobian w;
        CK(reef_msm(P.c.key, f0p.W.data(), P.num_vars, REEF_HOST, true, &w, REEF_HOST));
        CK(reef_msm(V.c.key, f0v.W.data(), V.num_vars, REEF_HOST, true, &w, REEF_HOST));
        if (paired) {   // and the workspaces of a batch of two rows, which commit_step's first call would otherwise allocate on the clock
            reef_jacobian w2[2];
            std::vector<reef_fe> two(f0p.W);
            two.insert(two.end(), f0p.W.begin(), f0p.W.end());
            CK(reef_msm_rows(P.c.key, two.data(), 2, P.num_vars, REEF_HOST, true, 255, nullptr, nullptr, w2, REEF_HOST));
            two.assign(f0v.W.begin(), f0v.W.end());
            two.insert(two.end(), f0v.W.begin(), f0v.W.end());
            CK(reef_msm_rows(V.c.key, two.data(), 2, V.num_vars, REEF_HOST, true, 255, nullptr, nullptr, w2, REEF_HOST));
        }
    }
    nifs_init(P, f0p);
    nifs_init(V, f0v);
    std::vector<double> step_ms;
    double commit_w_ms = 0, nifs_ms = 0, sc_ms = 0;
    for (int k = 0; k < sh->steps; ++k) {
        const Inst fp = P.fresh(seed++), fv = V.fresh(seed++);     // witness generation: not timed
        const auto t0 = clk::now();
        if (sc) sc_ms += run_sumcheck_step(sc.get(), sh->table_log, sh->lookups);
        const StepOut op = step_fold(P, fp);
        const StepOut ov = step_fold(V, fv);
        step_ms.push_back(ms_since(t0));
        commit_w_ms += op.commit_w_ms + ov.commit_w_ms;
        nifs_ms += op.nifs_ms + ov.nifs_ms;
        step_record(P, fp, op, "step " + std::to_string(k));
        step_record(V, fv, ov, "step " + std::to_string(k));
    }
    // CompressedSNARK::prove folds the last secondary instance into the secondary running instance first
    const Inst flast = V.fresh(seed++);
    auto t0 = clk::now();
    const StepOut olast = step_fold(V, flast);
    const double final_fold_ms = ms_since(t0);
    step_record(V, flast, olast, "the last fold");
    final_snark(P);
    final_snark(V);
    if (hyrax) {
        StandinTranscript ht(mp, 0xD0C);
        const reef_provider::Transcript tr = ht.fn();
        t0 = clk::now();
        point.clear();
        for (int j = 0; j < sh->doc_log; ++j) point.push_back(tr("q", nullptr, 0));   // running_q: the proof's, a stand-in here
        hyrax->prove(row_key, point.data(), row_aff.data(), REEF_HOST, tr, [&](const reef_fe &r) { return scaled_G(P, fmul(mp, g1, r)); }, hpf, g_small_key);
        consistency_ms = ms_since(t0);
    }
    double steps_total = 0;
    for (double v : step_ms) steps_total += v;
    const double total = P.init_ms + V.init_ms + steps_total + final_fold_ms + P.spartan_ms + V.spartan_ms + P.open_ms + V.open_ms + consistency_ms;

    // ---- the checks
    t0 = clk::now();
    read_back(P);
    read_back(V);
    apply_tamper(mp, tamper, P.rec, P.pf, hyrax ? &hpf : nullptr);
    const PointCheck pcp = point_check(P), pcv = point_check(V);
    check_nifs(mp, P.rec, P.fin, P.g, P.violations, pcp, "pallas");
    check_nifs(mv, V.rec, V.fin, V.g, V.violations, pcv, "vesta");
    check_sumchecks(mp, P.S, P.fin, P.ncp, P.nvp, P.pf, "pallas");
    check_sumchecks(mv, V.S, V.fin, V.ncp, V.nvp, V.pf, "vesta");
    check_opening(mp, P.fin, P.ncp, P.nvp, P.pf, P.g, P.rec.dW, P.rec.dE, P.gs, pcp, "pallas");
    check_opening(mv, V.fin, V.ncp, V.nvp, V.pf, V.g, V.rec.dW, V.rec.dE, V.gs, pcv, "vesta");
    if (hyrax) {
        for (const PointRec &p : row_points) pcp("hyrax", p.pt, p.dlog, p.what);
        check_hyrax(mp, doc, (size_t)sh->doc_log, left, point, hpf, hg, blinds, hd, g1, pcp);
    }
    const double check_ms = ms_since(t0);
    device_matrix_evals(P);                                   // the host checks passed: a tampered record never gets here
    device_matrix_evals(V);
    device_ipa_verify(P);
    device_ipa_verify(V);

    std::string steps_list = "[";
    for (size_t k = 0; k < step_ms.size(); ++k) {
        char b[32];
        snprintf(b, sizeof b, "%s%.3f", k ? ", " : "", step_ms[k]);
        steps_list += b;
    }
    steps_list += "]";
    const double ns = (double)sh->steps;
    std::vector<char> line(8192);
    snprintf(line.data(), line.size(),
             "{\"replay\": \"%s\", \"leg\": \"prove\", \"note\": \"every device row of one proof through the C ABI (reef_provider.hpp Nifs, RelaxedR1CSSnark, HyraxEval), "
             "checked with the verifier's equations on the host\", \"matrices\": \"SYNTHETIC: layered satisfiable R1CS of the shape's sizes (2-4 entries per A/B row, "
             "one output per constraint, num_io = 2), not Reef's circuits\", \"transcript\": \"stand-in hash for nova's Keccak transcript [R]\", "
             "\"point_ops\": \"comm_W, comm_E of folded instances and comm_a tracked as discrete logarithms; q = dlog*G through a one-point key\", "
             "\"w1\": %zu, \"c1\": %zu, \"w2\": %zu, \"c2\": %zu, \"num_cons_pad_pallas\": %zu, \"num_vars_pad_pallas\": %zu, \"num_cons_pad_vesta\": %zu, "
             "\"num_vars_pad_vesta\": %zu, \"pad_pallas\": %zu, \"pad_vesta\": %zu, \"nnz_pallas\": %zu, \"nnz_vesta\": %zu, \"steps\": %d, \"nifs_init_ms\": %.3f, "
             "\"step_ms\": %s, \"ms_per_step\": %.3f, \"commit_w_ms_per_step\": %.3f, \"nifs_ms_per_step\": %.3f, \"sumcheck_ms_per_step\": %.3f, "
             "\"final_fold_ms\": %.3f, \"spartan_ms_pallas\": %.3f, \"spartan_ms_vesta\": %.3f, \"outer_rounds_pallas\": %zu, \"inner_rounds_pallas\": %zu, "
             "\"outer_rounds_vesta\": %zu, \"inner_rounds_vesta\": %zu, \"open_ms_pallas\": %.3f, \"open_ms_vesta\": %.3f, \"ipa_rounds_pallas\": %zu, "
             "\"ipa_rounds_vesta\": %zu, \"doc_log\": %d, \"hyrax_left\": %zu, \"consistency_ms\": %.3f, \"consistency_rounds\": %zu, "
             "\"commit_hyrax_ms\": %.3f, \"hyrax_create_ms\": %.3f, \"total_prove_device_ms\": %.3f, "
             "\"timed\": \"first instance, folding steps (N2 sum-check step, comm_W, commit_T, challenge, fold per curve), last fold, Spartan and opening per curve, "
             "consistency argument; host glue included; witness and matrix generation, the document commitment and the checks excluded\", "
             "\"check_ms\": %.3f, \"points_checked\": %d, \"proof_checked\": true, "
             "\"verify_evals_ms_pallas\": %.3f, \"verify_evals_ms_vesta\": %.3f, \"verify_evals_host_ms_pallas\": %.3f, \"verify_evals_host_ms_vesta\": %.3f, "
             "\"verify_evals\": \"A~, B~, C~ at the recorded (r_x, r_y): reef_spartan_eval_matrices host to host (second call; eq tables included) against the loop "
             "of the host check on one core (eq tables included); A~ + r B~ + r^2 C~ equals claims_inner[0] and the host's value; neither this nor verify_ipa_ms (InnerProductArgument::verify on the opening) is in total_prove_device_ms\", "
             "\"verify_ipa_ms_pallas\": %.3f, \"verify_ipa_ms_vesta\": %.3f, \"device_verified\": true%s}",
             sh->name.c_str(), sh->w1, sh->c1, sh->w2, sh->c2, P.ncp, P.nvp, V.ncp, V.nvp, P.n, V.n, P.S.nnz(), V.S.nnz(), sh->steps, P.init_ms + V.init_ms,
             steps_list.c_str(), steps_total / ns, commit_w_ms / ns, nifs_ms / ns, sc_ms / ns, final_fold_ms, P.spartan_ms, V.spartan_ms, P.pf.outer.size(),
             P.pf.inner.size(), V.pf.outer.size(), V.pf.inner.size(), P.open_ms, V.open_ms, P.pf.r_rounds.size(), V.pf.r_rounds.size(), sh->doc_log, left,
             consistency_ms, hpf.r_rounds.size(), commit_hyrax_ms, hyrax_create_ms, total, check_ms, g_checked, P.verify_evals_ms, V.verify_evals_ms,
             P.verify_evals_host_ms, V.verify_evals_host_ms, P.verify_ipa_ms, V.verify_ipa_ms, paired ? ", \"paired\": true" : "");
    return std::string(line.data());
}
