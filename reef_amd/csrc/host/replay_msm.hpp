// replay_msm.hpp -- the MSM replay of reef_replay.cpp (reef_replay_run): the discrete-logarithm check, the IPA drivers, the work
// around the MSMs, the multi-device leg and the replay of one config.
#pragma once
#include "replay_util.hpp"

// ---- host-side check: discrete logarithm of an MSM over generators in arithmetic progression ------------------
struct Big { uint64_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0}; };
static void big_addmul(Big &a, const uint64_t s[4], uint64_t m) {   // a += s * m
    unsigned __int128 carry = 0;
    for (int i = 0; i < 8; ++i) {
        unsigned __int128 t = (unsigned __int128)a.w[i] + carry + (i < 4 ? (unsigned __int128)s[i] * m : 0);
        a.w[i] = (uint64_t)t;
        carry = t >> 64;
    }
}
static Big big_shifted(const uint64_t r[4], int shift) {   // r << shift
    Big b;
    const int ws = shift / 64, bs = shift % 64;
    for (int i = 0; i < 4; ++i) {
        if (i + ws < 8) b.w[i + ws] |= r[i] << bs;
        if (bs && i + ws + 1 < 8) b.w[i + ws + 1] |= r[i] >> (64 - bs);
    }
    return b;
}
static int big_cmp_shifted(const Big &a, const uint64_t r[4], int shift) {   // a <=> r << shift
    const Big b = big_shifted(r, shift);
    for (int i = 7; i >= 0; --i)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
    return 0;
}
static void big_sub_shifted(Big &a, const uint64_t r[4], int shift) {
    const Big b = big_shifted(r, shift);
    unsigned __int128 borrow = 0;
    for (int i = 0; i < 8; ++i) {
        unsigned __int128 t = (unsigned __int128)a.w[i] - b.w[i] - borrow;
        a.w[i] = (uint64_t)t;
        borrow = (t >> 64) & 1;
    }
}
// (sum_i canon[i] * (k0 + i*d)) mod r as a canonical 4-limb scalar
static reef_fe dlog_of_msm(int curve, const reef_fe *canon, size_t n, uint64_t k0, uint64_t d) {
    Big acc;
    for (size_t i = 0; i < n; ++i) big_addmul(acc, canon[i].l, k0 + (uint64_t)i * d);
    for (int shift = 511 - 255; shift >= 0; --shift)
        if (big_cmp_shifted(acc, ORDER[curve], shift) >= 0) big_sub_shifted(acc, ORDER[curve], shift);
    reef_fe r;
    for (int i = 0; i < 4; ++i) r.l[i] = acc.w[i];
    return r;
}

struct Curve {
    int id;
    reef_msm_ctx *key = nullptr;      // pre-shifted resident commitment key
    reef_msm_ctx *ipa[2] = {nullptr, nullptr};  // plain contexts re-keyed every IPA round
    reef_affine *d_gens = nullptr;    // device copy of the key for the IPA
    size_t n = 0;
    uint64_t k0 = 0, d = 0;           // generators B_i = (k0 + i*d)*G
    reef_msm_ctx *one = nullptr;      // the one-point key [G]: turns an expected discrete logarithm into a point
};
static int g_checked = 0;
// whether `got` is dlog*G (both normalised to affine; dlog canonical, or in Montgomery form with is_mont); counts the points that are
static bool is_dlog_point(Curve &c, const reef_jacobian &got, const reef_fe &dlog, bool is_mont) {
    reef_jacobian both[2] = {got, {}};
    CK(reef_msm(c.one, &dlog, 1, REEF_HOST, is_mont, &both[1], REEF_HOST));
    reef_affine aff[2];
    CK(reef_normalize(c.id, both, 2, REEF_HOST, aff, nullptr));
    const bool same = memcmp(&aff[0], &aff[1], sizeof(reef_affine)) == 0;
    g_checked += same;
    return same;
}
static void check_point(Curve &c, const reef_jacobian &got, const reef_fe &dlog, const char *what) {   // the MSM replay aborts on a mismatch
    if (!is_dlog_point(c, got, dlog, false)) fail(std::string("reef_replay: ") + what + " on curve " + std::to_string(c.id) + " differs from its discrete-logarithm closed form");
}

// the one-point key [G] of a curve, on the caller's device (the caller owns it)
static reef_msm_ctx *one_point_key(int curve) {
    reef_affine g1;
    CK(reef_gen_bases(curve, 1, 0, 1, &g1, REEF_HOST));           // 1*G
    reef_msm_opts og = {};
    og.bucket_groups = 1;
    og.device = -1;
    reef_msm_ctx *one = nullptr;
    CK(reef_msm_ctx_create(&one, curve, &g1, 1, REEF_HOST, &og));
    return one;
}

static dev_ptr<reef_fe> device_scalars(int curve, uint64_t seed, int kind, size_t n) {
    dev_ptr<reef_fe> p = device_alloc<reef_fe>(n);
    CK(reef_gen_scalars(curve, seed, kind, 0, n, true, p.get(), REEF_DEVICE));
    return p;
}

// One IPA without generator folding: every round's cross terms are two MSMs over the ORIGINAL
// pre-shifted key with scalars a[.] * prod(challenges) (reef_ipa_cross_terms); the vector fold
// a' = r*a_lo + r^-1*a_hi is field-only host work in nova and is not replayed.
static double run_ipa_nofold(Curve &c, size_t n, const reef_fe *d_scalars, int *rounds_out) {
    auto t0 = clk::now();
    std::vector<reef_fe> w1s, w2s;
    reef_jacobian L, R;
    int rounds = 0;
    for (size_t len = n; len > 1; len /= 2, ++rounds) {
        CK(reef_ipa_cross_terms(c.key, d_scalars, len, REEF_DEVICE, true, w1s.data(), w2s.data(), w1s.size(), &L, &R));
        reef_fe w1 = {{0x1234567890abcdefULL + rounds, 0x0fedcba987654321ULL, 0x1111111122222222ULL, 0x0333333344444444ULL}};
        reef_fe w2 = {{0x0badc0ffee0ddf00ULL + rounds, 0x0123456789abcdefULL, 0x5555555566666666ULL, 0x0777777788888888ULL}};
        w1s.push_back(w1);
        w2s.push_back(w2);
    }
    if (rounds_out) *rounds_out = rounds;
    return ms_since(t0);
}

// One IPA: log2(n) rounds, two cross MSMs of n/2 points on two streams + the generator fold.
static double run_ipa(Curve &c, size_t n, const reef_fe *d_scalars, int *rounds_out) {
    auto t0 = clk::now();
    reef_affine *cur = c.d_gens;
    dev_ptr<reef_affine> buf[2] = {device_alloc<reef_affine>(n / 2 + 1), device_alloc<reef_affine>(n / 2 + 1)};
    reef_jacobian L, R;
    reef_fe w1 = {{0x1234567890abcdefULL, 0x0fedcba987654321ULL, 0x1111111122222222ULL, 0x0333333344444444ULL}};
    reef_fe w2 = {{0x0badc0ffee0ddf00ULL, 0x0123456789abcdefULL, 0x5555555566666666ULL, 0x0777777788888888ULL}};
    int rounds = 0, flip = 0;
    for (size_t len = n; len > 1; len /= 2, ++rounds) {
        const size_t half = len / 2;
        CK(reef_msm_ctx_set_bases(c.ipa[0], cur + half, half, REEF_DEVICE));   // L = <a_lo, G_hi>
        CK(reef_msm_ctx_set_bases(c.ipa[1], cur, half, REEF_DEVICE));          // R = <a_hi, G_lo>
        // the cross terms feed the transcript, so they go straight to the host: for keys without
        // pre-shifted tables the library then finishes the window combine on a host core
        CK(reef_msm(c.ipa[0], d_scalars, half, REEF_DEVICE, true, &L, REEF_HOST));
        CK(reef_msm(c.ipa[1], d_scalars + half, half, REEF_DEVICE, true, &R, REEF_HOST));
        CK(reef_fold(c.id, cur, half, REEF_DEVICE, &w1, &w2, buf[flip].get()));   // G' = w1*G_lo + w2*G_hi
        cur = buf[flip].get();
        flip ^= 1;
    }
    if (rounds_out) *rounds_out = rounds;
    return ms_since(t0);
}

// ---- the work around the MSMs that this backend also covers -------------------------------------
// --commit: HyraxPC::commit over the document matrix (commitment.rs:187), from the document bytes.
// per step: the nlookup sum-check of witness generation (r1cs.rs:2318-2385) as reef_sc_* rounds, the
//           Poseidon challenge of every round replaced by a fixed field element (it stays on the host).
// proof end: doc_poly.evaluate / the row binding of prove_eval (commitment.rs:357,371-391).
static std::vector<uint8_t> host_symbols(size_t n, int bits, uint64_t seed) {
    std::vector<uint8_t> h(n);
    uint64_t x = seed;
    const uint32_t bound = bits >= 8 ? 131u : (bits == 3 ? 7u : (1u << bits));
    for (size_t i = 0; i < n; ++i) {
        x = x * 6364136223846793005ULL + 1442695040888963407ULL;
        h[i] = (uint8_t)((x >> 33) % bound);
    }
    return h;
}
static dev_ptr<uint8_t> device_symbols(size_t n, int bits, uint64_t seed) {
    const std::vector<uint8_t> h = host_symbols(n, bits, seed);
    dev_ptr<uint8_t> d = device_alloc<uint8_t>(n);
    CK(reef_memcpy(d.get(), h.data(), n, REEF_DEVICE, REEF_HOST));
    return d;
}

static double run_hyrax_commit(const Shape *sh, reef_affine *d_gens, const uint8_t *d_doc, double *first_ms) {
    const size_t rows = (size_t)1 << (sh->doc_log / 2), row_len = (size_t)1 << (sh->doc_log - sh->doc_log / 2);
    reef_msm_ctx *key = nullptr;
    CK(reef_msm_ctx_create(&key, REEF_PALLAS, d_gens, row_len, REEF_DEVICE, nullptr));
    const ctx_ptr key_owner(key);
    const dev_ptr<reef_jacobian> d_out_owner = device_alloc<reef_jacobian>(rows);
    reef_jacobian *d_out = d_out_owner.get();
    auto t0 = clk::now();
    CK(reef_msm_rows_symbols(key, d_doc, rows, row_len, REEF_DEVICE, (uint32_t)sh->symbol_bits, nullptr, nullptr, true, d_out, REEF_DEVICE));
    CK(reef_msm_ctx_sync(key));
    *first_ms = ms_since(t0);                          // includes the construction of the symbol tables
    t0 = clk::now();
    CK(reef_msm_rows_symbols(key, d_doc, rows, row_len, REEF_DEVICE, (uint32_t)sh->symbol_bits, nullptr, nullptr, true, d_out, REEF_DEVICE));
    CK(reef_msm_ctx_sync(key));
    return ms_since(t0);
}

static double run_sumcheck_step(reef_sc_ctx *sc, int ell, int lookups) {
    std::vector<reef_fe> rs(lookups + 1), last_q(ell);
    std::vector<uint32_t> qs(lookups);
    for (int i = 0; i <= lookups; ++i) rs[i] = reef_fe{{0x9e3779b97f4a7c15ULL * (i + 1), 0x1234ULL + i, 0, 0}};
    for (int i = 0; i < lookups; ++i) qs[i] = (uint32_t)((0x2545F4914F6CDD1DULL * (i + 7)) >> (64 - ell));
    for (int j = 0; j < ell; ++j) last_q[j] = reef_fe{{0xabcdef12345ULL + j, 0x77ULL * j, 0, 0}};
    auto t0 = clk::now();
    CK(reef_sc_reset_table(sc));
    CK(reef_sc_gen_eq_table(sc, rs.data(), qs.data(), lookups, last_q.data(), ell));
    reef_fe g[3];
    CK(reef_sc_round_coeffs(sc, (size_t)1 << (ell - 1), g));
    for (int i = 1; i <= ell; ++i) {
        const reef_fe r = {{0x5851f42d4c957f2dULL + i, 0x14057b7ef767814fULL, 0x0123456789abcdefULL, 0x0fedcba987654321ULL}};
        const size_t pow = (size_t)1 << (ell - i);
        if (pow >= 2) CK(reef_sc_fold_and_next_coeffs(sc, pow, &r, g));
        else CK(reef_sc_fold(sc, pow, &r));
    }
    reef_fe v;
    CK(reef_sc_read(sc, 0, 1, &v));                    // next_running_v (r1cs.rs:2379-2385)
    return ms_since(t0);
}

// The nlookup table of one config on a resident sum-check context (rows N2; sh->table_log > 0)
static sc_ptr sumcheck_ctx(const Shape *sh) {
    const size_t len = (size_t)1 << sh->table_log;
    reef_sc_ctx *sc = nullptr;
    CK(reef_sc_create(&sc, REEF_PALLAS, len));
    sc_ptr sc_owner(sc);
    dev_ptr<reef_fe> tab_owner = device_alloc<reef_fe>(len);
    reef_fe *d_tab = tab_owner.get();
    // the table as Reef builds it (canonical integers): --hybrid puts the transition table and then ONE value (`calc_fill`)
    // in the public half and the document in the private half (r1cs.rs:481-484, :2105-2112); otherwise it is the document
    const uint64_t sym_bound = 1ull << sh->symbol_bits;
    if (sh->table_log == sh->doc_log + 1) {
        const size_t half = len / 2, trans = std::min<size_t>(256, half / 2);
        CK(reef_gen_scalars(REEF_PALLAS, 0x7AB1E, 0, 0, trans, false, d_tab, REEF_DEVICE));
        const reef_fe fill = {{0x123456789abcdef1ULL, 0x0fedcba987654321ULL, 0x1111111122222222ULL, 0x0333333344444444ULL}};
        CK(reef_memcpy(d_tab + trans, &fill, sizeof fill, REEF_DEVICE, REEF_HOST));
        for (size_t have = 1; trans + have < half; have *= 2)
            CK(reef_memcpy(d_tab + trans + have, d_tab + trans, std::min(have, half - trans - have) * sizeof(reef_fe), REEF_DEVICE, REEF_DEVICE));
        CK(reef_gen_scalars(REEF_PALLAS, 0xD0C, 2, sym_bound, half, false, d_tab + half, REEF_DEVICE));
    } else {
        CK(reef_gen_scalars(REEF_PALLAS, 0xD0C, 2, sym_bound, len, false, d_tab, REEF_DEVICE));
    }
    CK(reef_sc_set_table(sc, 0, d_tab, len, REEF_DEVICE));
    return sc_owner;
}

// ---- the multi-device leg: what ONE prover process can hand to the other GPUs of its node (include/reef_msm.h section 5) ----
// Reef's per-step MSMs are 2^14-2^16 points and are not split.  What a node can take from a --prove run is WHOLE units:
//   * the final SNARK's three arguments (two Spartan IPAs, the consistency IPA; src/backend/framework.rs:695-721) on up to three
//     devices, each argument's key and scalars resident on its device (reef_msm_opts.device), issued from three caller threads;
//   * the Hyrax commitment of the document (src/backend/commitment.rs:187) through a device group (reef_msm_group_rows_symbols:
//     rows dealt out whole, the document in host memory as Reef holds it), checked row for row against one device.
// `ordinals` may repeat a device (a one-GPU box runs the whole leg on device 0; the JSON says how many devices were distinct).
struct DeviceScope {
    int prev = 0;
    explicit DeviceScope(int dev) {
        CK(reef_get_device(&prev));
        CK(reef_set_device(dev));
    }
    ~DeviceScope() { (void)reef_set_device(prev); }
};
struct GroupFree { void operator()(reef_msm_group *p) const { if (p) reef_msm_group_destroy(p); } };
static std::string replay_devices(const Shape &shape, const std::vector<int> &ordinals, bool tables) {
    const Shape *sh = &shape;
    const size_t nd = ordinals.size();
    std::vector<int> uniq(ordinals);
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    struct Arg { const char *name; Curve c; int device; dev_ptr<reef_affine> gens; dev_ptr<reef_fe> sc; ctx_ptr key; double alone_ms = 0; };
    std::vector<Arg> args(3);
    args[0].name = "ipa_pallas"; args[0].c.id = REEF_PALLAS; args[0].c.n = next_pow2(std::max(sh->w1, sh->c1));
    args[1].name = "ipa_vesta";  args[1].c.id = REEF_VESTA;  args[1].c.n = next_pow2(std::max(sh->w2, sh->c2));
    args[2].name = "consistency"; args[2].c.id = REEF_PALLAS; args[2].c.n = sh->hyrax_row;
    if (sh->hyrax_row < 2) args.pop_back();
    // longest argument first onto the least loaded device (deterministic; the same rule as reef_amd/distributed.py::place_units)
    std::vector<size_t> order(args.size());
    for (size_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return args[a].c.n > args[b].c.n; });
    std::vector<double> load(nd, 0.0);
    for (size_t k : order) {
        size_t best = 0;
        for (size_t d = 1; d < nd; ++d)
            if (load[d] < load[best]) best = d;
        args[k].device = ordinals[best];
        load[best] += (double)args[k].c.n;
    }
    for (Arg &a : args) {
        DeviceScope ds(a.device);
        a.gens = device_alloc<reef_affine>(a.c.n);
        CK(reef_gen_bases(a.c.id, 0xC0FFEE + a.c.id, 7, a.c.n, a.gens.get(), REEF_DEVICE));
        a.sc = device_scalars(a.c.id, 12 + a.c.id, 0, a.c.n);
        const reef_msm_opts o = fixed_key_opts(tables, a.device);
        CK(reef_msm_ctx_create(&a.c.key, a.c.id, a.gens.get(), a.c.n, REEF_DEVICE, &o));
        a.key.reset(a.c.key);
        run_ipa_nofold(a.c, a.c.n, a.sc.get(), nullptr);                     // warm-up: workspaces
        a.alone_ms = run_ipa_nofold(a.c, a.c.n, a.sc.get(), nullptr);
    }
    const double together_ms = run_together(args.size(), [&](size_t k) { run_ipa_nofold(args[k].c, args[k].c.n, args[k].sc.get(), nullptr); });
    // the document commitment over the group, against one device
    double commit_group_ms = 0, commit_one_ms = 0;
    reef_msm_group_info gi;
    memset(&gi, 0, sizeof gi);
    if (sh->doc_log) {
        const size_t n_doc = (size_t)1 << sh->doc_log;
        const size_t rows = (size_t)1 << (sh->doc_log / 2), row_len = (size_t)1 << (sh->doc_log - sh->doc_log / 2);
        const std::vector<uint8_t> doc = host_symbols(n_doc, sh->symbol_bits, 0xD0C);
        std::vector<reef_affine> gens(row_len);
        CK(reef_gen_bases(REEF_PALLAS, 0xFEED, 3, row_len, gens.data(), REEF_HOST));
        reef_msm_group *grp = nullptr;
        reef_msm_group_opts go = {};
        go.split = REEF_SPLIT_WINDOWS;
        CK(reef_msm_group_create(&grp, REEF_PALLAS, gens.data(), row_len, REEF_HOST, nullptr, ordinals.data(), nd, &go));
        const std::unique_ptr<reef_msm_group, GroupFree> grp_owner(grp);
        CK(reef_msm_group_info_get(grp, &gi));
        std::vector<reef_jacobian> out_g(rows), out_1(rows);
        CK(reef_msm_group_rows_symbols(grp, doc.data(), rows, row_len, REEF_HOST, (uint32_t)sh->symbol_bits, nullptr, nullptr, true, out_g.data()));   // builds the symbol tables
        // the median of five: the first pageable copy a pool stream carries pays for the runtime's staging buffers (one-off, 5-20 ms),
        // and the members take whichever stream is least busy
        auto median5 = [&](const std::function<void()> &f) {
            double t[5];
            for (double &x : t) { auto t0 = clk::now(); f(); x = ms_since(t0); }
            std::sort(t, t + 5);
            return t[2];
        };
        commit_group_ms = median5([&] { CK(reef_msm_group_rows_symbols(grp, doc.data(), rows, row_len, REEF_HOST, (uint32_t)sh->symbol_bits, nullptr, nullptr, true, out_g.data())); });
        reef_msm_ctx *one = nullptr;
        reef_msm_opts o1 = {};
        o1.device = ordinals[0];
        CK(reef_msm_ctx_create(&one, REEF_PALLAS, gens.data(), row_len, REEF_HOST, &o1));
        const ctx_ptr one_owner(one);
        CK(reef_msm_rows_symbols(one, doc.data(), rows, row_len, REEF_HOST, (uint32_t)sh->symbol_bits, nullptr, nullptr, true, out_1.data(), REEF_HOST));
        commit_one_ms = median5([&] { CK(reef_msm_rows_symbols(one, doc.data(), rows, row_len, REEF_HOST, (uint32_t)sh->symbol_bits, nullptr, nullptr, true, out_1.data(), REEF_HOST)); });
        std::vector<reef_affine> ag(rows), a1(rows);
        CK(reef_normalize(REEF_PALLAS, out_g.data(), rows, REEF_HOST, ag.data(), nullptr));
        CK(reef_normalize(REEF_PALLAS, out_1.data(), rows, REEF_HOST, a1.data(), nullptr));
        if (memcmp(ag.data(), a1.data(), rows * sizeof(reef_affine)) != 0) fail("reef_replay: the group's row commitments differ from one device's");
    }
    // --merkle: the Poseidon tree of the document in blocks over the devices (reef_merkle_commit_devices), root against one device's
    double merkle_devices_ms = 0, merkle_one_ms = 0;
    uint32_t merkle_blocks = 0;
    if (sh->merkle_log) {
        const size_t n_doc = (size_t)1 << sh->merkle_log;
        std::vector<uint32_t> doc(n_doc);
        for (size_t i = 0; i < n_doc; ++i) doc[i] = (uint32_t)((i * 2654435761u) >> 24);
        const reef_poseidon_params pp = standin_poseidon();
        reef_fe root_d, root_1;
        CK(reef_merkle_commit_devices(REEF_PALLAS, &pp, doc.data(), std::min(n_doc, (size_t)1 << 16), false, ordinals.data(), nd, nullptr, &root_d, nullptr));      // warm-up (never beyond the document)
        auto t0 = clk::now();
        CK(reef_merkle_commit_devices(REEF_PALLAS, &pp, doc.data(), n_doc, false, ordinals.data(), nd, nullptr, &root_d, &merkle_blocks));
        merkle_devices_ms = ms_since(t0);
        t0 = clk::now();
        CK(reef_merkle_commit(REEF_PALLAS, &pp, doc.data(), n_doc, REEF_HOST, false, nullptr, REEF_HOST, &root_1));
        merkle_one_ms = ms_since(t0);
        if (memcmp(&root_d, &root_1, sizeof root_1) != 0) fail("reef_replay: the Merkle commitment built in blocks differs from one device's");
    }
    double sum_alone = 0, longest = 0;
    for (Arg &a : args) { sum_alone += a.alone_ms; longest = std::max(longest, a.alone_ms); }
    std::string placed = "[";
    for (size_t k = 0; k < args.size(); ++k) {
        char b[160];
        snprintf(b, sizeof b, "%s{\"argument\": \"%s\", \"points\": %zu, \"device\": %d, \"alone_ms\": %.3f}", k ? ", " : "", args[k].name, args[k].c.n, args[k].device, args[k].alone_ms);
        placed += b;
    }
    placed += "]";
    std::vector<char> line(4096);
    snprintf(line.data(), line.size(), "{\"members\": %zu, \"distinct_devices\": %zu, \"visible_devices\": %d, \"note\": \"one process: the final SNARK's arguments placed whole on the devices "
             "(per-device contexts, one caller thread each), the document commitment through a device group; ordinals repeat when the box has fewer GPUs than members\", "
             "\"final_snark_placed\": %s, \"three_arguments_one_after_the_other_ms\": %.3f, \"three_arguments_on_devices_ms\": %.3f, \"longest_argument_ms\": %.3f, "
             "\"commit_hyrax_group_ms\": %.3f, \"commit_hyrax_one_device_ms\": %.3f, \"commit_rows_checked_against_one_device\": %s, \"group_exchange\": \"%s\", \"group_peer_members\": %u, "
             "\"commit_merkle_devices_ms\": %.3f, \"commit_merkle_one_device_ms\": %.3f, \"commit_merkle_blocks\": %u, \"commit_merkle_root_checked_against_one_device\": %s}",
             nd, uniq.size(), reef_device_count(), placed.c_str(), sum_alone, together_ms, longest, commit_group_ms, commit_one_ms, sh->doc_log ? "true" : "false",
             gi.exchange == REEF_EXCHANGE_HOST ? "host-staged" : "peer copies (hipMemcpyPeerAsync; in place on a shared device)", gi.peer_members,
             merkle_devices_ms, merkle_one_ms, merkle_blocks, sh->merkle_log ? "true" : "false");
    return std::string(line.data());
}

// ---- the replay of one config: its state, and one member function per stage, run by replay_body in the order they stand here ----
struct HostVec { std::vector<reef_fe> mont, canon; };   // scalars in HOST memory: Montgomery form (what nova holds) and canonical integers (for the check)
static HostVec host_vec(int curve, uint64_t seed, int kind, size_t n) {
    HostVec v{std::vector<reef_fe>(n), std::vector<reef_fe>(n)};
    CK(reef_gen_scalars(curve, seed, kind, 0, n, true, v.mont.data(), REEF_HOST));
    CK(reef_gen_scalars(curve, seed, kind, 0, n, false, v.canon.data(), REEF_HOST));
    return v;
}
struct MsmReplay {
    const Shape *sh;
    const bool nofold, tables;
    Curve cv[2];
    std::vector<dev_ptr<reef_affine>> owned_gens;       // destroyed after the contexts below
    std::vector<ctx_ptr> owned_ctx;
    dev_ptr<reef_fe> oW1, oT1, oW2, oT2;                // witness-like scalars for W, uniform for the cross terms T, on the device (the IPAs read T)
    HostVec hW1, hT1, hW2, hT2;                         // the same vectors in host memory
    reef_fe eW1, eT1, eW2, eT2;                         // expected discrete logarithms of the four per-step commitments
    int timed_steps = 0;
    Curve hy; ctx_ptr hy_owner;                         // the consistency argument's key
    double setup_first_ms = 0, setup_ms = 0, check_keys_ms = 0, steps_ms = 0, steps_batched_ms = 0, steps_conc_ms = 0, steps_all4_ms = 0;
    double final_ms = 0, ipa1_ms = 0, ipa2_ms = 0, cons_ms = 0, concurrent_ms = 0;
    int r1 = 0, r2 = 0, r3 = 0;
    double commit_ms = 0, commit_first_ms = 0, sc_step_ms = 0, mle_ms = 0, merkle_ms = 0;

    MsmReplay(const Shape &shape, bool nofold_, bool tables_) : sh(&shape), nofold(nofold_), tables(tables_) {
        cv[0].id = REEF_PALLAS; cv[0].n = next_pow2(sh->w1 > sh->c1 ? sh->w1 : sh->c1);
        cv[1].id = REEF_VESTA;  cv[1].n = next_pow2(sh->w2 > sh->c2 ? sh->w2 : sh->c2);
    }
    // ---- set-up as a --prove run pays it.  Reef derives its commitment keys from their labels on EVERY run (src/backend/framework.rs:115,
    // 297-303 -> CommitmentGens::new), so set-up is prove time: per curve, on a caller thread of its own -- the two curves at
    // once -- label -> n generators on the device (row N1: reef_derive_generators; stand-in hash-to-curve parameters, replay_standins.h) ->
    // resident pre-shifted key straight from the device buffer (reef_msm_ctx_create): what CommitmentGens(label, n, params) of
    // reef_provider.hpp does.  Timed twice: setup_first_ms is the first pass in this process (first launches of the kernels, the
    // workspaces' allocations), setup_ms the second.  The keys built here are dropped again: the MSMs below run on keys of the same
    // sizes whose generators are an arithmetic progression (so that every commitment has a known discrete logarithm), built after the
    // clock has stopped (check_keys_ms).
    void derive_key(int k) {
        const int id = cv[k].id;
        reef_keygen_params kp;
        const reef_fe *sp = id == REEF_PALLAS ? STANDIN_KEYGEN_0 : STANDIN_KEYGEN_1;
        const char *dst = id == REEF_PALLAS ? STANDIN_KEYGEN_DST_0 : STANDIN_KEYGEN_DST_1;
        kp.a = sp[0]; kp.b = sp[1]; kp.z = sp[2];
        memcpy(kp.iso, sp + 3, 13 * sizeof(reef_fe));
        kp.dst = (const uint8_t *)dst; kp.dst_len = (uint32_t)strlen(dst); kp.little_endian = 0;
        const dev_ptr<reef_affine> gens = device_alloc<reef_affine>(cv[k].n);
        CK(reef_derive_generators(id, (const uint8_t *)"ck", 2, cv[k].n, &kp, false, gens.get(), REEF_DEVICE));
        const reef_msm_opts o = fixed_key_opts(tables, -1);
        reef_msm_ctx *key = nullptr;
        CK(reef_msm_ctx_create(&key, id, gens.get(), cv[k].n, REEF_DEVICE, &o));
        const ctx_ptr owner(key);
        CK(reef_msm_ctx_sync(key));
    }
    void setup() {
        auto derive_both = [&] { return run_together(2, [&](size_t k) { derive_key((int)k); }); };
        setup_first_ms = derive_both();
        setup_ms = derive_both();
    }
    // the keys the MSMs run on: generators in arithmetic progression, and per curve the one-point key the checks turn a logarithm into a point with
    void check_keys() {
        auto t_check_keys = clk::now();
        for (Curve &c : cv) {
            owned_gens.push_back(device_alloc<reef_affine>(c.n));
            c.d_gens = owned_gens.back().get();
            c.k0 = 0xC0FFEE + c.id; c.d = 7;
            CK(reef_gen_bases(c.id, c.k0, c.d, c.n, c.d_gens, REEF_DEVICE));
            c.one = one_point_key(c.id);
            owned_ctx.emplace_back(c.one);
            const reef_msm_opts o = fixed_key_opts(tables, -1);
            CK(reef_msm_ctx_create(&c.key, c.id, c.d_gens, c.n, REEF_DEVICE, &o));
            owned_ctx.emplace_back(c.key);
            CK(reef_msm_ctx_sync(c.key));
            reef_msm_opts plain = {}; plain.device = -1;
            if (!nofold)   // the per-round re-keyed contexts exist only in the generator-fold IPA
                for (auto &x : c.ipa) { CK(reef_msm_ctx_create(&x, c.id, c.d_gens, c.n / 2, REEF_DEVICE, &plain)); owned_ctx.emplace_back(x); }
        }
        check_keys_ms = ms_since(t_check_keys);
    }
    // host scalars in, commitment back to the host: it feeds the next circuit
    reef_jacobian msm(Curve &c, const HostVec &s, size_t n) {
        reef_jacobian out;
        CK(reef_msm(c.key, s.mont.data(), n, REEF_HOST, true, &out, REEF_HOST));
        return out;
    }
    // the scalar vectors, their expected commitments (computed once, outside the timed loops), the warm-up and the first check
    void scalars() {
        oW1 = device_scalars(REEF_PALLAS, 11, 1, cv[0].n); oT1 = device_scalars(REEF_PALLAS, 12, 0, cv[0].n);
        oW2 = device_scalars(REEF_VESTA, 13, 1, cv[1].n); oT2 = device_scalars(REEF_VESTA, 14, 0, cv[1].n);
        hW1 = host_vec(REEF_PALLAS, 11, 1, cv[0].n); hT1 = host_vec(REEF_PALLAS, 12, 0, cv[0].n);
        hW2 = host_vec(REEF_VESTA, 13, 1, cv[1].n); hT2 = host_vec(REEF_VESTA, 14, 0, cv[1].n);
        eW1 = dlog_of_msm(0, hW1.canon.data(), sh->w1, cv[0].k0, cv[0].d); eT1 = dlog_of_msm(0, hT1.canon.data(), sh->c1, cv[0].k0, cv[0].d);
        eW2 = dlog_of_msm(1, hW2.canon.data(), sh->w2, cv[1].k0, cv[1].d); eT2 = dlog_of_msm(1, hT2.canon.data(), sh->c2, cv[1].k0, cv[1].d);
        check_point(cv[0], msm(cv[0], hW1, sh->w1), eW1, "comm_W1");   // warm-up (workspace allocation)
        check_point(cv[1], msm(cv[1], hW2, sh->w2), eW2, "comm_W2");
        // a config may fold in a single step: time at least three so that the per-step figure is not one sample; the totals
        // charge the config's own number of steps
        timed_steps = sh->steps < 3 ? 3 : sh->steps;
    }
    // the four commitments of a folding step, one call after the other
    void fold_steps() {
        std::vector<double> step_ms;
        for (int i = 0; i < timed_steps; ++i) {
            auto ts = clk::now();
            reef_jacobian o[4];
            o[0] = msm(cv[1], hT2, sh->c2);
            o[1] = msm(cv[0], hW1, sh->w1);
            o[2] = msm(cv[0], hT1, sh->c1);
            o[3] = msm(cv[1], hW2, sh->w2);
            step_ms.push_back(ms_since(ts));
            check_point(cv[1], o[0], eT2, "comm_T2");           // outside the step's timing
            check_point(cv[0], o[1], eW1, "comm_W1");
            check_point(cv[0], o[2], eT1, "comm_T1");
            check_point(cv[1], o[3], eW2, "comm_W2");
        }
        for (double v : step_ms) steps_ms += v;
        steps_ms = steps_ms / timed_steps * sh->steps;
    }
    // The same commitments with the two of each curve issued as ONE batched call (comm_W and comm_T of a
    // step are both absorbed before the folding challenge is drawn, so neither needs the other): rows = 2
    // over the same resident key share one pass of the pipeline.  Needs prove_step to hand both vectors
    // over together; reported next to the call-by-call figure, not instead of it.
    void batched_pairs() {
        const size_t len[2] = {sh->w1 > sh->c1 ? sh->w1 : sh->c1, sh->w2 > sh->c2 ? sh->w2 : sh->c2};
        std::vector<reef_fe> hostbuf[2];
        const HostVec *hv[2][2] = {{&hW1, &hT1}, {&hW2, &hT2}};
        reef_fe expect[2][2];
        for (int k = 0; k < 2; ++k) {
            hostbuf[k].resize(2 * len[k]);                // the two vectors of a curve side by side in host memory
            memcpy(hostbuf[k].data(), hv[k][0]->mont.data(), len[k] * sizeof(reef_fe));
            memcpy(hostbuf[k].data() + len[k], hv[k][1]->mont.data(), len[k] * sizeof(reef_fe));
            for (int j = 0; j < 2; ++j) expect[k][j] = dlog_of_msm(k, hv[k][j]->canon.data(), len[k], cv[k].k0, cv[k].d);
        }
        reef_jacobian two[2];
        auto both = [&](int k) { CK(reef_msm_rows(cv[k].key, hostbuf[k].data(), 2, len[k], REEF_HOST, true, 255, nullptr, nullptr, two, REEF_HOST)); };
        for (int k = 0; k < 2; ++k) {                    // warm-up and check
            both(k);
            check_point(cv[k], two[0], expect[k][0], "batched comm_W");
            check_point(cv[k], two[1], expect[k][1], "batched comm_T");
        }
        auto tb = clk::now();
        for (int i = 0; i < timed_steps; ++i) { both(1); both(0); }
        steps_batched_ms = ms_since(tb) / timed_steps * sh->steps;
    }
    // The pair of a curve issued as two CONCURRENT MSMs instead (reef_msm_multi: both enqueued, then both waited for; the second
    // commitment runs on a clone of the key, i.e. on another stream of the library's pool), and -- an upper bound only, because
    // the two curves of a step depend on each other through the step circuits -- all four at once.
    void concurrent_pairs() {
        reef_msm_ctx *cl[2] = {nullptr, nullptr};
        for (int k = 0; k < 2; ++k) { CK(reef_msm_ctx_clone(&cl[k], cv[k].key)); owned_ctx.emplace_back(cl[k]); }
        reef_msm_ctx *pair_ctx[2][2] = {{cv[0].key, cl[0]}, {cv[1].key, cl[1]}};
        const reef_fe *pair_sc[2][2] = {{hW1.mont.data(), hT1.mont.data()}, {hW2.mont.data(), hT2.mont.data()}};
        const size_t pair_n[2][2] = {{sh->w1, sh->c1}, {sh->w2, sh->c2}};
        const reef_fe pair_e[2][2] = {{eW1, eT1}, {eW2, eT2}};
        reef_jacobian two[2];
        for (int k = 0; k < 2; ++k) {                    // warm-up (the clones' workspaces) and check
            CK(reef_msm_multi(2, pair_ctx[k], pair_sc[k], pair_n[k], REEF_HOST, true, two));
            check_point(cv[k], two[0], pair_e[k][0], "concurrent comm_W");
            check_point(cv[k], two[1], pair_e[k][1], "concurrent comm_T");
        }
        auto tb = clk::now();
        for (int i = 0; i < timed_steps; ++i) {
            CK(reef_msm_multi(2, pair_ctx[1], pair_sc[1], pair_n[1], REEF_HOST, true, two));
            CK(reef_msm_multi(2, pair_ctx[0], pair_sc[0], pair_n[0], REEF_HOST, true, two));
        }
        steps_conc_ms = ms_since(tb) / timed_steps * sh->steps;
        reef_msm_ctx *all_ctx[4] = {cv[1].key, cv[0].key, cl[0], cl[1]};
        const reef_fe *all_sc[4] = {hT2.mont.data(), hW1.mont.data(), hT1.mont.data(), hW2.mont.data()};
        const size_t all_n[4] = {sh->c2, sh->w1, sh->c1, sh->w2};
        reef_jacobian four[4];
        CK(reef_msm_multi(4, all_ctx, all_sc, all_n, REEF_HOST, true, four));
        check_point(cv[1], four[0], eT2, "all-four comm_T2");
        check_point(cv[0], four[2], eT1, "all-four comm_T1");
        tb = clk::now();
        for (int i = 0; i < timed_steps; ++i) CK(reef_msm_multi(4, all_ctx, all_sc, all_n, REEF_HOST, true, four));
        steps_all4_ms = ms_since(tb) / timed_steps * sh->steps;
    }
    // the last NIFS fold and the two Spartan IPAs; the consistency IPA; then the three arguments at once
    void final_snark() {
        const reef_fe *sT1 = oT1.get(), *sT2 = oT2.get();
        auto t_final = clk::now();
        msm(cv[1], hT2, sh->c2);  // last NIFS fold
        ipa1_ms = nofold ? run_ipa_nofold(cv[0], cv[0].n, sT1, &r1) : run_ipa(cv[0], cv[0].n, sT1, &r1);
        ipa2_ms = nofold ? run_ipa_nofold(cv[1], cv[1].n, sT2, &r2) : run_ipa(cv[1], cv[1].n, sT2, &r2);
        final_ms = ms_since(t_final);

        if (sh->hyrax_row >= 2) {
            hy.id = REEF_PALLAS; hy.n = sh->hyrax_row; hy.d_gens = cv[0].d_gens;  // prefix of the same key shape
            for (int k = 0; k < 2; ++k) hy.ipa[k] = cv[0].ipa[k];
            if (nofold) {   // the Hyrax row generators are a resident key of their own (commitment.rs:176-186)
                const reef_msm_opts o = fixed_key_opts(tables, -1);
                CK(reef_msm_ctx_create(&hy.key, hy.id, hy.d_gens, hy.n, REEF_DEVICE, &o));
                hy_owner.reset(hy.key);
                reef_jacobian warm_l, warm_r;
                CK(reef_ipa_cross_terms(hy.key, sT1, hy.n, REEF_DEVICE, true, nullptr, nullptr, 0, &warm_l, &warm_r));
                cons_ms = run_ipa_nofold(hy, hy.n, sT1, &r3);
            } else {
                cons_ms = run_ipa(hy, hy.n, sT1, &r3);
            }
        }

        // The two Spartan arguments (primary and secondary curve) and the consistency argument do not depend on one another: issued
        // from three caller threads at once -- what rayon::join around them does -- their latency-bound rounds share the GPU.
        if (nofold) {
            Curve *c3[3] = {&hy, &cv[0], &cv[1]};            // the consistency argument (when the config has one) on the calling thread
            const reef_fe *s3[3] = {sT1, sT1, sT2};
            concurrent_ms = run_together(3, [&](size_t k) { if (c3[k]->key) run_ipa_nofold(*c3[k], c3[k]->n, s3[k], nullptr); });
        }
    }
    // ---- commitment of the document, the per-step sum-check and the document polynomial at proof end
    void side_rows() {
        if (sh->doc_log) {
            const size_t n_doc = (size_t)1 << sh->doc_log;
            const dev_ptr<uint8_t> doc = device_symbols(n_doc, sh->symbol_bits, 0xD0C);
            const uint8_t *d_doc = doc.get();
            const size_t row_len = (size_t)1 << (sh->doc_log - sh->doc_log / 2);
            const dev_ptr<reef_affine> row_gens = device_alloc<reef_affine>(row_len);
            CK(reef_gen_bases(REEF_PALLAS, 0xFEED, 3, row_len, row_gens.get(), REEF_DEVICE));
            commit_ms = run_hyrax_commit(sh, row_gens.get(), d_doc, &commit_first_ms);
            std::vector<reef_fe> point(sh->doc_log);
            for (int j = 0; j < sh->doc_log; ++j) point[j] = reef_fe{{0x1f83d9abfb41bd6bULL + j, 0x5be0cd19137e2179ULL, 0x3c6ef372fe94f82bULL, 0x0a54ff53a5f1d36fULL}};
            std::vector<reef_fe> lz(row_len);
            reef_fe ev;
            CK(reef_mle_bound_rows(REEF_PALLAS, d_doc, n_doc, 1, REEF_DEVICE, true, point.data(), sh->doc_log, sh->doc_log / 2, lz.data(), REEF_HOST, &ev));
            auto t0 = clk::now();
            CK(reef_mle_bound_rows(REEF_PALLAS, d_doc, n_doc, 1, REEF_DEVICE, true, point.data(), sh->doc_log, sh->doc_log / 2, lz.data(), REEF_HOST, &ev));
            mle_ms = ms_since(t0);
        }
        if (sh->table_log) {
            const sc_ptr sc = sumcheck_ctx(sh);
            run_sumcheck_step(sc.get(), sh->table_log, sh->lookups);      // warm-up
            // the median of three steps: one sample read 2.5 ms instead of 1.6 now and then on a box's first large run (round 4)
            double t3[3];
            for (double &t : t3) t = run_sumcheck_step(sc.get(), sh->table_log, sh->lookups);
            std::sort(t3, t3 + 3);
            sc_step_ms = t3[1];
        }
        // ---- row N4 with STAND-IN parameters (replay_standins.h): for --merkle the Poseidon tree of the document.  Timing only: parity is
        // tests/test_gpu_merkle.py.  (Row N1, the keys derived from their labels, is the set-up above.)
        if (sh->merkle_log) {
            const size_t n_doc = (size_t)1 << sh->merkle_log;
            std::vector<uint32_t> doc(n_doc);
            for (size_t i = 0; i < n_doc; ++i) doc[i] = (uint32_t)((i * 2654435761u) >> 24);               // one-byte symbols
            const reef_poseidon_params pp = standin_poseidon();
            reef_fe root;
            CK(reef_merkle_commit(REEF_PALLAS, &pp, doc.data(), std::min(n_doc, (size_t)1 << 16), REEF_HOST, false, nullptr, REEF_HOST, &root));   // warm-up
            auto t0 = clk::now();
            CK(reef_merkle_commit(REEF_PALLAS, &pp, doc.data(), n_doc, REEF_HOST, false, nullptr, REEF_HOST, &root));
            merkle_ms = ms_since(t0);
        }
    }

    std::string json_line(const std::string &devices_json) const {
        const size_t pairs_step = sh->c2 + sh->w1 + sh->c1 + sh->w2;
        std::vector<char> line(16384);
        snprintf(line.data(), line.size(), "{\"replay\": \"%s\", \"ipa\": \"%s\", \"note\": \"MSM work of reef --prove replayed through the C ABI; host-side proving work not included\", "
               "\"shapes\": \"PREDICTED by Reef's cost model (src/backend/costs.rs restated in oracle/costs_oracle.py, read from %s), not measured on a Reef run\", \"w1\": %zu, \"c1\": %zu, \"w2\": %zu, \"c2\": %zu, "
               "\"scalars\": \"per-step vectors in host memory, commitments returned to the host (PCIe inclusive)\", \"commitments_checked_against_dlog\": %d, "
               "\"key_pallas\": %zu, \"key_vesta\": %zu, \"steps\": %d, \"setup_ms\": %.3f, \"setup_first_ms\": %.3f, \"setup_path\": \"both curves at once, each label -> derived generators on the device -> resident pre-shifted key (Reef re-derives its keys on every --prove: framework.rs:297-303)\", \"check_keys_ms\": %.3f, \"fold_steps_ms\": %.3f, \"ms_per_step\": %.3f, "
               "\"ms_per_step_batched_pairs\": %.3f, \"ms_per_step_concurrent\": %.3f, \"ms_per_step_all_four_at_once\": %.3f, \"pairs_per_step\": %zu, \"final_snark_ms\": %.3f, \"ipa_pallas_ms\": %.3f, \"ipa_pallas_rounds\": %d, \"ipa_vesta_ms\": %.3f, "
               "\"ipa_vesta_rounds\": %d, \"consistency_ipa_ms\": %.3f, \"consistency_rounds\": %d, \"three_arguments_concurrently_ms\": %.3f, \"total_prove_msm_ms\": %.3f, "
               "\"commit_hyrax_ms\": %.3f, \"commit_hyrax_first_call_ms\": %.3f, \"sumcheck_table_log\": %d, \"sumcheck_ms_per_step\": %.3f, "
               "\"doc_poly_bind_rows_ms\": %.3f, \"total_prove_gpu_ms\": %.3f, \"prove_gpu_incl_setup_ms\": %.3f, \"commit_merkle_log\": %d, \"commit_merkle_ms\": %.3f, "
               "\"standins\": \"key derivation and Poseidon run on stand-in parameter sets (replay_standins.h), timing only\", \"byte_tables\": %s, \"devices\": %s}",
               sh->name.c_str(), nofold ? "cross terms over the original key (no generator fold)" : "generator fold per round", sh->file.c_str(), sh->w1, sh->c1, sh->w2, sh->c2, g_checked, cv[0].n, cv[1].n, sh->steps, setup_ms, setup_first_ms, check_keys_ms, steps_ms, steps_ms / sh->steps, steps_batched_ms / sh->steps, steps_conc_ms / sh->steps, steps_all4_ms / sh->steps, pairs_step, final_ms, ipa1_ms, r1, ipa2_ms, r2,
               cons_ms, r3, concurrent_ms, steps_ms + final_ms + cons_ms, commit_ms, commit_first_ms, sh->table_log, sc_step_ms, mle_ms,
               steps_ms + final_ms + cons_ms + sh->steps * sc_step_ms + mle_ms, setup_ms + steps_ms + final_ms + cons_ms + sh->steps * sc_step_ms + mle_ms, sh->merkle_log, merkle_ms,
               tables ? "\"built with the keys (inside setup_ms): MSMs of 1025..65536 points are sums of table entries\"" : "\"none (bucket pipeline)\"", devices_json.c_str());
        return std::string(line.data());
    }
};

// The whole replay of one config; returns the JSON line.
static std::string replay_body(const Shape &shape, bool nofold, bool tables, const std::vector<int> &ordinals) {
    MsmReplay r(shape, nofold, tables);
    r.setup(); r.check_keys(); r.scalars();
    r.fold_steps(); r.batched_pairs(); r.concurrent_pairs();
    r.final_snark(); r.side_rows();
    const std::string devices_json = ordinals.empty() ? std::string("null") : replay_devices(shape, ordinals, tables);
    return r.json_line(devices_json);        // r's owners release every context and device buffer, here or on an exception
}
