// reef_replay -- issues, through the C ABI only, the MSM sequence of one `reef --prove` run
// (eniac/Reef src/backend/framework.rs:642-754) with synthetic scalars of the right shapes, and
// times it.  Reef itself is Rust and cannot be built in this image (no cargo, crates not
// vendored), so the "--prove" numbers of this backend are REPLAYS of the commitment work, never
// an end-to-end proof: in the MSM replay (reef_replay_run) NFA construction, witness generation
// and the final SNARK's sum-checks stay on the host and are not part of what is timed.  The prove
// leg (reef_replay_run_prove, `reef_replay cfgN prove`, below) runs every device row of one proof
// instead -- NIFS steps, Spartan sum-checks, the batched opening, the Hyrax consistency argument --
// on synthetic R1CS of the same sizes, and checks the proof with the verifier's equations.
//
// Sequence (sizes from Reef's cost model, src/backend/costs.rs):
//   setup            keys for G1 (Pallas) and G2 (Vesta): generated + pre-shifted on the GPU
//   per folding step comm_T2 (|C2| Vesta) -> comm_W1 (|W1| Pallas) -> comm_T1 (|C1| Pallas)
//                    -> comm_W2 (|W2| Vesta); each commitment feeds the next circuit's public
//                    input, so the four MSMs are issued one after the other, result to host
//   final SNARK      one more |C2| MSM, then for each curve an IPA over the padded key length:
//                    log2 N rounds of { L, R cross MSMs (issued on two streams), generator fold }
//   consistency      IPA of the Hyrax row length (prove_eval, commitment.rs:371/383)
//   devices=N        the multi-device leg (replay_devices): arguments placed whole on N members, the document commitment through a device group
// and, beside the MSMs: the Hyrax commitment of the document (--commit), one nlookup sum-check per
// folding step (rows N2) and the document polynomial's row binding at proof end (row N3).
//
// What crosses PCIe: the per-step scalar vectors live in ordinary HOST memory, as nova hands them over
// (framework.rs:668), and every commitment comes back to the host.  What is checked: the generators are an
// arithmetic progression B_i = (k0 + i*d)*G, so each MSM has a known discrete logarithm; every per-step
// commitment is compared with (sum_i s_i*(k0 + i*d) mod r)*G computed from host big-integer arithmetic and a
// one-point key, and the replay aborts on the first mismatch.  The sizes are PREDICTIONS of Reef's cost model
// (src/backend/costs.rs), not measurements of a Reef run: flagged in the JSON line.  No MSM length is typed in here: the
// shapes are read from tests/golden/replay_shapes.json, which oracle/gen_replay_shapes.py derives from its restatement of
// costs.rs (the SAFA shape of each regex is an input of that script).
//
// One translation unit, two artefacts (csrc/Makefile): libreef_replay.so exports reef_replay_run() -- bench.py calls it
// in-process after its timed region, tests/test_gpu_replay.py under pytest -- and the reef_replay executable is its main().
// Build: g++ -O2 -std=c++17 -fPIC -shared reef_replay.cpp -I../../../include -L../../_lib -lreef_msm -o libreef_replay.so
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "reef_msm.h"
#include "reef_provider.hpp"
#include "replay_standins.h"

// a failed call ends the replay with its message (reef_replay_run returns it; the executable prints it and exits non-zero)
[[noreturn]] static void fail(const std::string &msg) { throw std::runtime_error(msg); }
#define CK(x)                                                                              \
    do {                                                                                   \
        reef_status s_ = (x);                                                              \
        if (s_ != REEF_OK) fail(std::string(#x) + " failed: " + reef_last_error());        \
    } while (0)

// Everything the replay allocates is owned by one of these: a failed call (an exception) unwinds through them, so a replay that
// ends early inside bench.py's process leaves no key and no device buffer behind.
struct DevFree { void operator()(void *p) const { if (p) reef_device_free(p); } };
template <class T> using dev_ptr = std::unique_ptr<T, DevFree>;
struct CtxFree { void operator()(reef_msm_ctx *p) const { if (p) reef_msm_ctx_destroy(p); } };
using ctx_ptr = std::unique_ptr<reef_msm_ctx, CtxFree>;
struct ScFree { void operator()(reef_sc_ctx *p) const { if (p) reef_sc_destroy(p); } };
using sc_ptr = std::unique_ptr<reef_sc_ctx, ScFree>;
template <class T> static dev_ptr<T> device_alloc(size_t count) {
    T *p = (T *)reef_device_alloc(count * sizeof(T));
    if (!p) throw std::runtime_error(std::string("alloc: ") + reef_last_error());
    return dev_ptr<T>(p);
}

using clk = std::chrono::steady_clock;
static double ms_since(clk::time_point t0) { return std::chrono::duration<double, std::milli>(clk::now() - t0).count(); }

// ---- host-side check: discrete logarithm of an MSM over generators in arithmetic progression ------------------
static const uint64_t ORDER[2][4] = {   // group orders: Pallas (= Fq), Vesta (= Fp); little-endian limbs
    {0x8c46eb2100000001ULL, 0x224698fc0994a8ddULL, 0x0ULL, 0x4000000000000000ULL},
    {0x992d30ed00000001ULL, 0x224698fc094cf91bULL, 0x0ULL, 0x4000000000000000ULL}};
struct Big { uint64_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0}; };
static void big_addmul(Big &a, const uint64_t s[4], uint64_t m) {   // a += s * m
    unsigned __int128 carry = 0;
    for (int i = 0; i < 8; ++i) {
        unsigned __int128 t = (unsigned __int128)a.w[i] + carry + (i < 4 ? (unsigned __int128)s[i] * m : 0);
        a.w[i] = (uint64_t)t;
        carry = t >> 64;
    }
}
static int big_cmp_shifted(const Big &a, const uint64_t r[4], int shift) {   // a <=> r << shift
    Big b;
    const int ws = shift / 64, bs = shift % 64;
    for (int i = 0; i < 4; ++i) {
        if (i + ws < 8) b.w[i + ws] |= r[i] << bs;
        if (bs && i + ws + 1 < 8) b.w[i + ws + 1] |= r[i] >> (64 - bs);
    }
    for (int i = 7; i >= 0; --i)
        if (a.w[i] != b.w[i]) return a.w[i] < b.w[i] ? -1 : 1;
    return 0;
}
static void big_sub_shifted(Big &a, const uint64_t r[4], int shift) {
    Big b;
    const int ws = shift / 64, bs = shift % 64;
    for (int i = 0; i < 4; ++i) {
        if (i + ws < 8) b.w[i + ws] |= r[i] << bs;
        if (bs && i + ws + 1 < 8) b.w[i + ws + 1] |= r[i] >> (64 - bs);
    }
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

struct Shape {
    std::string name;
    size_t w1 = 0, c1 = 0, w2 = 0, c2 = 0;   // |W1|, |C1| (Pallas), |W2|, |C2| (Vesta)
    int steps = 0;
    size_t hyrax_row = 0;    // R = 2^(l - l/2): length of the consistency IPA (0 = merkle mode)
    int doc_log = 0;         // l = log2 of the padded document length the Hyrax commitment covers (0: no Hyrax commitment)
    int symbol_bits = 0;     // width of a document symbol (alphabet + EOF/EPSILON, framework.rs:978-1011)
    int table_log = 0;       // log2 of the table the per-step nlookup sum-check runs over (r1cs.rs:2318-2385); 0: not replayed
    int lookups = 0;         // lookups folded per step (batch size)
    int merkle_log = 0;      // --merkle: log2 of the document the Poseidon tree commits to (0: Hyrax commitment)
};

// ---- tests/golden/replay_shapes.json: the "shapes" array of flat objects written by oracle/gen_replay_shapes.py ----
static std::string read_file(const std::string &path) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) fail("cannot open the replay shapes file " + path + " (generated by oracle/gen_replay_shapes.py)");
    std::string s;
    char buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0) s.append(buf, got);
    fclose(f);
    return s;
}
static long long json_int(const std::string &obj, const char *key) {
    const std::string k = std::string("\"") + key + "\":";
    size_t p = obj.find(k);
    if (p == std::string::npos) fail(std::string("replay shapes: field ") + key + " missing");
    return atoll(obj.c_str() + p + k.size());
}
static Shape load_shape(const std::string &path, const char *which) {
    const std::string text = read_file(path);
    size_t p = text.find("\"shapes\":");
    if (p == std::string::npos) fail("replay shapes: no \"shapes\" array in " + path);
    for (;;) {
        const size_t b = text.find('{', p);
        if (b == std::string::npos) break;
        const size_t e = text.find('}', b);
        if (e == std::string::npos) break;
        const std::string obj = text.substr(b, e - b + 1);
        p = e + 1;
        const size_t np = obj.find("\"name\":");
        if (np == std::string::npos) continue;
        const size_t q0 = obj.find('"', np + 7), q1 = obj.find('"', q0 + 1);
        const std::string name = obj.substr(q0 + 1, q1 - q0 - 1);
        if (name.find(which) == std::string::npos) continue;
        Shape s;
        s.name = name;
        s.w1 = (size_t)json_int(obj, "w1"); s.c1 = (size_t)json_int(obj, "c1");
        s.w2 = (size_t)json_int(obj, "w2"); s.c2 = (size_t)json_int(obj, "c2");
        s.steps = (int)json_int(obj, "steps");
        s.hyrax_row = (size_t)json_int(obj, "hyrax_row");
        s.doc_log = (int)json_int(obj, "doc_log");
        s.symbol_bits = (int)json_int(obj, "symbol_bits");
        s.table_log = (int)json_int(obj, "table_log");
        s.lookups = (int)json_int(obj, "lookups");
        s.merkle_log = (int)json_int(obj, "merkle_log");
        if (!s.w1 || !s.c1 || !s.w2 || !s.c2 || s.steps < 1) fail("replay shapes: " + name + " is not a usable shape");
        return s;
    }
    fail(std::string("replay shapes: no config matching '") + which + "' in " + path);
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
// abort unless `got` is dlog*G (both normalised to affine)
static void check_point(Curve &c, const reef_jacobian &got, const reef_fe &dlog, const char *what) {
    reef_jacobian want;
    CK(reef_msm(c.one, &dlog, 1, REEF_HOST, false, &want, REEF_HOST));
    reef_jacobian both[2] = {got, want};
    reef_affine aff[2];
    CK(reef_normalize(c.id, both, 2, REEF_HOST, aff, nullptr));
    if (memcmp(&aff[0], &aff[1], sizeof(reef_affine)) != 0)
        fail(std::string("reef_replay: ") + what + " on curve " + std::to_string(c.id) + " differs from its discrete-logarithm closed form");
    ++g_checked;
}

static size_t next_pow2(size_t x) { size_t p = 1; while (p < x) p <<= 1; return p; }

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
    const double again = ms_since(t0);
    return again;
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
        reef_msm_opts o = {};
        o.bucket_groups = 1;
        o.byte_tables = tables ? 1 : 2;
        o.device = a.device;
        CK(reef_msm_ctx_create(&a.c.key, a.c.id, a.gens.get(), a.c.n, REEF_DEVICE, &o));
        a.key.reset(a.c.key);
        run_ipa_nofold(a.c, a.c.n, a.sc.get(), nullptr);                     // warm-up: workspaces
        a.alone_ms = run_ipa_nofold(a.c, a.c.n, a.sc.get(), nullptr);
    }
    double together_ms = 0;
    {
        std::vector<std::exception_ptr> err(args.size());
        std::vector<std::thread> th;
        auto tc = clk::now();
        for (size_t k = 1; k < args.size(); ++k)
            th.emplace_back([&, k] { try { run_ipa_nofold(args[k].c, args[k].c.n, args[k].sc.get(), nullptr); } catch (...) { err[k] = std::current_exception(); } });
        try { run_ipa_nofold(args[0].c, args[0].c.n, args[0].sc.get(), nullptr); } catch (...) { err[0] = std::current_exception(); }
        for (auto &t : th) t.join();
        together_ms = ms_since(tc);
        for (auto &e : err)
            if (e) std::rethrow_exception(e);
    }
    // the document commitment over the group, against one device
    double commit_group_ms = 0, commit_one_ms = 0;
    reef_msm_group_info gi;
    memset(&gi, 0, sizeof gi);
    if (sh->doc_log) {
        const size_t n_doc = (size_t)1 << sh->doc_log;
        const size_t rows = (size_t)1 << (sh->doc_log / 2), row_len = (size_t)1 << (sh->doc_log - sh->doc_log / 2);
        std::vector<uint8_t> doc(n_doc);
        uint64_t x = 0xD0C;
        const uint32_t bound = sh->symbol_bits >= 8 ? 131u : (sh->symbol_bits == 3 ? 7u : (1u << sh->symbol_bits));
        for (size_t i = 0; i < n_doc; ++i) { x = x * 6364136223846793005ULL + 1442695040888963407ULL; doc[i] = (uint8_t)((x >> 33) % bound); }
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
        reef_poseidon_params pp;
        pp.width = 5; pp.full_rounds = STANDIN_POSEIDON_RF; pp.partial_rounds = STANDIN_POSEIDON_RP; pp.reserved = 0;
        pp.round_constants = STANDIN_POSEIDON_RC; pp.mds = STANDIN_POSEIDON_MDS;
        pp.tag_leaf = STANDIN_POSEIDON_TAGS[0]; pp.tag_node = STANDIN_POSEIDON_TAGS[1];
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

// The whole replay of one config; returns the JSON line.
static std::string replay_body(const Shape &shape, bool nofold, bool tables, const std::string &shapes_path, const std::vector<int> &ordinals) {
    const Shape *sh = &shape;
    Curve cv[2];
    cv[0].id = REEF_PALLAS; cv[0].n = next_pow2(sh->w1 > sh->c1 ? sh->w1 : sh->c1);
    cv[1].id = REEF_VESTA;  cv[1].n = next_pow2(sh->w2 > sh->c2 ? sh->w2 : sh->c2);

    std::vector<dev_ptr<reef_affine>> owned_gens;       // destroyed after the contexts below
    std::vector<ctx_ptr> owned_ctx;

    // ---- set-up as a --prove run pays it.  Reef derives its commitment keys from their labels on EVERY run (src/backend/framework.rs:115,
    // 297-303 -> CommitmentGens::new), so set-up is prove time: per curve, on a caller thread of its own -- the two curves at
    // once -- label -> n generators on the device (row N1: reef_derive_generators; stand-in hash-to-curve parameters, replay_standins.h) ->
    // resident pre-shifted key straight from the device buffer (reef_msm_ctx_create): what CommitmentGens(label, n, params) of
    // reef_provider.hpp does.  Timed twice: setup_first_ms is the first pass in this process (first launches of the kernels, the
    // workspaces' allocations), setup_ms the second.  The keys built here are dropped again: the MSMs below run on keys of the same
    // sizes whose generators are an arithmetic progression (so that every commitment has a known discrete logarithm), built after the
    // clock has stopped (check_keys_ms).
    auto derive_both = [&]() {
        std::exception_ptr err[2];
        auto one = [&](int k) {
            try {
                const int id = cv[k].id;
                reef_keygen_params kp;
                const reef_fe *sp = id == REEF_PALLAS ? STANDIN_KEYGEN_0 : STANDIN_KEYGEN_1;
                const char *dst = id == REEF_PALLAS ? STANDIN_KEYGEN_DST_0 : STANDIN_KEYGEN_DST_1;
                kp.a = sp[0]; kp.b = sp[1]; kp.z = sp[2];
                memcpy(kp.iso, sp + 3, 13 * sizeof(reef_fe));
                kp.dst = (const uint8_t *)dst; kp.dst_len = (uint32_t)strlen(dst); kp.little_endian = 0;
                const dev_ptr<reef_affine> gens = device_alloc<reef_affine>(cv[k].n);
                CK(reef_derive_generators(id, (const uint8_t *)"ck", 2, cv[k].n, &kp, false, gens.get(), REEF_DEVICE));
                reef_msm_opts o = {};
                o.bucket_groups = 1;              // commitment keys are fixed for the life of PublicParams: pre-shift once
                o.byte_tables = tables ? 1 : 2;   // explicit: built with the key, or never (no switch of paths mid-run)
                o.device = -1;
                reef_msm_ctx *key = nullptr;
                CK(reef_msm_ctx_create(&key, id, gens.get(), cv[k].n, REEF_DEVICE, &o));
                const ctx_ptr owner(key);
                CK(reef_msm_ctx_sync(key));
            } catch (...) { err[k] = std::current_exception(); }
        };
        auto t0 = clk::now();
        std::thread other(one, 1);
        one(0);
        other.join();
        const double ms = ms_since(t0);
        for (auto &e : err)
            if (e) std::rethrow_exception(e);
        return ms;
    };
    const double setup_first_ms = derive_both();
    const double setup_ms = derive_both();

    auto t_check_keys = clk::now();
    for (Curve &c : cv) {
        owned_gens.push_back(device_alloc<reef_affine>(c.n));
        c.d_gens = owned_gens.back().get();
        c.k0 = 0xC0FFEE + c.id; c.d = 7;
        CK(reef_gen_bases(c.id, c.k0, c.d, c.n, c.d_gens, REEF_DEVICE));
        {
            reef_affine g1;
            CK(reef_gen_bases(c.id, 1, 0, 1, &g1, REEF_HOST));           // 1*G
            reef_msm_opts og = {};
            og.bucket_groups = 1;
            og.device = -1;
            CK(reef_msm_ctx_create(&c.one, c.id, &g1, 1, REEF_HOST, &og));
            owned_ctx.emplace_back(c.one);
        }
        reef_msm_opts o = {};
        o.bucket_groups = 1;
        o.byte_tables = tables ? 1 : 2;
        o.device = -1;
        CK(reef_msm_ctx_create(&c.key, c.id, c.d_gens, c.n, REEF_DEVICE, &o));
        owned_ctx.emplace_back(c.key);
        CK(reef_msm_ctx_sync(c.key));
        reef_msm_opts plain = {};
        plain.device = -1;
        if (!nofold)   // the per-round re-keyed contexts exist only in the generator-fold IPA
            for (auto &x : c.ipa) { CK(reef_msm_ctx_create(&x, c.id, c.d_gens, c.n / 2, REEF_DEVICE, &plain)); owned_ctx.emplace_back(x); }
    }
    const double check_keys_ms = ms_since(t_check_keys);

    // witness-like scalars for W, uniform for the cross terms T
    const dev_ptr<reef_fe> oW1 = device_scalars(REEF_PALLAS, 11, 1, cv[0].n), oT1 = device_scalars(REEF_PALLAS, 12, 0, cv[0].n);
    const dev_ptr<reef_fe> oW2 = device_scalars(REEF_VESTA, 13, 1, cv[1].n), oT2 = device_scalars(REEF_VESTA, 14, 0, cv[1].n);
    reef_fe *sW1 = oW1.get(), *sT1 = oT1.get(), *sW2 = oW2.get(), *sT2 = oT2.get();
    // the same vectors in HOST memory (Montgomery form, what nova holds) and as canonical integers (for the check)
    struct HostVec { std::vector<reef_fe> mont, canon; };
    auto host_vec = [&](int curve, uint64_t seed, int kind, size_t n) {
        HostVec v;
        v.mont.resize(n); v.canon.resize(n);
        CK(reef_gen_scalars(curve, seed, kind, 0, n, true, v.mont.data(), REEF_HOST));
        CK(reef_gen_scalars(curve, seed, kind, 0, n, false, v.canon.data(), REEF_HOST));
        return v;
    };
    HostVec hW1 = host_vec(REEF_PALLAS, 11, 1, cv[0].n), hT1 = host_vec(REEF_PALLAS, 12, 0, cv[0].n);
    HostVec hW2 = host_vec(REEF_VESTA, 13, 1, cv[1].n), hT2 = host_vec(REEF_VESTA, 14, 0, cv[1].n);
    // expected discrete logarithms of the four per-step commitments (computed once, outside the timed loops)
    const reef_fe eW1 = dlog_of_msm(0, hW1.canon.data(), sh->w1, cv[0].k0, cv[0].d), eT1 = dlog_of_msm(0, hT1.canon.data(), sh->c1, cv[0].k0, cv[0].d);
    const reef_fe eW2 = dlog_of_msm(1, hW2.canon.data(), sh->w2, cv[1].k0, cv[1].d), eT2 = dlog_of_msm(1, hT2.canon.data(), sh->c2, cv[1].k0, cv[1].d);

    reef_jacobian out;
    auto msm = [&](Curve &c, const HostVec &s, size_t n) {
        CK(reef_msm(c.key, s.mont.data(), n, REEF_HOST, true, &out, REEF_HOST));   // host scalars in, commitment back to the host: it feeds the next circuit
    };
    // warm-up (workspace allocation) and the first check
    msm(cv[0], hW1, sh->w1); check_point(cv[0], out, eW1, "comm_W1");
    msm(cv[1], hW2, sh->w2); check_point(cv[1], out, eW2, "comm_W2");

    // a config may fold in a single step: time at least three so that the per-step figure is not one sample; the totals
    // below charge the config's own number of steps
    const int timed_steps = sh->steps < 3 ? 3 : sh->steps;
    std::vector<double> step_ms;
    for (int i = 0; i < timed_steps; ++i) {
        auto ts = clk::now();
        reef_jacobian o[4];
        msm(cv[1], hT2, sh->c2); o[0] = out;
        msm(cv[0], hW1, sh->w1); o[1] = out;
        msm(cv[0], hT1, sh->c1); o[2] = out;
        msm(cv[1], hW2, sh->w2); o[3] = out;
        step_ms.push_back(ms_since(ts));
        check_point(cv[1], o[0], eT2, "comm_T2");           // outside the step's timing
        check_point(cv[0], o[1], eW1, "comm_W1");
        check_point(cv[0], o[2], eT1, "comm_T1");
        check_point(cv[1], o[3], eW2, "comm_W2");
    }
    double steps_ms = 0;
    for (double v : step_ms) steps_ms += v;
    steps_ms = steps_ms / timed_steps * sh->steps;

    // The same commitments with the two of each curve issued as ONE batched call (comm_W and comm_T of a
    // step are both absorbed before the folding challenge is drawn, so neither needs the other): rows = 2
    // over the same resident key share one pass of the pipeline.  Needs prove_step to hand both vectors
    // over together; reported next to the call-by-call figure, not instead of it.
    double steps_batched_ms = 0;
    {
        struct Pair { Curve *c; const reef_fe *a, *b; size_t len; reef_fe *buf; } pairs[2] = {
            {&cv[0], sW1, sT1, sh->w1 > sh->c1 ? sh->w1 : sh->c1, nullptr}, {&cv[1], sW2, sT2, sh->w2 > sh->c2 ? sh->w2 : sh->c2, nullptr}};
        std::vector<reef_fe> hostbuf[2];
        const HostVec *hv[2][2] = {{&hW1, &hT1}, {&hW2, &hT2}};
        reef_fe expect[2][2];
        for (int k = 0; k < 2; ++k) {
            Pair &p = pairs[k];
            hostbuf[k].resize(2 * p.len);                // the two vectors of a curve side by side in host memory
            memcpy(hostbuf[k].data(), hv[k][0]->mont.data(), p.len * sizeof(reef_fe));
            memcpy(hostbuf[k].data() + p.len, hv[k][1]->mont.data(), p.len * sizeof(reef_fe));
            for (int j = 0; j < 2; ++j) expect[k][j] = dlog_of_msm(k, hv[k][j]->canon.data(), p.len, p.c->k0, p.c->d);
        }
        reef_jacobian two[2];
        auto both = [&](int k) { CK(reef_msm_rows(pairs[k].c->key, hostbuf[k].data(), 2, pairs[k].len, REEF_HOST, true, 255, nullptr, nullptr, two, REEF_HOST)); };
        for (int k = 0; k < 2; ++k) {                    // warm-up and check
            both(k);
            check_point(*pairs[k].c, two[0], expect[k][0], "batched comm_W");
            check_point(*pairs[k].c, two[1], expect[k][1], "batched comm_T");
        }
        auto tb = clk::now();
        for (int i = 0; i < timed_steps; ++i) { both(1); both(0); }
        steps_batched_ms = ms_since(tb) / timed_steps * sh->steps;
    }

    // The pair of a curve issued as two CONCURRENT MSMs instead (reef_msm_multi: both enqueued, then both waited for; the second
    // commitment runs on a clone of the key, i.e. on another stream of the library's pool), and -- an upper bound only, because
    // the two curves of a step depend on each other through the step circuits -- all four at once.
    double steps_conc_ms = 0, steps_all4_ms = 0;
    {
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

    auto t_final = clk::now();
    msm(cv[1], hT2, sh->c2);  // last NIFS fold
    int r1 = 0, r2 = 0, r3 = 0;
    const double ipa1_ms = nofold ? run_ipa_nofold(cv[0], cv[0].n, sT1, &r1) : run_ipa(cv[0], cv[0].n, sT1, &r1);
    const double ipa2_ms = nofold ? run_ipa_nofold(cv[1], cv[1].n, sT2, &r2) : run_ipa(cv[1], cv[1].n, sT2, &r2);
    const double final_ms = ms_since(t_final);

    double cons_ms = 0, concurrent_ms = 0;
    Curve hy;
    ctx_ptr hy_owner;
    if (sh->hyrax_row >= 2) {
        hy.id = REEF_PALLAS; hy.n = sh->hyrax_row; hy.d_gens = cv[0].d_gens;  // prefix of the same key shape
        for (int k = 0; k < 2; ++k) hy.ipa[k] = cv[0].ipa[k];
        if (nofold) {   // the Hyrax row generators are a resident key of their own (commitment.rs:176-186)
            reef_msm_opts o = {};
            o.bucket_groups = 1;
            o.byte_tables = tables ? 1 : 2;
            o.device = -1;
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
        std::exception_ptr err[2];
        auto guarded = [&](int k, Curve &c, const reef_fe *sc) {
            try { run_ipa_nofold(c, c.n, sc, nullptr); } catch (...) { err[k] = std::current_exception(); }
        };
        auto tc = clk::now();
        std::thread a(guarded, 0, std::ref(cv[0]), (const reef_fe *)sT1), b(guarded, 1, std::ref(cv[1]), (const reef_fe *)sT2);
        if (hy.key) run_ipa_nofold(hy, hy.n, sT1, nullptr);
        a.join();
        b.join();
        concurrent_ms = ms_since(tc);
        for (auto &e : err)
            if (e) std::rethrow_exception(e);
    }

    // ---- commitment of the document, the per-step sum-check and the document polynomial at proof end
    double commit_ms = 0, commit_first_ms = 0, sc_step_ms = 0, mle_ms = 0;
    if (sh->doc_log) {
        const size_t n_doc = (size_t)1 << sh->doc_log;
        const dev_ptr<uint8_t> doc_owner = device_symbols(n_doc, sh->symbol_bits, 0xD0C);
        uint8_t *d_doc = doc_owner.get();
        const size_t row_len = (size_t)1 << (sh->doc_log - sh->doc_log / 2);
        const dev_ptr<reef_affine> row_gens_owner = device_alloc<reef_affine>(row_len);
        reef_affine *d_row_gens = row_gens_owner.get();
        CK(reef_gen_bases(REEF_PALLAS, 0xFEED, 3, row_len, d_row_gens, REEF_DEVICE));
        commit_ms = run_hyrax_commit(sh, d_row_gens, d_doc, &commit_first_ms);
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
        const sc_ptr sc_owner = sumcheck_ctx(sh);
        reef_sc_ctx *sc = sc_owner.get();
        run_sumcheck_step(sc, sh->table_log, sh->lookups);            // warm-up
        // the median of three steps: one sample read 2.5 ms instead of 1.6 now and then on a box's first large run (round 4)
        double t3[3];
        for (double &t : t3) t = run_sumcheck_step(sc, sh->table_log, sh->lookups);
        std::sort(t3, t3 + 3);
        sc_step_ms = t3[1];
    }

    // ---- row N4 with STAND-IN parameters (replay_standins.h): for --merkle the Poseidon tree of the document.  Timing only: parity is
    // tests/test_gpu_merkle.py.  (Row N1, the keys derived from their labels, is the set-up above.)
    double merkle_ms = 0;
    if (sh->merkle_log) {
        const size_t n_doc = (size_t)1 << sh->merkle_log;
        std::vector<uint32_t> doc(n_doc);
        for (size_t i = 0; i < n_doc; ++i) doc[i] = (uint32_t)((i * 2654435761u) >> 24);               // one-byte symbols
        reef_poseidon_params pp;
        pp.width = 5; pp.full_rounds = STANDIN_POSEIDON_RF; pp.partial_rounds = STANDIN_POSEIDON_RP; pp.reserved = 0;
        pp.round_constants = STANDIN_POSEIDON_RC; pp.mds = STANDIN_POSEIDON_MDS;
        pp.tag_leaf = STANDIN_POSEIDON_TAGS[0]; pp.tag_node = STANDIN_POSEIDON_TAGS[1];
        reef_fe root;
        CK(reef_merkle_commit(REEF_PALLAS, &pp, doc.data(), std::min(n_doc, (size_t)1 << 16), REEF_HOST, false, nullptr, REEF_HOST, &root));   // warm-up
        auto t0 = clk::now();
        CK(reef_merkle_commit(REEF_PALLAS, &pp, doc.data(), n_doc, REEF_HOST, false, nullptr, REEF_HOST, &root));
        merkle_ms = ms_since(t0);
    }

    const std::string devices_json = ordinals.empty() ? std::string("null") : replay_devices(shape, ordinals, tables);
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
           sh->name.c_str(), nofold ? "cross terms over the original key (no generator fold)" : "generator fold per round", shapes_path.c_str(), sh->w1, sh->c1, sh->w2, sh->c2, g_checked, cv[0].n, cv[1].n, sh->steps, setup_ms, setup_first_ms, check_keys_ms, steps_ms, steps_ms / sh->steps, steps_batched_ms / sh->steps, steps_conc_ms / sh->steps, steps_all4_ms / sh->steps, pairs_step, final_ms, ipa1_ms, r1, ipa2_ms, r2,
           cons_ms, r3, concurrent_ms, steps_ms + final_ms + cons_ms, commit_ms, commit_first_ms, sh->table_log, sc_step_ms, mle_ms,
           steps_ms + final_ms + cons_ms + sh->steps * sc_step_ms + mle_ms, setup_ms + steps_ms + final_ms + cons_ms + sh->steps * sc_step_ms + mle_ms, sh->merkle_log, merkle_ms,
           tables ? "\"built with the keys (inside setup_ms): MSMs of 1025..65536 points are sums of table entries\"" : "\"none (bucket pipeline)\"", devices_json.c_str());
    return std::string(line.data());        // the owners above release every context and device buffer, here or on an exception
}

// ==== the prove leg (`reef_replay cfgN prove`) =========================================================================================
// Every device row of one proof, through the C ABI and the provider mirror (reef_provider.hpp), in the order `reef --prove` runs
// them (framework.rs:642-754): per folding step the N2 sum-check step and, per curve, comm_W, NIFS commit_T, a challenge and the
// fold (3f); the last fold; per curve the Spartan sum-checks (3g) and the batched IPA opening (3h) on the instance the folds left
// on the device; the Hyrax consistency argument over the committed document (3i).  The R1CS matrices are SYNTHETIC (layered,
// satisfiable, of the shape's sizes), the transcript is a stand-in hash, and the point operations the Rust host does on
// commitments (comm_W, comm_E of a folded instance, comm_a) are tracked as discrete logarithms, which every generator here has.
// After the timed region the proof is checked with the verifier's equations on the host, and every point the device returned
// against its discrete logarithm; `tamper=<phase>` alters one recorded value first, to show that the checks can fail.

// ---- host scalar arithmetic: 4x64 Montgomery products mod a group order (R = 2^256, the form of pasta's scalars) ---------------
// Elements are reef_fe in Montgomery form throughout: what the rows take and return with is_mont = true.
struct Mod {
    uint64_t p[4];
    uint64_t inv;           // -p^-1 mod 2^64
    reef_fe one, r2;        // R mod p, R^2 mod p
    reef_fe inv2, inv6;     // 1/2, 1/6 (the sum-check interpolation)
    explicit Mod(const uint64_t q[4]);
};
static bool geq_p(const uint64_t a[4], const uint64_t p[4]) {
    for (int i = 3; i >= 0; --i)
        if (a[i] != p[i]) return a[i] > p[i];
    return true;
}
static void sub_p(uint64_t a[4], const uint64_t p[4]) {
    unsigned __int128 borrow = 0;
    for (int i = 0; i < 4; ++i) {
        const unsigned __int128 t = (unsigned __int128)a[i] - p[i] - borrow;
        a[i] = (uint64_t)t;
        borrow = (t >> 64) & 1;
    }
}
static inline reef_fe fadd(const Mod &m, const reef_fe &a, const reef_fe &b) {   // both < p < 2^255: no carry out of 256 bits
    reef_fe r;
    unsigned __int128 c = 0;
    for (int i = 0; i < 4; ++i) {
        c += (unsigned __int128)a.l[i] + b.l[i];
        r.l[i] = (uint64_t)c;
        c >>= 64;
    }
    if (geq_p(r.l, m.p)) sub_p(r.l, m.p);
    return r;
}
static inline reef_fe fsub(const Mod &m, const reef_fe &a, const reef_fe &b) {
    reef_fe r;
    unsigned __int128 borrow = 0;
    for (int i = 0; i < 4; ++i) {
        const unsigned __int128 t = (unsigned __int128)a.l[i] - b.l[i] - borrow;
        r.l[i] = (uint64_t)t;
        borrow = (t >> 64) & 1;
    }
    if (borrow) {
        unsigned __int128 c = 0;
        for (int i = 0; i < 4; ++i) {
            c += (unsigned __int128)r.l[i] + m.p[i];
            r.l[i] = (uint64_t)c;
            c >>= 64;
        }
    }
    return r;
}
static inline reef_fe fmul(const Mod &m, const reef_fe &a, const reef_fe &b) {   // CIOS
    uint64_t t[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < 4; ++i) {
        unsigned __int128 c = 0;
        for (int j = 0; j < 4; ++j) {
            c += (unsigned __int128)a.l[j] * b.l[i] + t[j];
            t[j] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[4] = (uint64_t)c;
        t[5] = (uint64_t)(c >> 64);
        const uint64_t q = t[0] * m.inv;
        c = ((unsigned __int128)q * m.p[0] + t[0]) >> 64;
        for (int j = 1; j < 4; ++j) {
            c += (unsigned __int128)q * m.p[j] + t[j];
            t[j - 1] = (uint64_t)c;
            c >>= 64;
        }
        c += t[4];
        t[3] = (uint64_t)c;
        t[4] = t[5] + (uint64_t)(c >> 64);
    }
    reef_fe r = {{t[0], t[1], t[2], t[3]}};
    if (t[4] || geq_p(r.l, m.p)) sub_p(r.l, m.p);
    return r;
}
static bool feq(const reef_fe &a, const reef_fe &b) { return memcmp(&a, &b, sizeof a) == 0; }
static reef_fe to_m(const Mod &m, const reef_fe &canon) { return fmul(m, canon, m.r2); }
static reef_fe fsmall(const Mod &m, uint64_t v) { return to_m(m, reef_fe{{v, 0, 0, 0}}); }
static reef_fe finv(const Mod &m, const reef_fe &a) {   // a^(p-2)
    uint64_t e[4];
    memcpy(e, m.p, sizeof e);
    e[0] -= 2;   // p is odd and > 2: no borrow
    reef_fe r = m.one;
    for (int i = 255; i >= 0; --i) {
        r = fmul(m, r, r);
        if ((e[i / 64] >> (i % 64)) & 1) r = fmul(m, r, a);
    }
    return r;
}
Mod::Mod(const uint64_t q[4]) {
    memcpy(p, q, sizeof p);
    uint64_t x = p[0];                                  // Newton: x = p^-1 mod 2^64 (3 correct bits to start, doubled per step)
    for (int i = 0; i < 6; ++i) x *= 2 - p[0] * x;
    inv = 0 - x;
    reef_fe a = {{1, 0, 0, 0}};
    for (int i = 0; i < 256; ++i) a = fadd(*this, a, a);
    one = a;
    for (int i = 0; i < 256; ++i) a = fadd(*this, a, a);
    r2 = a;
    inv2 = finv(*this, fsmall(*this, 2));
    inv6 = finv(*this, fsmall(*this, 6));
}
static reef_fe dot(const Mod &m, const reef_fe *a, const reef_fe *b, size_t n) {
    reef_fe s = {};
    for (size_t i = 0; i < n; ++i) s = fadd(m, s, fmul(m, a[i], b[i]));
    return s;
}
// eq(t)[i] = prod_j (bit_j(i) ? t_j : 1 - t_j), t_0 pairing with the most significant bit (reef_msm.h 3g)
static std::vector<reef_fe> eq_evals(const Mod &m, const reef_fe *t, size_t k) {
    std::vector<reef_fe> ev((size_t)1 << k);
    ev[0] = m.one;
    for (size_t j = 0; j < k; ++j) {
        const size_t len = (size_t)1 << j;
        for (size_t i = len; i-- > 0;) {
            const reef_fe hi = fmul(m, ev[i], t[j]);
            ev[2 * i] = fsub(m, ev[i], hi);
            ev[2 * i + 1] = hi;
        }
    }
    return ev;
}
static reef_fe eq_at(const Mod &m, const std::vector<reef_fe> &a, const std::vector<reef_fe> &b) {
    reef_fe out = m.one;
    for (size_t j = 0; j < a.size(); ++j) {
        const reef_fe ab = fmul(m, a[j], b[j]);   // a b + (1 - a)(1 - b) = 1 - a - b + 2ab
        out = fmul(m, out, fadd(m, fsub(m, fsub(m, m.one, a[j]), b[j]), fadd(m, ab, ab)));
    }
    return out;
}
// the cubic through (0, y0) .. (3, y3) at r, and the quadratic through (0, y0) .. (2, y2)
static reef_fe interp3(const Mod &m, const reef_fe y[4], const reef_fe &r) {
    const reef_fe r1 = fsub(m, r, m.one), r2 = fsub(m, r, fsmall(m, 2)), r3 = fsub(m, r, fsmall(m, 3));
    const reef_fe l0 = fsub(m, reef_fe{}, fmul(m, fmul(m, fmul(m, r1, r2), r3), m.inv6));
    const reef_fe l1 = fmul(m, fmul(m, fmul(m, r, r2), r3), m.inv2);
    const reef_fe l2 = fsub(m, reef_fe{}, fmul(m, fmul(m, fmul(m, r, r1), r3), m.inv2));
    const reef_fe l3 = fmul(m, fmul(m, fmul(m, r, r1), r2), m.inv6);
    return fadd(m, fadd(m, fmul(m, l0, y[0]), fmul(m, l1, y[1])), fadd(m, fmul(m, l2, y[2]), fmul(m, l3, y[3])));
}
static reef_fe interp2(const Mod &m, const reef_fe y[3], const reef_fe &r) {
    const reef_fe r1 = fsub(m, r, m.one), r2 = fsub(m, r, fsmall(m, 2));
    const reef_fe l0 = fmul(m, fmul(m, r1, r2), m.inv2);
    const reef_fe l1 = fsub(m, reef_fe{}, fmul(m, r, r2));
    const reef_fe l2 = fmul(m, fmul(m, r, r1), m.inv2);
    return fadd(m, fadd(m, fmul(m, l0, y[0]), fmul(m, l1, y[1])), fmul(m, l2, y[2]));
}
// s_j = prod_k (bit of round k in j ? r_k : r_k^-1), round 0 on the most significant bit: <s, G> = the folded generator
static std::vector<reef_fe> s_vector(const Mod &m, const std::vector<reef_fe> &rs) {
    std::vector<reef_fe> s(1, m.one);
    for (const reef_fe &r : rs) {
        const reef_fe ri = finv(m, r);
        std::vector<reef_fe> t(2 * s.size());
        for (size_t i = 0; i < s.size(); ++i) { t[2 * i] = fmul(m, s[i], ri); t[2 * i + 1] = fmul(m, s[i], r); }
        s.swap(t);
    }
    return s;
}

// A stand-in for nova's Keccak transcript [R]: a deterministic 256-bit mix of every label and byte absorbed; a challenge is the
// state reduced mod the scalar field, never 0, in Montgomery form.  Not a hash anyone should rely on: it only has to make every
// challenge depend on everything the prover returned before it.
struct StandinTranscript {
    const Mod *m;
    uint64_t s[4] = {0x6a09e667f3bcc908ULL, 0xbb67ae8584caa73bULL, 0x3c6ef372fe94f82bULL, 0xa54ff53a5f1d36f1ULL};
    unsigned lane = 0;
    explicit StandinTranscript(const Mod &mod, uint64_t domain) : m(&mod) { word(domain); }
    static uint64_t mix(uint64_t z) {
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
        return z ^ (z >> 31);
    }
    void word(uint64_t w) {
        s[lane] = mix(s[lane] ^ w ^ (s[(lane + 1) & 3] << 1));
        lane = (lane + 1) & 3;
    }
    void absorb(const char *label, const void *bytes, size_t len) {
        for (const char *c = label; *c; ++c) word(0x100u | (uint8_t)*c);
        word(len);
        const uint8_t *b = (const uint8_t *)bytes;
        for (size_t i = 0; i < len; i += 8) {
            uint64_t w = 0;
            memcpy(&w, b + i, std::min<size_t>(8, len - i));
            word(w);
        }
    }
    reef_fe squeeze() {
        for (int i = 0; i < 4; ++i) word(0x5155eeeeULL + i);
        reef_fe r = {{s[0], s[1], s[2], s[3]}};
        while (geq_p(r.l, m->p)) sub_p(r.l, m->p);   // < 2^256 < 4p
        if (feq(r, reef_fe{})) r.l[0] = 1;
        word(0xC0DEULL);
        return to_m(*m, r);
    }
    reef_provider::Transcript fn() {
        return [this](const char *label, const void *bytes, size_t len) { absorb(label, bytes, len); return squeeze(); };
    }
};

// ---- the synthetic R1CS: the layered scheme of oracle/r1cs_oracle.py::layered_shape, restated ----------------------------------
// Variables: num_inputs free inputs, then one output per non-empty constraint; z = W || u || X (num_io = 2).  Constraint i:
// (2-4 terms) * (2-4 terms) = c_i out_i + (0-1 term) over u, X, the inputs and the outputs of earlier constraints, coefficients from
// a pool of small, negative, power-of-two and full-width values.  num_vars = num_cons is met by leaving the last rows empty.
struct R1cs {
    size_t num_cons = 0, num_vars = 0, num_io = 2, num_inputs = 0;
    std::vector<size_t> start[3];             // CSR row offsets of A, B, C (num_cons + 1); C's first entry of a row is its output
    std::vector<uint32_t> row[3], col[3];
    std::vector<reef_fe> val[3];              // Montgomery
    std::vector<reef_fe> c_inv;               // per constraint: 1 / c_i (zero for an empty row)
    std::vector<uint8_t> has_out;
    size_t nnz() const { return row[0].size() + row[1].size() + row[2].size(); }
};
struct Inst {                                 // a relaxed instance with its witness: (W, E, u, X)
    std::vector<reef_fe> W, E, X;
    reef_fe u = {};
};
struct Rng {
    uint64_t x;
    uint64_t next() { x += 0x9e3779b97f4a7c15ULL; return StandinTranscript::mix(x); }
    reef_fe full(const Mod &m) {   // uniform below 2^254 < p
        reef_fe r = {{next(), next(), next(), next() >> 2}};
        return to_m(m, r);
    }
};
static R1cs layered_r1cs(const Mod &m, size_t num_cons, size_t num_vars, uint64_t seed) {
    R1cs S;
    S.num_cons = num_cons;
    S.num_vars = num_vars;
    if (num_vars < 9 || num_cons < 1) fail("layered_r1cs: at least 9 variables and one constraint");
    const size_t nout = std::min(num_cons, num_vars - 8);
    S.num_inputs = num_vars - nout;
    Rng rng{seed};
    std::vector<reef_fe> pool;
    for (uint64_t v : {1ull, 2ull, 3ull, 7ull, 1000ull, 0xFFFFull, 0x10000ull, 1ull << 40}) {
        pool.push_back(fsmall(m, v));
        pool.push_back(fsub(m, reef_fe{}, fsmall(m, v)));
    }
    for (int k = 1; k < 16; ++k) pool.push_back(fsmall(m, 1ull << k));
    for (int k = 0; k < 8; ++k) pool.push_back(rng.full(m));   // full-width coefficients
    std::vector<reef_fe> pool_inv(pool.size());
    for (size_t k = 0; k < pool.size(); ++k) pool_inv[k] = finv(m, pool[k]);
    std::vector<uint32_t> avail;
    for (size_t v = 0; v < S.num_inputs; ++v) avail.push_back((uint32_t)v);
    for (size_t j = 0; j <= S.num_io; ++j) avail.push_back((uint32_t)(num_vars + j));   // u, X
    for (int k = 0; k < 3; ++k) S.start[k].reserve(num_cons + 1);
    S.c_inv.assign(num_cons, reef_fe{});
    S.has_out.assign(num_cons, 0);
    auto term = [&](int k, size_t i, uint32_t c, const reef_fe &v) {
        S.row[k].push_back((uint32_t)i);
        S.col[k].push_back(c);
        S.val[k].push_back(v);
    };
    for (size_t i = 0; i < num_cons; ++i) {
        for (int k = 0; k < 3; ++k) S.start[k].push_back(S.row[k].size());
        if (i >= nout) continue;                                            // an empty row
        for (int k = 0; k < 2; ++k) {
            const int terms = 2 + (int)(rng.next() % 3);
            for (int t = 0; t < terms; ++t) term(k, i, avail[rng.next() % avail.size()], pool[rng.next() % pool.size()]);
        }
        const size_t ci = rng.next() % pool.size();
        const uint32_t out = (uint32_t)(S.num_inputs + i);
        term(2, i, out, pool[ci]);
        if (rng.next() & 1) term(2, i, avail[rng.next() % avail.size()], pool[rng.next() % pool.size()]);
        S.c_inv[i] = pool_inv[ci];
        S.has_out[i] = 1;
        avail.push_back(out);
    }
    for (int k = 0; k < 3; ++k) S.start[k].push_back(S.row[k].size());
    return S;
}
static std::vector<reef_fe> z_of(const Inst &I) {
    std::vector<reef_fe> z(I.W);
    z.push_back(I.u);
    z.insert(z.end(), I.X.begin(), I.X.end());
    return z;
}
static reef_fe row_dot(const Mod &m, const R1cs &S, int k, size_t i, const std::vector<reef_fe> &z, size_t skip = 0) {
    reef_fe s = {};
    for (size_t e = S.start[k][i] + skip; e < S.start[k][i + 1]; ++e) s = fadd(m, s, fmul(m, S.val[k][e], z[S.col[k][e]]));
    return s;
}
static std::vector<reef_fe> matvec(const Mod &m, const R1cs &S, int k, const std::vector<reef_fe> &z) {
    std::vector<reef_fe> out(S.num_cons);
    for (size_t i = 0; i < S.num_cons; ++i) out[i] = row_dot(m, S, k, i, z);
    return out;
}
// a fresh instance: u = 1, E = 0, random inputs and X, every output solved for in constraint order
static Inst fresh_instance(const Mod &m, const R1cs &S, uint64_t seed) {
    Rng rng{seed};
    std::vector<reef_fe> z(S.num_vars + 1 + S.num_io);
    for (size_t v = 0; v < S.num_inputs; ++v) z[v] = (rng.next() & 3) ? fsmall(m, rng.next() % 1000) : rng.full(m);
    z[S.num_vars] = m.one;
    for (size_t j = 0; j < S.num_io; ++j) z[S.num_vars + 1 + j] = rng.full(m);
    for (size_t i = 0; i < S.num_cons; ++i) {
        if (!S.has_out[i]) continue;
        const reef_fe ab = fmul(m, row_dot(m, S, 0, i, z), row_dot(m, S, 1, i, z));
        z[S.col[2][S.start[2][i]]] = fmul(m, fsub(m, ab, row_dot(m, S, 2, i, z, 1)), S.c_inv[i]);
    }
    Inst I;
    I.W.assign(z.begin(), z.begin() + S.num_vars);
    I.X.assign(z.begin() + S.num_vars + 1, z.end());
    I.u = m.one;
    I.E.assign(S.num_cons, reef_fe{});
    return I;
}

// ---- the checks: the verifier's equations on the host, and the honest prover's values under the recorded challenges -------------
// A rejected proof throws Rejected, naming the phase: nifs | spartan | open | hyrax.
struct Rejected : std::runtime_error { using std::runtime_error::runtime_error; };
[[noreturn]] static void reject(const char *phase, const std::string &what) {
    throw Rejected(std::string("proof check failed [") + phase + "]: " + what);
}
#define EXPECT(phase, cond, what) \
    do {                          \
        if (!(cond)) reject(phase, what); \
    } while (0)
// compares a point the device returned with dlog*G (dlog in Montgomery form); empty in the host-only self-test
using PointCheck = std::function<void(const char *phase, const reef_jacobian &pt, const reef_fe &dlog, const std::string &what)>;

struct PointRec { reef_jacobian pt; reef_fe dlog; std::string what; };
struct NifsRecord {                          // what the folding steps of one curve left, tracked on the host
    reef_fe dW = {}, dE = {}, u = {};         // discrete logarithms of comm_W, comm_E of the running instance; its u
    std::vector<reef_fe> X;
    std::vector<PointRec> points;             // comm_W and comm_T of every step with <W2, g>, <T, g>
};
template <class Pf> struct HyraxRec { Pf pf; std::vector<reef_fe> point; };

// the host's fold of a fresh instance (u2 = 1, E2 = 0) into the running one: returns T
static std::vector<reef_fe> host_cross_term(const Mod &m, const R1cs &S, const Inst &I1, const Inst &I2) {
    const std::vector<reef_fe> z1 = z_of(I1), z2 = z_of(I2);
    std::vector<reef_fe> T(S.num_cons);
    for (size_t i = 0; i < S.num_cons; ++i) {
        const reef_fe a1 = row_dot(m, S, 0, i, z1), b1 = row_dot(m, S, 1, i, z1), c1 = row_dot(m, S, 2, i, z1);
        const reef_fe a2 = row_dot(m, S, 0, i, z2), b2 = row_dot(m, S, 1, i, z2), c2 = row_dot(m, S, 2, i, z2);
        T[i] = fsub(m, fsub(m, fadd(m, fmul(m, a1, b2), fmul(m, a2, b1)), fmul(m, I1.u, c2)), c1);
    }
    return T;
}
static uint64_t host_violations(const Mod &m, const R1cs &S, const Inst &I) {
    const std::vector<reef_fe> z = z_of(I);
    uint64_t bad = 0;
    for (size_t i = 0; i < S.num_cons; ++i)
        if (!feq(fmul(m, row_dot(m, S, 0, i, z), row_dot(m, S, 1, i, z)), fadd(m, fmul(m, I.u, row_dot(m, S, 2, i, z)), I.E[i]))) ++bad;
    return bad;
}

static void check_nifs(const Mod &m, const NifsRecord &rec, const Inst &fin, const std::vector<reef_fe> &g, uint64_t violations, const PointCheck &pc,
                       const char *curve) {
    const char *ph = "nifs";
    const std::string c(curve);
    EXPECT(ph, violations == 0, c + ": " + std::to_string(violations) + " rows of the final running instance are not relaxed-satisfied");
    EXPECT(ph, feq(dot(m, fin.W.data(), g.data(), fin.W.size()), rec.dW), c + ": <W, gens> of the folded W differs from the tracked discrete log of comm_W");
    EXPECT(ph, feq(dot(m, fin.E.data(), g.data(), fin.E.size()), rec.dE), c + ": <E, gens> of the folded E differs from the tracked discrete log of comm_E");
    EXPECT(ph, feq(fin.u, rec.u) && fin.X.size() == rec.X.size(), c + ": u of the folded instance differs from 1 + sum of the challenges");
    for (size_t j = 0; j < fin.X.size(); ++j) EXPECT(ph, feq(fin.X[j], rec.X[j]), c + ": X of the folded instance differs from the host's fold");
    if (pc)
        for (const PointRec &p : rec.points) pc(ph, p.pt, p.dlog, c + " " + p.what);
}

// 3g's verifier: challenges as recorded, every evaluation straight from the unpadded shape and instance
template <class Pf> static void check_sumchecks(const Mod &m, const R1cs &S, const Inst &I, size_t ncp, size_t nvp, const Pf &pf, const char *curve) {
    const char *ph = "spartan";
    const std::string cn(curve);
    const size_t ell_x = reef_provider::log2_exact(ncp), ell_y = reef_provider::log2_exact(nvp) + 1;
    EXPECT(ph, pf.outer.size() == ell_x && pf.r_x.size() == ell_x && pf.tau.size() == ell_x, cn + ": outer rounds");
    EXPECT(ph, pf.inner.size() == ell_y && pf.r_y.size() == ell_y, cn + ": inner rounds");
    reef_fe claim = {};
    for (size_t i = 0; i < ell_x; ++i) {
        const reef_fe y[4] = {pf.outer[i][0], fsub(m, claim, pf.outer[i][0]), pf.outer[i][1], pf.outer[i][2]};
        claim = interp3(m, y, pf.r_x[i]);
    }
    const std::vector<reef_fe> z = z_of(I);
    const std::vector<reef_fe> erx = eq_evals(m, pf.r_x.data(), ell_x);
    reef_fe ev[3];
    for (int k = 0; k < 3; ++k) {
        const std::vector<reef_fe> mz = matvec(m, S, k, z);
        ev[k] = dot(m, erx.data(), mz.data(), S.num_cons);
    }
    const reef_fe ex = dot(m, erx.data(), I.E.data(), S.num_cons);
    EXPECT(ph, feq(pf.claims_outer[0], ev[0]) && feq(pf.claims_outer[1], ev[1]) && feq(pf.claims_outer[2], ev[2]) && feq(pf.claims_outer[3], ex),
           cn + ": claims_outer differ from AZ, BZ, CZ, E evaluated on the host at r_x");
    const reef_fe rhs = fmul(m, eq_at(m, pf.tau, pf.r_x), fsub(m, fsub(m, fmul(m, ev[0], ev[1]), fmul(m, I.u, ev[2])), ex));
    EXPECT(ph, feq(claim, rhs), cn + ": outer final claim != eq(tau, r_x) (AZ BZ - u CZ - E)");
    const reef_fe r = pf.r_joint, r2 = fmul(m, r, r);
    claim = fadd(m, fadd(m, ev[0], fmul(m, r, ev[1])), fmul(m, r2, ev[2]));
    for (size_t j = 0; j < ell_y; ++j) {
        const reef_fe y[3] = {pf.inner[j][0], fsub(m, claim, pf.inner[j][0]), pf.inner[j][1]};
        claim = interp2(m, y, pf.r_y[j]);
    }
    // the verifier's sparse evaluation: sum val eq(r_x)[row] eq(r_y)[col'] over A + r B + r^2 C, columns renumbered as R1CSShape::pad
    const std::vector<reef_fe> ery = eq_evals(m, pf.r_y.data(), ell_y);
    reef_fe abc = {};
    const reef_fe coef[3] = {m.one, r, r2};
    for (int k = 0; k < 3; ++k) {
        reef_fe s = {};
        for (size_t e = 0; e < S.row[k].size(); ++e) {
            const size_t c = S.col[k][e] < S.num_vars ? S.col[k][e] : S.col[k][e] + nvp - S.num_vars;
            s = fadd(m, s, fmul(m, fmul(m, S.val[k][e], erx[S.row[k][e]]), ery[c]));
        }
        abc = fadd(m, abc, fmul(m, coef[k], s));
    }
    // z(r_y) of z = W || 0 || u || X || 0: (1 - r_y[0]) W~(r_y[1..]) + r_y[0] (u, X)~(r_y[1..])
    const std::vector<reef_fe> eq1 = eq_evals(m, pf.r_y.data() + 1, ell_y - 1);
    const reef_fe eval_w = dot(m, eq1.data(), I.W.data(), S.num_vars);
    reef_fe ux = fmul(m, eq1[0], I.u);
    for (size_t j = 0; j < I.X.size(); ++j) ux = fadd(m, ux, fmul(m, eq1[1 + j], I.X[j]));
    const reef_fe zr = fadd(m, fmul(m, fsub(m, m.one, pf.r_y[0]), eval_w), fmul(m, pf.r_y[0], ux));
    EXPECT(ph, feq(pf.claims_inner[0], abc) && feq(pf.claims_inner[1], zr) && feq(pf.claims_inner[2], eval_w),
           cn + ": claims_inner differ from ABC(r_y), z(r_y), eval_W evaluated on the host");
    EXPECT(ph, feq(claim, fmul(m, abc, zr)), cn + ": inner final claim != ABC(r_y) z(r_y)");
}

// 3h / 3i's IPA in discrete-logarithm form: L = <a_lo, G_hi> + c_L q, R = <a_hi, G_lo> + c_R q; a' = a_lo r + a_hi r^-1,
// b' = b_lo r^-1 + b_hi r, G' = G_lo r^-1 + G_hi r.  next_r(k, L, R) gives round k's challenge.
struct IpaTrace { std::vector<reef_fe> dL, dR, rs; reef_fe a_hat = {}, b_hat = {}; };
static IpaTrace ipa_honest(const Mod &m, std::vector<reef_fe> a, std::vector<reef_fe> b, std::vector<reef_fe> G, const reef_fe &qd,
                           const std::function<reef_fe(size_t, const reef_fe &, const reef_fe &)> &next_r) {
    IpaTrace t;
    for (size_t k = 0; a.size() > 1; ++k) {
        const size_t h = a.size() / 2;
        const reef_fe c_l = dot(m, a.data(), b.data() + h, h), c_r = dot(m, a.data() + h, b.data(), h);
        t.dL.push_back(fadd(m, dot(m, a.data(), G.data() + h, h), fmul(m, c_l, qd)));
        t.dR.push_back(fadd(m, dot(m, a.data() + h, G.data(), h), fmul(m, c_r, qd)));
        const reef_fe r = next_r(k, t.dL.back(), t.dR.back()), ri = finv(m, r);
        t.rs.push_back(r);
        for (size_t i = 0; i < h; ++i) {
            a[i] = fadd(m, fmul(m, a[i], r), fmul(m, a[h + i], ri));
            b[i] = fadd(m, fmul(m, b[i], ri), fmul(m, b[h + i], r));
            G[i] = fadd(m, fmul(m, G[i], ri), fmul(m, G[h + i], r));
        }
        a.resize(h); b.resize(h); G.resize(h);
    }
    t.a_hat = a[0];
    t.b_hat = b[0];
    return t;
}
// the IPA verifier: comm + c q + sum (r_k^2 L_k + r_k^-2 R_k) == a_hat <s, G> + a_hat <s, b> q, s expanded from the challenges
static bool ipa_identity(const Mod &m, const reef_fe &d_comm, const reef_fe &c, const reef_fe &qd, const IpaTrace &t, const reef_fe &a_hat,
                         const std::vector<reef_fe> &G0, const std::vector<reef_fe> &b0) {
    reef_fe P = fadd(m, d_comm, fmul(m, c, qd));
    for (size_t k = 0; k < t.rs.size(); ++k) {
        const reef_fe r2 = fmul(m, t.rs[k], t.rs[k]);
        P = fadd(m, P, fadd(m, fmul(m, r2, t.dL[k]), fmul(m, finv(m, r2), t.dR[k])));
    }
    const std::vector<reef_fe> s = s_vector(m, t.rs);
    const reef_fe g_hat = dot(m, s.data(), G0.data(), s.size()), b_hat = dot(m, s.data(), b0.data(), s.size());
    return feq(P, fadd(m, fmul(m, a_hat, g_hat), fmul(m, fmul(m, a_hat, b_hat), qd)));
}

// the two instances of EE::prove_batch over [E, W]: a1 = E, b1 = eq(r_x); a2 = W, b2 = eq(r_y[1..]); zero-padded to n
struct OpenVectors { std::vector<reef_fe> a1, b1, a2, b2; };
template <class Pf> static OpenVectors open_vectors(const Mod &m, const Inst &I, size_t ncp, size_t nvp, const Pf &pf) {
    const size_t n = std::max(ncp, nvp);
    OpenVectors v;
    v.a1 = I.E; v.a1.resize(n);
    v.a2 = I.W; v.a2.resize(n);
    v.b1 = eq_evals(m, pf.r_x.data(), pf.r_x.size()); v.b1.resize(n);
    v.b2 = eq_evals(m, pf.r_y.data() + 1, pf.r_y.size() - 1); v.b2.resize(n);
    return v;
}
static std::vector<reef_fe> lin(const Mod &m, const std::vector<reef_fe> &x, const reef_fe &r, const std::vector<reef_fe> &y) {   // x + r y
    std::vector<reef_fe> o(x.size());
    for (size_t i = 0; i < x.size(); ++i) o[i] = fadd(m, x[i], fmul(m, r, y[i]));
    return o;
}

template <class Pf> static void check_opening(const Mod &m, const Inst &I, size_t ncp, size_t nvp, const Pf &pf, const std::vector<reef_fe> &g,
                                              const reef_fe &dW, const reef_fe &dE, const reef_fe &gs, const PointCheck &pc, const char *curve) {
    const char *ph = "open";
    const std::string cn(curve);
    const size_t n = std::max(ncp, nvp), rounds = reef_provider::log2_exact(n);
    EXPECT(ph, pf.r_rounds.size() == rounds && (!pc || (pf.L.size() == rounds && pf.R.size() == rounds)) && g.size() == n, cn + ": IPA rounds");
    const OpenVectors v = open_vectors(m, I, ncp, nvp, pf);
    const reef_fe cross = fadd(m, dot(m, v.a1.data(), v.b2.data(), n), dot(m, v.a2.data(), v.b1.data(), n));
    EXPECT(ph, feq(pf.cross_term, cross), cn + ": cross_term differs from <E, eq(r_y[1..])> + <W, eq(r_x)>");
    const reef_fe r = pf.r_fold;
    const std::vector<reef_fe> a = lin(m, v.a1, r, v.a2), b = lin(m, v.b1, r, v.b2);
    EXPECT(ph, feq(pf.c, dot(m, a.data(), b.data(), n)), cn + ": c differs from <a, b> of the folded instance");
    // the verifier's c: eval_E + r^2 eval_W + r cross, from the sum-checks' claims
    const reef_fe c_v = fadd(m, fadd(m, pf.claims_outer[3], fmul(m, fmul(m, r, r), pf.claims_inner[2])), fmul(m, r, pf.cross_term));
    EXPECT(ph, feq(pf.c, c_v), cn + ": c differs from eval_E + r^2 eval_W + r cross_term");
    const reef_fe qd = fmul(m, gs, pf.r_ipa), d_comm_a = fadd(m, dE, fmul(m, r, dW));
    const IpaTrace t = ipa_honest(m, a, b, g, qd, [&](size_t k, const reef_fe &, const reef_fe &) { return pf.r_rounds[k]; });
    if (pc)
        for (size_t k = 0; k < rounds; ++k) {
            pc(ph, pf.L[k], t.dL[k], cn + " L_" + std::to_string(k));
            pc(ph, pf.R[k], t.dR[k], cn + " R_" + std::to_string(k));
        }
    EXPECT(ph, feq(pf.a_hat, t.a_hat), cn + ": a_hat differs from the honest prover's");
    EXPECT(ph, ipa_identity(m, d_comm_a, c_v, qd, t, pf.a_hat, g, b), cn + ": the IPA verifier's identity fails");
}

// LZ = L^T Z over the zero-padded document (2^left rows of `cols` symbols)
static std::vector<reef_fe> host_lz(const Mod &m, const std::vector<uint8_t> &doc, size_t cols, const std::vector<reef_fe> &L) {
    reef_fe sym[256];
    for (int s = 0; s < 256; ++s) sym[s] = fsmall(m, (uint64_t)s);
    std::vector<reef_fe> lz(cols);
    for (size_t i = 0; i < L.size(); ++i)
        for (size_t j = 0; j < cols && i * cols + j < doc.size(); ++j)
            if (const uint8_t v = doc[i * cols + j]) lz[j] = fadd(m, lz[j], fmul(m, L[i], sym[v]));
    return lz;
}
template <class Pf> static void check_hyrax(const Mod &m, const std::vector<uint8_t> &doc, size_t num_vars, size_t left, const std::vector<reef_fe> &point,
                                            const Pf &pf, const std::vector<reef_fe> &g, const std::vector<reef_fe> &blinds, const reef_fe &hd, const reef_fe &g1,
                                            const PointCheck &pc) {
    const char *ph = "hyrax";
    const size_t right = num_vars - left, cols = (size_t)1 << right;
    EXPECT(ph, point.size() == num_vars && pf.r_rounds.size() == right && (!pc || (pf.L.size() == right && pf.R.size() == right)) && g.size() == cols, "IPA rounds");
    const std::vector<reef_fe> L = eq_evals(m, point.data(), left), Rv = eq_evals(m, point.data() + left, right);
    const std::vector<reef_fe> lz = host_lz(m, doc, cols, L);
    const reef_fe ev = dot(m, lz.data(), Rv.data(), cols);
    EXPECT(ph, feq(pf.eval, ev), "eval differs from the host's evaluation of the document polynomial at the point");
    const reef_fe lzb = dot(m, L.data(), blinds.data(), L.size());
    EXPECT(ph, feq(pf.lz_blind, lzb), "lz_blind differs from sum_i L_i blind_i");
    const reef_fe d_lz = fadd(m, dot(m, lz.data(), g.data(), cols), fmul(m, lzb, hd));   // sum_i L_i C_i, C_i = <Z_i, G> + blind_i h
    if (pc) pc(ph, pf.comm_lz, d_lz, "comm_LZ");
    const reef_fe qd = fmul(m, g1, pf.r_q);
    const IpaTrace t = ipa_honest(m, lz, Rv, g, qd, [&](size_t k, const reef_fe &, const reef_fe &) { return pf.r_rounds[k]; });
    if (pc)
        for (size_t k = 0; k < right; ++k) {
            pc(ph, pf.L[k], t.dL[k], "L_" + std::to_string(k));
            pc(ph, pf.R[k], t.dR[k], "R_" + std::to_string(k));
        }
    EXPECT(ph, feq(pf.a_hat, t.a_hat) && feq(pf.b_hat, t.b_hat), "a_hat / b_hat differ from the honest prover's");
    // plain rounds: the blind of comm_LZ is the only multiple of h in P
    EXPECT(ph, ipa_identity(m, fsub(m, d_lz, fmul(m, lzb, hd)), pf.eval, qd, t, pf.a_hat, g, Rv), "the IPA verifier's identity fails");
}

// which recorded value tamper=<phase> changes (one per phase; nothing that was sent to the device)
static const char *const TAMPER_PHASES[] = {"nifs", "spartan", "open", "hyrax"};
static void check_tamper_name(const std::string &t) {
    if (t.empty()) return;
    for (const char *p : TAMPER_PHASES)
        if (t == p) return;
    fail("tamper=" + t + ": one of nifs, spartan, open, hyrax");
}
template <class Pf, class Hf> static void apply_tamper(const Mod &m, const std::string &t, NifsRecord &rec, Pf &pf, Hf *hyrax) {
    if (t == "nifs") rec.dE = fadd(m, rec.dE, m.one);                           // the tracked discrete log of comm_E
    else if (t == "spartan") pf.claims_outer[0] = fadd(m, pf.claims_outer[0], m.one);   // claim_Az
    else if (t == "open") pf.a_hat = fadd(m, pf.a_hat, m.one);
    else if (t == "hyrax" && hyrax) hyrax->eval = fadd(m, hyrax->eval, m.one);
}

// ---- the host-only self-test: a tiny honest transcript, produced on the host, through the same checks --------------------------------
template <class Pf> static void spartan_honest(const Mod &m, const R1cs &S, const Inst &I, size_t ncp, size_t nvp, const reef_provider::Transcript &tr, Pf &pf) {
    const size_t ell_x = reef_provider::log2_exact(ncp), ell_y = reef_provider::log2_exact(nvp) + 1;
    const std::vector<reef_fe> z = z_of(I);
    std::vector<reef_fe> az = matvec(m, S, 0, z), bz = matvec(m, S, 1, z), cz = matvec(m, S, 2, z), e = I.E;
    az.resize(ncp); bz.resize(ncp); cz.resize(ncp); e.resize(ncp);
    std::vector<reef_fe> d(ncp);
    for (size_t i = 0; i < ncp; ++i) d[i] = fadd(m, fmul(m, I.u, cz[i]), e[i]);
    for (size_t j = 0; j < ell_x; ++j) pf.tau.push_back(tr("t", nullptr, 0));
    std::vector<reef_fe> eqt = eq_evals(m, pf.tau.data(), ell_x), a = az, b = bz;
    auto bind = [&](std::vector<reef_fe> &x, const reef_fe &r) {
        const size_t h = x.size() / 2;
        for (size_t i = 0; i < h; ++i) x[i] = fadd(m, x[i], fmul(m, r, fsub(m, x[h + i], x[i])));
        x.resize(h);
    };
    auto at = [&](const std::vector<reef_fe> &x, size_t i, uint64_t t) { return fadd(m, x[i], fmul(m, fsmall(m, t), fsub(m, x[x.size() / 2 + i], x[i]))); };
    for (size_t k = 0; k < ell_x; ++k) {
        std::array<reef_fe, 3> ev = {};
        const uint64_t ts[3] = {0, 2, 3};
        for (int q = 0; q < 3; ++q)
            for (size_t i = 0; i < eqt.size() / 2; ++i)
                ev[q] = fadd(m, ev[q], fmul(m, at(eqt, i, ts[q]), fsub(m, fmul(m, at(a, i, ts[q]), at(b, i, ts[q])), at(d, i, ts[q]))));
        pf.outer.push_back(ev);
        pf.r_x.push_back(tr("outer", ev.data(), sizeof ev));
        for (auto *x : {&eqt, &a, &b, &d}) bind(*x, pf.r_x.back());
    }
    const std::vector<reef_fe> erx = eq_evals(m, pf.r_x.data(), ell_x);
    pf.claims_outer = {a[0], b[0], dot(m, erx.data(), cz.data(), ncp), dot(m, erx.data(), e.data(), ncp)};
    pf.r_joint = tr("claims_outer", pf.claims_outer.data(), sizeof pf.claims_outer);
    const reef_fe coef[3] = {m.one, pf.r_joint, fmul(m, pf.r_joint, pf.r_joint)};
    std::vector<reef_fe> abc(2 * nvp), zt(2 * nvp);
    for (int k = 0; k < 3; ++k)
        for (size_t q = 0; q < S.row[k].size(); ++q) {
            const size_t c = S.col[k][q] < S.num_vars ? S.col[k][q] : S.col[k][q] + nvp - S.num_vars;
            abc[c] = fadd(m, abc[c], fmul(m, coef[k], fmul(m, erx[S.row[k][q]], S.val[k][q])));
        }
    for (size_t i = 0; i < S.num_vars; ++i) zt[i] = I.W[i];
    zt[nvp] = I.u;
    for (size_t j = 0; j < I.X.size(); ++j) zt[nvp + 1 + j] = I.X[j];
    for (size_t k = 0; k < ell_y; ++k) {
        std::array<reef_fe, 2> ev = {};
        const uint64_t ts[2] = {0, 2};
        for (int q = 0; q < 2; ++q)
            for (size_t i = 0; i < abc.size() / 2; ++i) ev[q] = fadd(m, ev[q], fmul(m, at(abc, i, ts[q]), at(zt, i, ts[q])));
        pf.inner.push_back(ev);
        pf.r_y.push_back(tr("inner", ev.data(), sizeof ev));
        bind(abc, pf.r_y.back());
        bind(zt, pf.r_y.back());
    }
    const std::vector<reef_fe> eq1 = eq_evals(m, pf.r_y.data() + 1, ell_y - 1);
    pf.claims_inner = {abc[0], zt[0], dot(m, eq1.data(), I.W.data(), S.num_vars)};
}
template <class Pf> static void open_honest(const Mod &m, const Inst &I, size_t ncp, size_t nvp, const std::vector<reef_fe> &g, const reef_fe &dW,
                                            const reef_fe &dE, const reef_fe &gs, const reef_provider::Transcript &tr, Pf &pf) {
    const size_t n = std::max(ncp, nvp);
    const OpenVectors v = open_vectors(m, I, ncp, nvp, pf);
    pf.cross_term = fadd(m, dot(m, v.a1.data(), v.b2.data(), n), dot(m, v.a2.data(), v.b1.data(), n));
    pf.r_fold = tr("r", &pf.cross_term, sizeof(reef_fe));
    const std::vector<reef_fe> a = lin(m, v.a1, pf.r_fold, v.a2), b = lin(m, v.b1, pf.r_fold, v.b2);
    pf.c = dot(m, a.data(), b.data(), n);
    const reef_fe u[2] = {fadd(m, dE, fmul(m, pf.r_fold, dW)), pf.c};
    pf.r_ipa = tr("r", u, sizeof u);
    const IpaTrace t = ipa_honest(m, a, b, g, fmul(m, gs, pf.r_ipa), [&](size_t, const reef_fe &l, const reef_fe &r) {
        const reef_fe lr[2] = {l, r};
        return tr("challenge_r", lr, sizeof lr);
    });
    pf.r_rounds = t.rs;
    pf.a_hat = t.a_hat;
}

static std::string check_selftest(const std::string &tamper) {
    using Pf = reef_provider::RelaxedR1CSSnark<REEF_PALLAS>::Proof;
    using Hf = reef_provider::HyraxEval<REEF_PALLAS>::Proof;
    check_tamper_name(tamper);
    const Mod m(ORDER[0]);
    const size_t num_cons = 12, num_vars = 15, ncp = 16, nvp = 16;
    const R1cs S = layered_r1cs(m, num_cons, num_vars, 0x5E1F);
    std::vector<reef_fe> g(ncp);
    for (size_t i = 0; i < ncp; ++i) g[i] = fsmall(m, 0xC0FFEE + 7 * i);
    StandinTranscript T(m, 1);
    const reef_provider::Transcript tr = T.fn();
    // the NIFS: three fresh instances folded into the first, on the host, the discrete logs of comm_W and comm_E tracked
    Inst run = fresh_instance(m, S, 1);
    NifsRecord rec;
    rec.dW = dot(m, run.W.data(), g.data(), num_vars);
    rec.u = run.u;
    rec.X = run.X;
    for (int s = 0; s < 3; ++s) {
        const Inst f = fresh_instance(m, S, 10 + s);
        const std::vector<reef_fe> Tv = host_cross_term(m, S, run, f);
        const reef_fe d[2] = {dot(m, f.W.data(), g.data(), num_vars), dot(m, Tv.data(), g.data(), num_cons)};
        const reef_fe r = tr("fold", d, sizeof d);
        run.W = lin(m, run.W, r, f.W);
        run.E = lin(m, run.E, r, Tv);
        run.u = fadd(m, run.u, r);
        run.X = lin(m, run.X, r, f.X);
        rec.dW = fadd(m, rec.dW, fmul(m, r, d[0]));
        rec.dE = fadd(m, rec.dE, fmul(m, r, d[1]));
        rec.u = fadd(m, rec.u, r);
        rec.X = lin(m, rec.X, r, f.X);
    }
    const uint64_t violations = host_violations(m, S, run);
    Pf pf;
    spartan_honest(m, S, run, ncp, nvp, tr, pf);
    const reef_fe gs = fsmall(m, 0x5EED);
    open_honest(m, run, ncp, nvp, g, rec.dW, rec.dE, gs, tr, pf);
    // the Hyrax argument over a 2^6-symbol document as 2^3 x 2^3
    const size_t hv = 6, left = 3;
    std::vector<uint8_t> doc(50);
    for (size_t i = 0; i < doc.size(); ++i) doc[i] = (uint8_t)((i * 37 + 11) % 131);
    std::vector<reef_fe> hg(8), blinds(8), point(hv);
    for (size_t i = 0; i < 8; ++i) { hg[i] = fsmall(m, 0xFEED + 3 * i); blinds[i] = fsmall(m, 1000003 * (i + 1)); }
    for (size_t j = 0; j < hv; ++j) point[j] = tr("q", nullptr, 0);
    const reef_fe hd = fsmall(m, 0xB11D), g1 = fsmall(m, 0x6E1);
    Hf hf;
    {
        const std::vector<reef_fe> L = eq_evals(m, point.data(), left), Rv = eq_evals(m, point.data() + left, hv - left);
        const std::vector<reef_fe> lz = host_lz(m, doc, 8, L);
        hf.eval = dot(m, lz.data(), Rv.data(), 8);
        hf.lz_blind = dot(m, L.data(), blinds.data(), 8);
        const reef_fe u[2] = {fadd(m, dot(m, lz.data(), hg.data(), 8), fmul(m, hf.lz_blind, hd)), hf.eval};
        hf.r_q = tr("r", u, sizeof u);
        const IpaTrace t = ipa_honest(m, lz, Rv, hg, fmul(m, g1, hf.r_q), [&](size_t, const reef_fe &l, const reef_fe &r) {
            const reef_fe lr[2] = {l, r};
            return tr("challenge_r", lr, sizeof lr);
        });
        hf.r_rounds = t.rs;
        hf.a_hat = t.a_hat;
        hf.b_hat = t.b_hat;
    }
    apply_tamper(m, tamper, rec, pf, &hf);
    const PointCheck none;
    check_nifs(m, rec, run, g, violations, none, "pallas");
    check_sumchecks(m, S, run, ncp, nvp, pf, "pallas");
    check_opening(m, run, ncp, nvp, pf, g, rec.dW, rec.dE, gs, none, "pallas");
    check_hyrax(m, doc, hv, left, point, hf, hg, blinds, hd, g1, none);
    char line[512];
    snprintf(line, sizeof line, "{\"selftest\": \"accepted\", \"num_cons\": %zu, \"num_vars\": %zu, \"nnz\": %zu, \"outer_rounds\": %zu, \"inner_rounds\": %zu, "
             "\"ipa_rounds\": %zu, \"hyrax_rounds\": %zu, \"tamper\": \"%s\"}", num_cons, num_vars, S.nnz(), pf.outer.size(), pf.inner.size(), pf.r_rounds.size(),
             hf.r_rounds.size(), tamper.c_str());
    return line;
}

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
    reef_affine g1;
    CK(reef_gen_bases(CURVE, 1, 0, 1, &g1, REEF_HOST));
    reef_msm_opts og = {};
    og.bucket_groups = 1;
    og.device = -1;
    CK(reef_msm_ctx_create(&s.c.one, CURVE, &g1, 1, REEF_HOST, &og));
    s.one_owner.reset(s.c.one);
    reef_msm_opts o = {};
    o.bucket_groups = 1;
    o.byte_tables = tables ? 1 : 2;
    o.device = -1;
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
        reef_jacobian both[2] = {pt, {}};
        CK(reef_msm(c->one, &dlog, 1, REEF_HOST, true, &both[1], REEF_HOST));
        reef_affine aff[2];
        CK(reef_normalize(c->id, both, 2, REEF_HOST, aff, nullptr));
        if (memcmp(&aff[0], &aff[1], sizeof(reef_affine)) != 0) reject(phase, what + " differs from its discrete-logarithm closed form");
        ++g_checked;
    };
}

// the first running instance (u = 1, E = 0) and its comm_W
template <int CURVE> static void nifs_init(ProveSide<CURVE> &s, const Inst &f0) {
    const auto t0 = clk::now();
    s.nifs->set_running(f0.W.data(), nullptr, f0.u, f0.X.data(), REEF_HOST, true);
    reef_jacobian cw;
    CK(reef_msm(s.c.key, f0.W.data(), s.num_vars, REEF_HOST, true, &cw, REEF_HOST));
    s.tr.absorb("U1", &cw, sizeof cw);
    s.init_ms = ms_since(t0);
    s.rec.dW = dot(s.m, f0.W.data(), s.g.data(), s.num_vars);
    s.rec.u = f0.u;
    s.rec.X = f0.X;
    s.rec.points.push_back({cw, s.rec.dW, "comm_W of the first instance"});
}
// one NIFS::prove of a folding step: comm_W of the fresh witness (scalars from host memory), commit_T, the challenge, the fold
struct StepOut { reef_jacobian comm_W, comm_T; reef_fe r; double commit_w_ms, nifs_ms; };
template <int CURVE> static StepOut step_fold(ProveSide<CURVE> &s, const Inst &f) {
    StepOut o;
    const auto t0 = clk::now();
    CK(reef_msm(s.c.key, f.W.data(), s.num_vars, REEF_HOST, true, &o.comm_W, REEF_HOST));
    const auto t1 = clk::now();
    o.commit_w_ms = std::chrono::duration<double, std::milli>(t1 - t0).count();
    o.comm_T = s.nifs->commit_T(s.c.key, f.W.data(), f.X.data(), REEF_HOST, true);
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
            return std::vector<uint8_t>((const uint8_t *)&d, (const uint8_t *)&d + sizeof d);
        },
        [&](const reef_fe &r) { return scaled_G(s, fmul(s.m, s.gs, r)); }, s.pf);
    s.open_ms = ms_since(t0);
}
template <int CURVE> static void read_back(ProveSide<CURVE> &s) {
    s.fin.W = s.nifs->read(0, s.num_vars, true);
    s.fin.E = s.nifs->read(1, s.num_cons, true);
    s.fin.u = s.nifs->read(3, 1, true)[0];
    s.fin.X = s.nifs->read(4, s.S.num_io, true);
    s.violations = s.nifs->check_relaxed();
}

static std::string prove_body(const Shape &shape, const std::string &tamper, bool tables) {
    const Shape *sh = &shape;
    check_tamper_name(tamper);
    if (tamper == "hyrax" && !sh->doc_log) fail("tamper=hyrax: " + sh->name + " has no Hyrax consistency argument");
    const Mod mp(ORDER[REEF_PALLAS]), mv(ORDER[REEF_VESTA]);
    ProveSide<REEF_PALLAS> P(mp, "pallas", sh->c1, sh->w1, 0xA11A5);
    ProveSide<REEF_VESTA> V(mv, "vesta", sh->c2, sh->w2, 0x7E57A);
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
        reef_msm_opts o = {};
        o.bucket_groups = 1;
        o.byte_tables = tables ? 1 : 2;
        o.device = -1;
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
        hyrax->prove(row_key, point.data(), row_aff.data(), REEF_HOST, tr, [&](const reef_fe &r) { return scaled_G(P, fmul(mp, g1, r)); }, hpf);
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
             "\"check_ms\": %.3f, \"points_checked\": %d, \"proof_checked\": true}",
             sh->name.c_str(), sh->w1, sh->c1, sh->w2, sh->c2, P.ncp, P.nvp, V.ncp, V.nvp, P.n, V.n, P.S.nnz(), V.S.nnz(), sh->steps, P.init_ms + V.init_ms,
             steps_list.c_str(), steps_total / ns, commit_w_ms / ns, nifs_ms / ns, sc_ms / ns, final_fold_ms, P.spartan_ms, V.spartan_ms, P.pf.outer.size(),
             P.pf.inner.size(), V.pf.outer.size(), V.pf.inner.size(), P.open_ms, V.open_ms, P.pf.r_rounds.size(), V.pf.r_rounds.size(), sh->doc_log, left,
             consistency_ms, hpf.r_rounds.size(), commit_hyrax_ms, hyrax_create_ms, total, check_ms, g_checked);
    return std::string(line.data());
}

// ---- entry points ---------------------------------------------------------------------------------------------------
// Runs the replay of the config whose name contains `config` ("cfg1" | "cfg3" | "cfg4" | "cfg5") with the shapes of
// `shapes_json` (NULL: $REEF_REPLAY_SHAPES).  On success returns 0 and writes the JSON line (NUL-terminated) to out; on
// failure returns non-zero and writes the message.  Every per-step commitment has been checked by then.
// reef_replay_run_devices: the same, followed by the multi-device leg on `devices[0 .. ndev)` (ordinals may repeat; ndev = 0: none).
extern "C" __attribute__((visibility("default")))
int reef_replay_run_devices(const char *shapes_json, const char *config, int nofold, int tables, const int *devices, size_t ndev, char *out, size_t cap) {
    auto put = [&](const std::string &m) { if (out && cap) { snprintf(out, cap, "%s", m.c_str()); } };
    try {
        std::vector<int> ordinals;
        if (ndev > 64 || (ndev && !devices)) fail("devices: 0..64 ordinals");
        for (size_t i = 0; i < ndev; ++i) {
            if (devices[i] < 0 || devices[i] >= reef_device_count()) fail("devices: ordinal " + std::to_string(devices[i]) + " is not visible");
            ordinals.push_back(devices[i]);
        }
        if (ndev && !nofold) fail("the multi-device leg replays the fold-free final SNARK: pass nofold");
        const char *path = shapes_json && *shapes_json ? shapes_json : getenv("REEF_REPLAY_SHAPES");
        if (!path) fail("no replay shapes file given (argument or REEF_REPLAY_SHAPES)");
        if (reef_device_count() < 1) { put(std::string("no GPU: ") + reef_last_error()); return 3; }
        const Shape sh = load_shape(path, config && *config ? config : "cfg3");
        g_checked = 0;
        put(replay_body(sh, nofold != 0, tables != 0, path, ordinals));
        return 0;
    } catch (const std::exception &e) {
        put(e.what());
        return 1;
    }
}
extern "C" __attribute__((visibility("default")))
int reef_replay_run(const char *shapes_json, const char *config, int nofold, int tables, char *out, size_t cap) {
    return reef_replay_run_devices(shapes_json, config, nofold, tables, nullptr, 0, out, cap);
}

// The prove leg of the config whose name contains `config`.  flags: space-separated options -- "tamper=<phase>" (nifs | spartan |
// open | hyrax) alters one recorded value before the checks, so the run must fail naming that phase; "tables" builds the keys'
// byte tables.  Returns 0 and the JSON line, 1 and the message (a failed call or a rejected proof), 3 without a GPU.
extern "C" __attribute__((visibility("default")))
int reef_replay_run_prove(const char *shapes_json, const char *config, const char *flags, char *out, size_t cap) {
    auto put = [&](const std::string &m) { if (out && cap) { snprintf(out, cap, "%s", m.c_str()); } };
    try {
        std::string tamper;
        bool tables = false;
        const std::string f = flags ? flags : "";
        for (size_t p = 0; p < f.size();) {
            const size_t e = std::min(f.find(' ', p), f.size());
            const std::string w = f.substr(p, e - p);
            if (w.rfind("tamper=", 0) == 0) tamper = w.substr(7);
            else if (w == "tables") tables = true;
            else if (!w.empty()) fail("reef_replay_run_prove: unknown flag '" + w + "'");
            p = e + 1;
        }
        check_tamper_name(tamper);
        const char *path = shapes_json && *shapes_json ? shapes_json : getenv("REEF_REPLAY_SHAPES");
        if (!path) fail("no replay shapes file given (argument or REEF_REPLAY_SHAPES)");
        if (reef_device_count() < 1) { put(std::string("no GPU: ") + reef_last_error()); return 3; }
        const Shape sh = load_shape(path, config && *config ? config : "cfg3");
        g_checked = 0;
        put(prove_body(sh, tamper, tables));
        return 0;
    } catch (const std::exception &e) {
        put(e.what());
        return 1;
    }
}
// The prove leg's checks on a tiny honest transcript made on the host (no GPU): the NIFS bookkeeping, the sum-check identities, the
// sparse evaluation and the IPA identities.  tamper: NULL / "" or one phase, as above.  Returns 0 and a JSON line when every check
// accepts, 1 and the message naming the phase when one rejects, 2 on a usage error.
extern "C" __attribute__((visibility("default")))
int reef_replay_check_selftest(const char *tamper, char *out, size_t cap) {
    auto put = [&](const std::string &m) { if (out && cap) { snprintf(out, cap, "%s", m.c_str()); } };
    try {
        put(check_selftest(tamper ? tamper : ""));
        return 0;
    } catch (const Rejected &e) {
        put(e.what());
        return 1;
    } catch (const std::exception &e) {
        put(e.what());
        return 2;
    }
}

#if !defined(REEF_REPLAY_NO_MAIN)
#include <unistd.h>
int main(int argc, char **argv) {
    const char *which = argc > 1 ? argv[1] : "cfg3";
    bool nofold = false, tables = false;
    std::string shapes;
    int members = 0;
    bool prove = false;
    std::string prove_flags;
    {   // an embedder's first call: eight hardware queues for the concurrent arguments, asked for before the first HIP call
        reef_runtime_opts ro = {};
        ro.hw_queues = 8;
        (void)reef_runtime_init(&ro, nullptr);
    }
    for (int i = 2; i < argc; ++i) {
        if (strcmp(argv[i], "nofold") == 0) nofold = true;
        else if (strcmp(argv[i], "tables") == 0) tables = true;       // the keys' byte tables are ready before the first MSM (a real run builds them in the background)
        else if (strncmp(argv[i], "shapes=", 7) == 0) shapes = argv[i] + 7;
        else if (strncmp(argv[i], "devices=", 8) == 0) members = atoi(argv[i] + 8);     // the multi-device leg on N members (ordinal i mod the visible devices)
        else if (strcmp(argv[i], "prove") == 0) prove = true;                          // the prove leg: every device row of one proof, checked
        else if (strncmp(argv[i], "tamper=", 7) == 0) prove_flags += std::string(" ") + argv[i];
        else { fprintf(stderr, "usage: reef_replay [cfg1|cfg3|cfg4|cfg4b|cfg5] [nofold] [tables] [devices=N] [shapes=<replay_shapes.json>] | [prove [tamper=<phase>]]\n"); return 2; }
    }
    if (shapes.empty() && !getenv("REEF_REPLAY_SHAPES")) {   // the executable lives in reef_amd/_lib/: the shapes are two levels up, under tests/golden/
        char exe[4096];
        const ssize_t len = readlink("/proc/self/exe", exe, sizeof exe - 1);
        if (len > 0) {
            exe[len] = 0;
            std::string dir(exe);
            dir = dir.substr(0, dir.rfind('/'));
            shapes = dir + "/../../tests/golden/replay_shapes.json";
        }
    }
    std::vector<char> out(32768);
    if (prove) {
        if (tables) prove_flags += " tables";
        const int rc = reef_replay_run_prove(shapes.empty() ? nullptr : shapes.c_str(), which, prove_flags.c_str(), out.data(), out.size());
        if (rc == 0) printf("%s\n", out.data());
        else fprintf(stderr, "reef_replay: %s\n", out.data());
        return rc;
    }
    std::vector<int> ordinals;
    const int visible = reef_device_count();
    for (int i = 0; i < members && visible > 0; ++i) ordinals.push_back(i % visible);
    const int rc = reef_replay_run_devices(shapes.empty() ? nullptr : shapes.c_str(), which, nofold, tables, ordinals.data(), ordinals.size(), out.data(), out.size());
    if (rc == 0) printf("%s\n", out.data());
    else fprintf(stderr, "reef_replay: %s\n", out.data());
    return rc;
}
#endif
