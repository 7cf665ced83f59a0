// proof_check.hpp -- the verifier of the replay's prove leg (`reef_replay cfgN prove`, replay_prove.hpp): host scalar arithmetic, the
// stand-in transcript, the synthetic R1CS, the verifier's equations, the honest host prover and the self-test over them.  Host only:
// it takes its types from reef_msm.h and the Proof structs from reef_provider.hpp and calls nothing of the library, so
// proof_check_selftest.cpp builds from it with plain g++ and no -lreef_msm (host/Makefile).
#pragma once
#include <algorithm>
#include <cstdio>

#include "reef_msm.h"
#include "reef_provider.hpp"   // the Proof structs; and <array>, <cstring>, <functional>, <stdexcept>, <string>, <vector>

// a failed call or a usage error ends the replay with its message (the entry points return it; the executables print it and exit non-zero)
[[noreturn]] static void fail(const std::string &msg) { throw std::runtime_error(msg); }

static const uint64_t ORDER[2][4] = {   // group orders: Pallas (= Fq), Vesta (= Fp); little-endian limbs
    {0x8c46eb2100000001ULL, 0x224698fc0994a8ddULL, 0x0ULL, 0x4000000000000000ULL},
    {0x992d30ed00000001ULL, 0x224698fc094cf91bULL, 0x0ULL, 0x4000000000000000ULL}};

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

// The verifier's matrix evaluations on one host core: {A~, B~, C~}(r_x, r_y) = sum val eq(r_x)[row] eq(r_y)[col'] per matrix, columns
// renumbered as R1CSShape::pad; erx = eq(r_x), ery = eq(r_y).  What reef_spartan_eval_matrices (3k) does on the device.
static std::array<reef_fe, 3> host_matrix_evals(const Mod &m, const R1cs &S, size_t nvp, const std::vector<reef_fe> &erx, const std::vector<reef_fe> &ery) {
    std::array<reef_fe, 3> out;
    for (int k = 0; k < 3; ++k) {
        reef_fe s = {};
        for (size_t e = 0; e < S.row[k].size(); ++e) {
            const size_t c = S.col[k][e] < S.num_vars ? S.col[k][e] : S.col[k][e] + nvp - S.num_vars;
            s = fadd(m, s, fmul(m, fmul(m, S.val[k][e], erx[S.row[k][e]]), ery[c]));
        }
        out[k] = s;
    }
    return out;
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
    // the verifier's sparse evaluation over A + r B + r^2 C
    const std::vector<reef_fe> ery = eq_evals(m, pf.r_y.data(), ell_y);
    const std::array<reef_fe, 3> mev = host_matrix_evals(m, S, nvp, erx, ery);
    const reef_fe abc = fadd(m, fadd(m, mev[0], fmul(m, r, mev[1])), fmul(m, r2, mev[2]));
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
