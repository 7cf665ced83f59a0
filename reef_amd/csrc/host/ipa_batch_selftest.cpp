// The host preparation of reef_ipa_check_batch (../ipa_batch_host.inc over ../fe_scalars_host.inc and ../field.h) alone: no HIP, no
// library, its own main.  Checks, on both fields: the inverses from the one shared inversion (r r^-1 = 1); the closed-form b_hat against
// the dot product <s, pad(eq(p))> written out entry by entry (k = 1, 2, 9; one and two points; v = 0, v < k, v = k); the scalars of the
// one-off points against their definitions; every refusal the preparation owns, with the proof's index in the message.
//   g++ -O2 -std=c++17 -Wall -Wno-unknown-pragmas -DREEF_BOUNDS ipa_batch_selftest.cpp -I../../../include -o ipa_batch_selftest      (REEF_BOUNDS: field.h checks every
//   stated limb and value bound as it goes);  it may also be built with -fsanitize=address,undefined: tests/test_ipa_batch_selftest.py does
#include <stdarg.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <type_traits>
#include <vector>

#include "reef_msm.h"
#include "../field.h"

namespace reef {
static char g_error[512];
static void set_error(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static void set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}
}  // namespace reef
#define REEF_TRY(expr)                \
    do {                              \
        reef_status s_ = (expr);      \
        if (s_ != REEF_OK) return s_; \
    } while (0)
#include "../fe_scalars_host.inc"
#include "../ipa_batch_host.inc"

using namespace reef;

static int g_failed = 0;
#define EXPECT(cond, ...)                                   \
    do {                                                    \
        if (!(cond)) {                                      \
            ++g_failed;                                     \
            printf("FAILED %s:%d: ", __FILE__, __LINE__);   \
            printf(__VA_ARGS__);                            \
            printf("\n");                                   \
        }                                                   \
    } while (0)

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t next64() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return g_state;
}
static reef_fe rand_fe() {                                       // a canonical integer below 2^254 (below either modulus)
    reef_fe x;
    for (int i = 0; i < 4; ++i) x.l[i] = next64();
    x.l[3] &= (1ull << 62) - 1;
    return x;
}
template <int F> static fe in(const reef_fe &x) { return fe_import<F>(&x, false); }
template <int F> static bool same(const fe &a, const fe &b) {
    const fe256 x = fe_to_integer<F>(a), y = fe_to_integer<F>(b);
    return memcmp(&x, &y, sizeof x) == 0;
}
template <int F> static bool same_int(const fe256 &got, const fe &want) {
    const fe256 y = fe_to_integer<F>(want);
    return memcmp(&got, &y, sizeof y) == 0;
}

// one proof's host memory; the points are never read by the preparation, only their pointers are looked at
struct Proof {
    std::vector<reef_fe> rs, pts[2];
    reef_fe c, a_hat, blind, weights[2];
    const reef_fe *ptrs[2];
    size_t vars[2];
    reef_jacobian comm = {}, lr[32] = {};
    reef_affine q = {}, h = {};
    reef_ipa_proof view(size_t npoints, bool blinded) {
        ptrs[0] = pts[0].data();
        ptrs[1] = pts[1].data();
        return reef_ipa_proof{&comm, &c, &q, lr, lr, rs.data(), &a_hat, ptrs, vars, weights, npoints, blinded ? &h : nullptr, blinded ? &blind : nullptr};
    }
};
static Proof make(uint32_t k, size_t v0, size_t v1) {
    Proof p;
    for (uint32_t i = 0; i < k; ++i) {
        p.rs.push_back(rand_fe());
        p.rs.back().l[0] |= 1;                                   // never zero
    }
    p.vars[0] = v0;
    p.vars[1] = v1;
    for (int t = 0; t < 2; ++t) {
        for (size_t j = 0; j < p.vars[t]; ++j) p.pts[t].push_back(rand_fe());
        p.pts[t].push_back(rand_fe());                           // never an empty vector: data() stays non-null for v = 0
        p.weights[t] = rand_fe();
    }
    p.c = rand_fe();
    p.a_hat = rand_fe();
    p.blind = rand_fe();
    return p;
}

template <int F> static void check_one(uint32_t k, size_t npoints, size_t v0, size_t v1, bool blinded) {
    const size_t n = (size_t)1 << k;
    Proof p = make(k, v0, v1);
    const reef_ipa_proof pr = p.view(npoints, blinded);
    const reef_fe rho = rand_fe();
    std::vector<fe> r, rinv;
    EXPECT(ic_batch_challenges<F>(&pr, 1, k, false, r, rinv) == REEF_OK, "challenges: %s", g_error);
    for (uint32_t i = 0; i < k; ++i) EXPECT(same<F>(fe_mul<F>(r[i], rinv[i]), fe_one<F>()), "r r^-1 != 1 at k = %u, round %u", k, i);
    IcBatchProof<F> out;
    EXPECT(ic_batch_prepare<F>(pr, 0, n, k, r.data(), rinv.data(), &rho, false, out) == REEF_OK, "prepare: %s", g_error);
    // <s, pad(eq(p))> entry by entry: s_j over the bits of j (round 0 on the most significant), eq(p)_j over the low v bits
    fe want = fe_zero();
    for (size_t t = 0; t < npoints; ++t) {
        const size_t v = p.vars[t];
        fe sum = fe_zero();
        for (size_t j = 0; j < ((size_t)1 << v); ++j) {
            fe term = fe_one<F>();
            for (uint32_t i = 0; i < k; ++i) term = fe_mul<F>(term, ((j >> (k - 1 - i)) & 1) ? r[i] : rinv[i]);
            for (size_t b = 0; b < v; ++b) {
                const fe x = in<F>(p.pts[t][b]);
                term = fe_mul<F>(term, ((j >> (v - 1 - b)) & 1) ? x : fe_canon<F>(fe_sub<F, 2>(fe_one<F>(), x)));
            }
            sum = fe_canon<F>(fe_add<F>(sum, term));
        }
        want = fe_canon<F>(fe_add<F>(want, fe_mul<F>(in<F>(p.weights[t]), sum)));
    }
    EXPECT(same<F>(out.b_hat, want), "b_hat: field %d k %u points %zu vars %zu %zu", F, k, npoints, v0, v1);
    // the scalars: rho (c - a_hat b_hat) on q, rho r^2 on L, rho r^-2 on R, rho on comm, -rho blind on h; w = rho a_hat
    const fe rh = in<F>(rho), a = in<F>(p.a_hat), c = in<F>(p.c);
    EXPECT(out.sc.size() == 2 * (size_t)k + 2 + (blinded ? 1 : 0) && out.fac.size() == 2 * (size_t)k, "sizes");
    EXPECT(same_int<F>(out.sc[0], fe_mul<F>(rh, fe_canon<F>(fe_sub<F, 2>(c, fe_mul<F>(a, want))))), "the scalar of q");
    for (uint32_t i = 0; i < k; ++i) {
        EXPECT(same_int<F>(out.sc[1 + i], fe_mul<F>(rh, fe_mul<F>(r[i], r[i]))), "the scalar of L[%u]", i);
        EXPECT(same_int<F>(out.sc[1 + k + i], fe_mul<F>(rh, fe_mul<F>(rinv[i], rinv[i]))), "the scalar of R[%u]", i);
    }
    EXPECT(same_int<F>(out.sc[1 + 2 * k], rh), "the scalar of comm");
    if (blinded) EXPECT(same<F>(fe_add<F>(fe_from_integer<F>(out.sc[2 + 2 * k]), fe_mul<F>(rh, in<F>(p.blind))), fe_zero()), "the scalar of h");
    EXPECT(same<F>(out.w, fe_mul<F>(rh, a)), "w");
}

template <int F> static void check_refusals() {
    const uint32_t k = 4;
    const size_t n = 16;
    Proof good[3] = {make(k, 4, 2), make(k, 3, 4), make(k, 0, 1)};
    reef_ipa_proof prs[3] = {good[0].view(1, false), good[1].view(2, true), good[2].view(2, false)};
    reef_fe rho = rand_fe();
    std::vector<fe> r, rinv;
    IcBatchProof<F> out;
    auto refused = [&](const char *what, const char *needle) {
        reef_status st = ic_batch_challenges<F>(prs, 3, k, false, r, rinv);
        for (size_t i = 0; st == REEF_OK && i < 3; ++i) st = ic_batch_prepare<F>(prs[i], i, n, k, r.data() + i * k, rinv.data() + i * k, &rho, false, out);
        EXPECT(st == REEF_ERR_ARG && strstr(g_error, needle), "%s: status %d, message '%s'", what, (int)st, g_error);
        prs[0] = good[0].view(1, false);
        prs[1] = good[1].view(2, true);
        prs[2] = good[2].view(2, false);
        rho = rand_fe();
    };
    prs[1].rs = nullptr;           refused("a null field", "proof 1");
    prs[2].blind = &good[2].blind; refused("blind without h", "proof 2");
    prs[1].blind = nullptr;        refused("h without blind", "proof 1");
    prs[0].npoints = 0;            refused("npoints 0", "proof 0");
    prs[2].npoints = 3;            refused("npoints 3", "proof 2");
    good[1].vars[0] = k + 1;       refused("vars > k", "proof 1");
    good[1].vars[0] = 3;
    memset(&good[2].rs[1], 0, sizeof(reef_fe));  refused("a zero challenge", "proof 2");
    good[2].rs[1] = rand_fe();
    good[2].rs[1].l[0] |= 1;
    memset(&good[0].c, 0xff, sizeof(reef_fe));   refused("c = 2^256 - 1", "proof 0");
    good[0].c = rand_fe();
    memset(&rho, 0, sizeof rho);                 refused("rho = 0", "rho");
    memset(&rho, 0xff, sizeof rho);              refused("rho = 2^256 - 1", "rho");
    for (int i = 0; i < 4; ++i) rho.l[i] = 0;
    for (int i = 0; i < 9; ++i) {                // rho = the modulus itself
        const int bit = 29 * i;
        rho.l[bit / 64] |= (uint64_t)FC<F>::MOD[i] << (bit % 64);
        if (bit % 64 > 35 && bit / 64 + 1 < 4) rho.l[bit / 64 + 1] |= (uint64_t)FC<F>::MOD[i] >> (64 - bit % 64);
    }
    refused("rho = the modulus", "rho");
    reef_status st = ic_batch_challenges<F>(prs, 3, k, false, r, rinv);
    for (size_t i = 0; st == REEF_OK && i < 3; ++i) st = ic_batch_prepare<F>(prs[i], i, n, k, r.data() + i * k, rinv.data() + i * k, &rho, false, out);
    EXPECT(st == REEF_OK, "the honest batch after the refusals: %s", g_error);
    // the limits
    uint32_t kk = 0;
    EXPECT(ic_batch_shape(16, 4096, &kk) == REEF_OK && kk == 4, "m = 4096 at n = 16 is within the limits");
    EXPECT(ic_batch_shape(2, 4097, &kk) == REEF_ERR_ARG && strstr(g_error, "4097") && strstr(g_error, "4096"), "m = 4097: '%s'", g_error);
    EXPECT(ic_batch_shape(128, 4096, &kk) == REEF_ERR_ARG && strstr(g_error, "69632") && strstr(g_error, "65536"), "4096 * 17 points: '%s'", g_error);
    EXPECT(ic_batch_shape(128, 3855, &kk) == REEF_OK && ic_batch_shape(128, 3856, &kk) == REEF_ERR_ARG, "the point limit is exact");
    EXPECT(ic_batch_shape(3, 1, &kk) == REEF_ERR_ARG && ic_batch_shape(1, 1, &kk) == REEF_ERR_ARG && ic_batch_shape(0, 1, &kk) == REEF_ERR_ARG, "n");
}

template <int F> static void run() {
    for (uint32_t k : {1u, 2u, 9u}) {
        const size_t vs[4] = {0, k / 2, k - 1, k};
        for (size_t a : vs) {
            check_one<F>(k, 1, a, 0, a % 2 == 0);
            for (size_t b : vs) check_one<F>(k, 2, a, b, (a + b) % 2 == 1);
        }
    }
    check_refusals<F>();
}

int main() {
    run<0>();
    run<1>();
    if (g_failed) {
        printf("ipa_batch_selftest: %d FAILED\n", g_failed);
        return 1;
    }
    printf("ipa_batch_selftest ok: shared inversion, closed-form b_hat, one-off scalars, refusals and limits on both fields\n");
    return 0;
}
