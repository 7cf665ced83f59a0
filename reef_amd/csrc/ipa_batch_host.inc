// The host preparation of reef_ipa_check_batch (include/reef_msm.h 3m; ipa_check_engine.inc includes this): the limits, what is wrong
// with a proof, its closed-form b_hat, its table inputs and the scalars of its one-off points.  Pure field arithmetic through the
// conversion layer (fe_scalars_host.inc): no device, no state, so host/ipa_batch_selftest.cpp compiles and runs it alone.
namespace reef {

static constexpr size_t IC_BATCH_MAX = 4096, IC_BATCH_MAX_POINTS = (size_t)1 << 16;

template <int F> struct IcBatchProof {
    fe b_hat;                      // <s, b>, internal form
    fe w;                          // rho a_hat: the factor folded into the proof's hi table
    std::vector<fe256> fac;        // 2 k: r_t^-1, r_t (table form)
    std::vector<fe256> sc;         // canonical integers, in the order of the proof's points: q, L (k), R (k), comm, then h if blinded
};
// <s, pad(eq(p))> = prod_{i < k - v} r_i^-1 prod_{t < v} ((1 - p_t) r_{k-v+t}^-1 + p_t r_{k-v+t}): s_j is a product over the bits of
// j and so is eq(p)_j, the padding fixes the top k - v bits at zero, and the sum over the rest factors bit by bit
template <int F> static fe ic_eq_dot(const fe *r, const fe *rinv, u32 k, const fe *p, u32 v) {
    fe acc = fe_one<F>();
    for (u32 i = 0; i < k - v; ++i) acc = fe_mul<F>(acc, rinv[i]);
    for (u32 t = 0; t < v; ++t) {
        const u32 i = k - v + t;
        const fe term = fe_add<F>(fe_mul<F>(fe_sub<F, 2>(fe_one<F>(), p[t]), rinv[i]), fe_mul<F>(p[t], r[i]));
        acc = fe_mul<F>(acc, term);
    }
    return acc;
}
// Every proof's fields and round challenges, then ALL the m k inverses from one inversion (Montgomery's trick: prefix products, one
// fe_inv, the way back): an inversion is ~380 field products, and k of them per proof would be the whole cost of a batch.
// r, rinv: m k entries, proof i's at i k.
template <int F>
static reef_status ic_batch_challenges(const reef_ipa_proof *proofs, size_t m, u32 k, bool is_mont, std::vector<fe> &r, std::vector<fe> &rinv) {
    const size_t total = m * (size_t)k;
    r.resize(total);
    rinv.resize(total);
    for (size_t i = 0; i < m; ++i) {
        const reef_ipa_proof &pr = proofs[i];
        char name[64];
        snprintf(name, sizeof name, "reef_ipa_check_batch: proof %zu", i);
        if (!pr.comm || !pr.c || !pr.q || !pr.L || !pr.R || !pr.rs || !pr.a_hat || !pr.points || !pr.vars || !pr.weights) {
            set_error("%s: null field", name);
            return REEF_ERR_ARG;
        }
        if ((pr.h == nullptr) != (pr.blind == nullptr)) { set_error("%s: h and blind come together or not at all", name); return REEF_ERR_ARG; }
        if (pr.npoints < 1 || pr.npoints > 2) { set_error("%s: npoints = %zu, one or two points", name, pr.npoints); return REEF_ERR_ARG; }
        for (u32 t = 0; t < k; ++t) REEF_TRY(fe_challenge<F>(pr.rs + t, is_mont, name, r[i * k + t], true));
    }
    std::vector<fe> before(total);                             // before[j] = r_0 ... r_{j-1}
    fe acc = fe_one<F>();
    for (size_t j = 0; j < total; ++j) {
        before[j] = acc;
        acc = fe_mul<F>(acc, r[j]);
    }
    fe inv = fe_inv<F>(acc);                                   // no r is zero, so neither is the product
    for (size_t j = total; j-- > 0;) {
        rinv[j] = fe_mul<F>(inv, before[j]);
        inv = fe_mul<F>(inv, r[j]);
    }
    return REEF_OK;
}
// One proof of a checked batch (ic_batch_challenges has seen it): r, rinv are its k challenges and their inverses.
template <int F>
static reef_status ic_batch_prepare(const reef_ipa_proof &pr, size_t idx, size_t n, u32 k, const fe *r, const fe *rinv, const reef_fe *rho, bool is_mont,
                                    IcBatchProof<F> &out) {
    char name[64];
    snprintf(name, sizeof name, "reef_ipa_check_batch: proof %zu", idx);
    if (!fe_valid(rho, F)) { set_error("%s: rho is not below the modulus", name); return REEF_ERR_ARG; }
    const fe rh = fe_import<F>(rho, is_mont);
    if (fe_is_literal_zero(rh)) { set_error("%s: rho is zero (the proof would not be checked)", name); return REEF_ERR_ARG; }
    fe ci, ai, bl = fe_zero();
    REEF_TRY(fe_import_all<F>(pr.c, 1, is_mont, name, "c", &ci));
    REEF_TRY(fe_import_all<F>(pr.a_hat, 1, is_mont, name, "a_hat", &ai));
    if (pr.blind) REEF_TRY(fe_import_all<F>(pr.blind, 1, is_mont, name, "blind", &bl));
    fe bh = fe_zero();
    for (size_t t = 0; t < pr.npoints; ++t) {
        const size_t v = pr.vars[t];
        if (v > k) { set_error("%s: eq(points[%zu]) has 2^%zu entries, more than n = %zu", name, t, v, n); return REEF_ERR_ARG; }
        if (v && !pr.points[t]) { set_error("%s: null field", name); return REEF_ERR_ARG; }
        std::vector<fe> p(v);
        fe wt;
        REEF_TRY(fe_import_all<F>(pr.points[t], v, is_mont, name, "point", p.data()));
        REEF_TRY(fe_import_all<F>(pr.weights + t, 1, is_mont, name, "weights", &wt));
        bh = fe_canon<F>(fe_add<F>(bh, fe_mul<F>(wt, ic_eq_dot<F>(r, rinv, k, p.data(), (u32)v))));
    }
    out.b_hat = bh;
    out.w = fe_mul<F>(rh, ai);
    out.fac.resize(2 * (size_t)k);
    out.sc.resize(2 * (size_t)k + 2 + (pr.h ? 1 : 0));
    out.sc[0] = fe_to_integer<F>(fe_mul<F>(rh, fe_sub<F, 2>(ci, fe_mul<F>(ai, bh))));
    for (u32 i = 0; i < k; ++i) {
        out.sc[1 + i] = fe_to_integer<F>(fe_mul<F>(rh, fe_sqr<F>(r[i])));
        out.sc[1 + k + i] = fe_to_integer<F>(fe_mul<F>(rh, fe_sqr<F>(rinv[i])));
        out.fac[2 * i] = fe_to_table<F>(rinv[i]);
        out.fac[2 * i + 1] = fe_to_table<F>(r[i]);
    }
    out.sc[1 + 2 * k] = fe_to_integer<F>(rh);
    if (pr.h) out.sc[2 + 2 * k] = fe_to_integer<F>(fe_neg<F, 2>(fe_mul<F>(rh, bl)));
    return REEF_OK;
}
// n, m and the limits, before any proof is looked at; *k_out = log2(n)
static reef_status ic_batch_shape(size_t n, size_t m, u32 *k_out) {
    const char *name = "reef_ipa_check_batch";
    if (n < 2 || (n & (n - 1)) || n > ((size_t)1 << 27)) { set_error("%s: n = %zu is not a power of two >= 2 (at most 2^27)", name, n); return REEF_ERR_ARG; }
    u32 k = 0;
    while (((size_t)1 << k) < n) ++k;
    if (m > IC_BATCH_MAX || m * (2 * (size_t)k + 3) > IC_BATCH_MAX_POINTS) {
        set_error("%s: m = %zu proofs with %zu one-off points; the limits are %zu proofs and %zu points", name, m, m * (2 * (size_t)k + 3), IC_BATCH_MAX,
                  IC_BATCH_MAX_POINTS);
        return REEF_ERR_ARG;
    }
    *k_out = k;
    return REEF_OK;
}

}  // namespace reef
