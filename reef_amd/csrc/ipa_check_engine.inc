// Host side of the IPA check (ipa_check_kernels.inc; include/reef_msm.h 3j); included after ipa_engine.inc (sp_grid).  Two stateless
// calls on a key ctx that holds gens_v: no handle of their own, no call order.  Everything is enqueued -- the s vector, b_hat and
// the G_hat MSM on the key ctx's stream, the one-off points beside them on a second pool stream -- and the call waits once.
// reef_ipa_check_batch (3m) checks m proofs against the one key in a single pass; its host preparation is ipa_batch_host.inc.
#include "ipa_batch_host.inc"
namespace reef {

// where b comes from: the caller's vector (reef_ipa_check) or eq tables built on the device (reef_ipa_check_eq)
struct IcB {
    const reef_fe *b = nullptr;
    size_t b_len = 0;
    int b_loc = REEF_HOST;
    bool eq = false;
    const reef_fe *const *points = nullptr;
    const size_t *vars = nullptr;
    const reef_fe *weights = nullptr;
    size_t npoints = 0;
};

// an affine ABI point as an ABI Jacobian one (Z = 1, the identity (0, 0) as (0, 0, 0))
template <int C> static jacobian256 ic_lift(const reef_affine *p) {
    jacobian256 j;
    memset(&j, 0, sizeof j);
    static const reef_affine inf = {};
    if (memcmp(p, &inf, sizeof inf) == 0) return j;
    memcpy(&j, p, sizeof(reef_affine));
    j.z = fe_to_abi<C>(fe_one<C>());
    return j;
}

// The plain key the one-off points are summed over: made once per key ctx (64 slots: 2 log2(n) + 4 points at most), then
// re-keyed from a device buffer by every call -- for a plain key that is k_import_key into its one table, no host wait.
// c = 8: 32 bucket groups, which the host-side window combine of msm_device_scalars takes (host_combine_fits).
static constexpr size_t IC_SIDE_POINTS = 64;
template <int C> static reef_status ic_side_key(Ctx<C> *key) {
    if (key->side) return REEF_OK;
    reef_msm_opts o;
    memset(&o, 0, sizeof o);
    o.window_bits = 8;
    o.byte_tables = 2;
    o.device = key->key->device;
    std::vector<reef_affine> none(IC_SIDE_POINTS);
    memset(none.data(), 0, none.size() * sizeof(reef_affine));
    void *impl = nullptr;
    REEF_TRY(v_ctx_create<C>(&impl, none.data(), IC_SIDE_POINTS, REEF_HOST, &o));
    key->side = (Ctx<C> *)impl;
    return REEF_OK;
}

template <int C>
static reef_status ipa_check_run(void *key_impl, size_t n, const reef_jacobian *comm, const reef_fe *c, const reef_affine *q, const reef_jacobian *L,
                                 const reef_jacobian *R, const reef_fe *rs, const reef_fe *a_hat, const IcB &bs, const reef_affine *h,
                                 const reef_fe *blind, bool is_mont, uint32_t *accept, reef_jacobian *p_hat, reef_jacobian *g_hat, reef_fe *b_hat,
                                 const char *name) {
    constexpr int F = 1 - C;
    Ctx<C> *key = (Ctx<C> *)key_impl;
    if (!key || !comm || !c || !q || !L || !R || !rs || !a_hat || !accept) { set_error("null argument"); return REEF_ERR_ARG; }
    if (n < 2 || (n & (n - 1)) || n > ((size_t)1 << 27)) { set_error("%s: n = %zu is not a power of two >= 2 (at most 2^27)", name, n); return REEF_ERR_ARG; }
    if ((h == nullptr) != (blind == nullptr)) { set_error("%s: h and blind come together or not at all", name); return REEF_ERR_ARG; }
    u32 k = 0;
    while (((size_t)1 << k) < n) ++k;
    // ---- every scalar through the conversion layer, before anything is touched
    std::vector<fe> r(k), rinv(k);
    for (u32 i = 0; i < k; ++i) {
        REEF_TRY(fe_challenge<F>(rs + i, is_mont, name, r[i], true));
        rinv[i] = fe_inv<F>(r[i]);
    }
    fe ci, ai, bl = fe_zero();
    REEF_TRY(fe_import_all<F>(c, 1, is_mont, name, "c", &ci));
    REEF_TRY(fe_import_all<F>(a_hat, 1, is_mont, name, "a_hat", &ai));
    if (blind) REEF_TRY(fe_import_all<F>(blind, 1, is_mont, name, "blind", &bl));
    size_t nb = 0;                                              // entries of b on the device
    IcEq eq;
    memset(&eq, 0, sizeof eq);
    std::vector<fe256> eqf;                                     // the eq factors of both points
    if (bs.eq) {
        if (bs.npoints < 1 || bs.npoints > 2 || !bs.points || !bs.vars || !bs.weights) { set_error("%s: one or two points, with vars and weights", name); return REEF_ERR_ARG; }
        eq.npoints = (u32)bs.npoints;
        for (size_t t = 0; t < bs.npoints; ++t) {
            const size_t v = bs.vars[t];
            if (v > k) { set_error("%s: eq(points[%zu]) has 2^%zu entries, more than n = %zu", name, t, v, n); return REEF_ERR_ARG; }
            if (v && !bs.points[t]) { set_error("null argument"); return REEF_ERR_ARG; }
            std::vector<fe> p(v);
            fe w;
            REEF_TRY(fe_import_all<F>(bs.points[t], v, is_mont, name, "point", p.data()));
            REEF_TRY(fe_import_all<F>(bs.weights + t, 1, is_mont, name, "weights", &w));
            eq.vars[t] = (u32)v;
            eq.off[t] = (u32)eqf.size();
            eq.w[t] = fe_to_table<F>(w);
            for (size_t j = 0; j < v; ++j) {
                eqf.push_back(fe_to_table<F>(fe_sub<F, 2>(fe_one<F>(), p[j])));
                eqf.push_back(fe_to_table<F>(p[j]));
            }
            nb = std::max(nb, (size_t)1 << v);
        }
    } else {
        if (bs.b_len > n) { set_error("%s: b_len = %zu exceeds n = %zu", name, bs.b_len, n); return REEF_ERR_ARG; }
        if (bs.b_len && !bs.b) { set_error("null argument"); return REEF_ERR_ARG; }
        if (bs.b_loc == REEF_DEVICE && ((uintptr_t)bs.b & 15)) { set_error("%s: a device b must be 16-byte aligned", name); return REEF_ERR_ARG; }
        if (bs.b_loc != REEF_DEVICE)
            for (size_t j = 0; j < bs.b_len; ++j)
                if (!fe_valid(bs.b + j, F)) { set_error("%s: b[%zu] is not below the modulus", name, j); return REEF_ERR_ARG; }
        nb = bs.b_len;
    }
    // ---- the one-off points and their scalars: P_hat's terms first (c q, r_i^2 L_i, r_i^-2 R_i), then the right-hand side's
    // ((a_hat b_hat) q, whose scalar is formed on the device, and blind h)
    const u32 np = 1 + 2 * k, ab_idx = np, nt = np + 1 + (h ? 1u : 0u);
    const u32 hb = k / 2, m = k - hb, ntab = (1u << hb) + (1u << m);
    std::vector<jacobian256> pts(nt + 1);                       // the last one: comm
    std::vector<fe256> sc(nt), fac(2 * k);
    pts[0] = ic_lift<C>(q);
    sc[0] = fe_to_integer<F>(ci);
    for (u32 i = 0; i < k; ++i) {
        memcpy(&pts[1 + i], L + i, sizeof(jacobian256));
        memcpy(&pts[1 + k + i], R + i, sizeof(jacobian256));
        sc[1 + i] = fe_to_integer<F>(fe_sqr<F>(r[i]));
        sc[1 + k + i] = fe_to_integer<F>(fe_sqr<F>(rinv[i]));
        fac[2 * i] = fe_to_table<F>(rinv[i]);
        fac[2 * i + 1] = fe_to_table<F>(r[i]);
    }
    pts[ab_idx] = pts[0];
    memset(&sc[ab_idx], 0, sizeof(fe256));
    if (h) {
        pts[ab_idx + 1] = ic_lift<C>(h);
        sc[ab_idx + 1] = fe_to_integer<F>(bl);
    }
    memcpy(&pts[nt], comm, sizeof(jacobian256));
    // the key route sums the same nt + 1 points: rowD for D = P_hat - (a_hat b_hat) q - blind h (entry 0 becomes c - a_hat b_hat on the
    // device), rowP for P_hat itself
    const u32 npts = nt + 1;
    std::vector<fe256> rows(2 * (size_t)npts);
    memset(rows.data(), 0, rows.size() * sizeof(fe256));
    fe256 *rowD = rows.data(), *rowP = rowD + npts;
    for (u32 i = 0; i < np; ++i) rowD[i] = rowP[i] = sc[i];
    if (h) rowD[ab_idx + 1] = fe_to_integer<F>(fe_neg<F, 2>(bl));
    rowD[nt] = rowP[nt] = fe_to_integer<F>(fe_one<F>());

    std::lock_guard<std::mutex> lk(key->mu);
    if (n > key->key->n) { set_error("%s: n = %zu exceeds the key length %zu", name, n, key->key->n); return REEF_ERR_ARG; }
    if (key->wsplit_world > 1) { set_error("%s: the key ctx computes a window split of every MSM (reef_msm_ctx_set_window_split)", name); return REEF_ERR_ARG; }
    REEF_ON_DEVICE(key->key->device);
    CtxScope<C> scope(key);
    REEF_TRY(scope.enter());
    hipStream_t ks = key->stream;
    ScratchStream ss;                                           // the second stream, the call's buffers; waited for when it goes
    REEF_TRY(ss.init());
    hipEvent_t *ev = nullptr;                                   // the thread's two events (ScratchStream keeps them)
    REEF_TRY(ss.events(&ev));
    // The route of the one-off points.  Ships: the re-keyed plain key (0.3-0.4 ms beside the MSM).  +experiment build,
    // REEF_IPA_CHECK_ROUTE=lanes: one lane per point (2.1-2.9 ms), kept for the A/B of tools/time_ipa_check.py.
    static const bool lanes = [] { const char *e = exp_env("REEF_IPA_CHECK_ROUTE"); return e && strcmp(e, "lanes") == 0; }();
    if (npts > IC_SIDE_POINTS) { set_error("%s: %u one-off points, the side key holds %zu", name, npts, IC_SIDE_POINTS); return REEF_ERR_ARG; }
    if (!lanes) REEF_TRY(ic_side_key<C>(key));
    // one small buffer: [uploaded: points | scalars | rows | challenge factors | eq factors] [tables] [partial] [b_hat] [terms] [affine] [D, P]
    // [g_hat] [out]
    const size_t o_pts = 0, o_sc = o_pts + (nt + 1) * sizeof(jacobian256), o_rows = o_sc + nt * sizeof(fe256),
                 o_fac = o_rows + 2 * (size_t)npts * sizeof(fe256), o_eqf = o_fac + 2 * k * sizeof(fe256),
                 up_bytes = o_eqf + eqf.size() * sizeof(fe256), o_tab = up_bytes, o_part = o_tab + ntab * sizeof(fe256),
                 o_bhat = o_part + (size_t)SP_BLOCKS * 27 * sizeof(unsigned long long), o_terms = o_bhat + sizeof(fe256),
                 o_aff = o_terms + nt * sizeof(xyzz_mem), o_dp = o_aff + npts * sizeof(affine256), o_ghat = o_dp + 2 * sizeof(jacobian256),
                 o_out = o_ghat + sizeof(jacobian256), total = o_out + sizeof(IcOut);
    void *d_s_ = nullptr, *d_b_ = nullptr, *d_w_ = nullptr;
    REEF_TRY(ss.alloc(&d_s_, n * sizeof(fe256)));
    REEF_TRY(ss.alloc(&d_b_, std::max<size_t>(nb, 1) * sizeof(fe256)));
    REEF_TRY(ss.alloc(&d_w_, total));
    char *w = (char *)d_w_;
    std::vector<char> up(up_bytes);
    memcpy(up.data() + o_pts, pts.data(), (nt + 1) * sizeof(jacobian256));
    memcpy(up.data() + o_sc, sc.data(), nt * sizeof(fe256));
    memcpy(up.data() + o_rows, rows.data(), rows.size() * sizeof(fe256));
    memcpy(up.data() + o_fac, fac.data(), 2 * k * sizeof(fe256));
    if (!eqf.empty()) memcpy(up.data() + o_eqf, eqf.data(), eqf.size() * sizeof(fe256));
    fe256 *d_s = (fe256 *)d_s_, *d_bhat = (fe256 *)(w + o_bhat);
    const fe256 *d_b = (const fe256 *)d_b_;
    unsigned long long *d_part = (unsigned long long *)(w + o_part);
    jacobian256 *d_pts = (jacobian256 *)(w + o_pts), *d_ghat = (jacobian256 *)(w + o_ghat);
    xyzz_mem *d_terms = (xyzz_mem *)(w + o_terms);
    IcOut *d_out = (IcOut *)(w + o_out);

    // ---- the key ctx's stream: tables, b, s with the limb sums of s_j b_j, b_hat
    REEF_HIP_TRY(hipMemcpyAsync(w, up.data(), up_bytes, hipMemcpyHostToDevice, ks));
    int b_form = is_mont ? (int)SP_FORM_MONT : (int)SP_FORM_INTEGER;
    if (bs.eq) {
        hipLaunchKernelGGL(k_ic_eqb<F>, dim3(ceil_div(nb, 256)), dim3(256), 0, ks, eq, (const fe256 *)(w + o_eqf), (u32)nb, (fe256 *)d_b_);
        b_form = SP_FORM_TABLE;
    } else if (bs.b_loc == REEF_DEVICE) {
        d_b = (const fe256 *)bs.b;
    } else if (nb) {
        REEF_HIP_TRY(hipMemcpyAsync(d_b_, bs.b, nb * sizeof(fe256), hipMemcpyHostToDevice, ks));
    }
    hipLaunchKernelGGL(k_ic_tables<F>, dim3(ceil_div(ntab, 256)), dim3(256), 0, ks, (const fe256 *)(w + o_fac), hb, m, (fe256 *)(w + o_tab));
    const u32 grid = sp_grid(n);
    // Nobody asked for G_hat: the MSM runs over a_hat s and gives a_hat G_hat itself.  With g_hat asked for, a_hat G_hat is a
    // 255-step chain on one lane after the MSM (~1.9 ms, profiles/r10_ipa_check_timing.txt).
    const bool scaled = g_hat == nullptr;
    hipLaunchKernelGGL(k_ic_s<F>, dim3(grid), dim3(SP_THREADS), 0, ks, (const fe256 *)(w + o_tab), hb, m, (u32)n, d_b, (u32)nb, b_form,
                       fe_to_table<F>(ai), (int)scaled, d_s, d_part);
    hipLaunchKernelGGL(k_sp_finish<F>, dim3(1), dim3(SP_THREADS), 0, ks, (const unsigned long long *)d_part, grid, 1u, (int)SP_FORM_TABLE, d_bhat);
    REEF_HIP_TRY(hipGetLastError());
    const int out_form = is_mont ? (int)SP_FORM_MONT : (int)SP_FORM_INTEGER;
    // REEF_IPA_CHECK_ONE_STREAM=1 (+experiment build): the one-off points on the key ctx's stream ahead of the MSM, for the A/B
    static const bool one_stream = [] { const char *e = exp_env("REEF_IPA_CHECK_ONE_STREAM"); return e && e[0] == '1'; }();
    if (lanes) {
        // ---- one lane per point on the second stream, once b_hat stands; then G_hat, both sides and the comparison
        hipStream_t s2 = one_stream ? ks : ss.s;
        REEF_HIP_TRY(hipEventRecord(ev[0], ks));
        REEF_HIP_TRY(hipStreamWaitEvent(s2, ev[0], 0));
        hipLaunchKernelGGL(k_ic_terms<C>, dim3(ceil_div(nt, 64)), dim3(64), 0, s2, (const jacobian256 *)d_pts, (const fe256 *)(w + o_sc), nt, ab_idx,
                           fe_to_table<F>(ai), (const fe256 *)d_bhat, d_terms);
        REEF_HIP_TRY(hipGetLastError());
        REEF_HIP_TRY(hipEventRecord(ev[1], s2));
        REEF_TRY(msm_device_scalars<C>(key, d_s, n, false, (reef_jacobian *)d_ghat, REEF_DEVICE, d_ghat));
        REEF_HIP_TRY(hipStreamWaitEvent(ks, ev[1], 0));
        hipLaunchKernelGGL(k_ic_final<C>, dim3(1), dim3(64), 0, ks, (const jacobian256 *)(d_pts + nt), (const xyzz_mem *)d_terms, np, nt,
                           (const jacobian256 *)d_ghat, fe_to_integer<F>(ai), (int)scaled, (const fe256 *)d_bhat, out_form, d_out);
    } else {
        // ---- the side key on its own stream: the points made affine and imported as its table while the key ctx's stream builds
        // s; its MSMs once c - a_hat b_hat stands; G_hat beside them on the key ctx's stream
        Ctx<C> *side = key->side;
        fe256 *d_rowD = (fe256 *)(w + o_rows), *d_rowP = d_rowD + npts;
        affine256 *d_aff = (affine256 *)(w + o_aff);
        jacobian256 *d_D = (jacobian256 *)(w + o_dp), *d_P = d_D + 1;
        hipLaunchKernelGGL(k_ic_ab<F>, dim3(1), dim3(64), 0, ks, fe_to_table<F>(ci), fe_to_table<F>(ai), (const fe256 *)d_bhat, d_rowD);
        REEF_HIP_TRY(hipGetLastError());
        hipStream_t s2 = one_stream ? ks : (hipStream_t)v_ctx_stream<C>(side);     // the side ctx stays on one pool stream
        if (!s2) return REEF_ERR_HIP;
        REEF_HIP_TRY(hipEventRecord(ev[0], ks));
        REEF_HIP_TRY(hipStreamWaitEvent(s2, ev[0], 0));
        {
            std::lock_guard<std::mutex> sl(side->mu);
            CtxScope<C> sscope(side);
            REEF_TRY(sscope.enter());
            if (one_stream) side->stream = ks;
            hipLaunchKernelGGL(k_normalize<C>, dim3(ceil_div(ceil_div(npts, NORM_PER), 256)), dim3(256), 0, s2, (const jacobian256 *)d_pts, npts, d_aff,
                               (fe256 *)nullptr);
            hipLaunchKernelGGL(k_import_key<C>, dim3(ceil_div(npts, 256)), dim3(256), 0, s2, (const affine256 *)d_aff, npts, side->key->tables);
            REEF_HIP_TRY(hipGetLastError());
            REEF_TRY(msm_device_scalars<C>(side, d_rowD, npts, false, (reef_jacobian *)d_D, REEF_DEVICE, d_D));
            if (p_hat) REEF_TRY(msm_device_scalars<C>(side, d_rowP, npts, false, (reef_jacobian *)d_P, REEF_DEVICE, d_P));
            REEF_HIP_TRY(hipEventRecord(ev[1], s2));
        }
        REEF_TRY(msm_device_scalars<C>(key, d_s, n, false, (reef_jacobian *)d_ghat, REEF_DEVICE, d_ghat));
        REEF_HIP_TRY(hipStreamWaitEvent(ks, ev[1], 0));
        hipLaunchKernelGGL(k_ic_final_key<C>, dim3(1), dim3(64), 0, ks, (const jacobian256 *)d_D, p_hat ? (const jacobian256 *)d_P : (const jacobian256 *)nullptr,
                           (const jacobian256 *)d_ghat, fe_to_integer<F>(ai), (int)scaled, (const fe256 *)d_bhat, out_form, d_out);
    }
    REEF_HIP_TRY(hipGetLastError());
    IcOut res;
    jacobian256 gh;
    REEF_HIP_TRY(hipMemcpyAsync(&res, d_out, sizeof res, hipMemcpyDeviceToHost, ks));
    if (g_hat) REEF_HIP_TRY(hipMemcpyAsync(&gh, d_ghat, sizeof gh, hipMemcpyDeviceToHost, ks));
    REEF_HIP_TRY(hipStreamSynchronize(ks));                     // the call's one wait
    *accept = res.accept;
    if (p_hat) memcpy(p_hat, &res.p_hat, sizeof(jacobian256));
    if (g_hat) memcpy(g_hat, &gh, sizeof gh);
    if (b_hat) memcpy(b_hat, &res.b_hat, sizeof(fe256));
    return REEF_OK;
}

template <int C>
static reef_status v_ipa_check(void *key_impl, size_t n, const reef_jacobian *comm, const reef_fe *c, const reef_affine *q, const reef_jacobian *L,
                               const reef_jacobian *R, const reef_fe *rs, const reef_fe *a_hat, const reef_fe *b, size_t b_len, int b_loc,
                               const reef_affine *h, const reef_fe *blind, bool is_mont, uint32_t *accept, reef_jacobian *p_hat, reef_jacobian *g_hat,
                               reef_fe *b_hat) {
    IcB bs;
    bs.b = b;
    bs.b_len = b_len;
    bs.b_loc = b_loc;
    return ipa_check_run<C>(key_impl, n, comm, c, q, L, R, rs, a_hat, bs, h, blind, is_mont, accept, p_hat, g_hat, b_hat, "reef_ipa_check");
}
template <int C>
static reef_status v_ipa_check_eq(void *key_impl, size_t n, const reef_jacobian *comm, const reef_fe *c, const reef_affine *q, const reef_jacobian *L,
                                  const reef_jacobian *R, const reef_fe *rs, const reef_fe *a_hat, const reef_fe *const *points, const size_t *vars,
                                  const reef_fe *weights, size_t npoints, const reef_affine *h, const reef_fe *blind, bool is_mont, uint32_t *accept,
                                  reef_jacobian *p_hat, reef_jacobian *g_hat, reef_fe *b_hat) {
    IcB bs;
    bs.eq = true;
    bs.points = points;
    bs.vars = vars;
    bs.weights = weights;
    bs.npoints = npoints;
    return ipa_check_run<C>(key_impl, n, comm, c, q, L, R, rs, a_hat, bs, h, blind, is_mont, accept, p_hat, g_hat, b_hat, "reef_ipa_check_eq");
}

// ---------------------------------------------------------------- a batch of checks against one key (include/reef_msm.h 3m)
// The plain key the one-off points of a batch are summed over: the key ctx's own, sized to the largest batch seen (grow-only), freed
// with the ctx.  The 64-slot side key of the single calls is another one and stays as it is.
template <int C> static reef_status ic_side_batch_key(Ctx<C> *key, size_t npts) {
    if (key->side_batch && key->side_batch->key->n >= npts) return REEF_OK;
    if (key->side_batch) { v_ctx_destroy<C>(key->side_batch); key->side_batch = nullptr; }
    size_t cap = 256;
    while (cap < npts) cap <<= 1;
    reef_msm_opts o;
    memset(&o, 0, sizeof o);
    o.window_bits = 8;
    o.byte_tables = 2;
    o.device = key->key->device;
    std::vector<reef_affine> none(cap);
    memset(none.data(), 0, none.size() * sizeof(reef_affine));
    void *impl = nullptr;
    REEF_TRY(v_ctx_create<C>(&impl, none.data(), cap, REEF_HOST, &o));
    key->side_batch = (Ctx<C> *)impl;
    return REEF_OK;
}

// Everything up to the call's one wait.  prep: the proofs' host preparation; npts: the one-off points of all of them.
template <int C>
static reef_status ipa_check_batch_device(Ctx<C> *key, size_t n, u32 k, const reef_ipa_proof *proofs, size_t m, const std::vector<IcBatchProof<1 - C>> &prep,
                                          size_t npts, uint32_t *accept_all, reef_fe *s_comb, int s_loc, reef_jacobian *d_comb, reef_jacobian *g_comb) {
    constexpr int F = 1 - C;
    const char *name = "reef_ipa_check_batch";
    std::lock_guard<std::mutex> lk(key->mu);
    if (n > key->key->n) { set_error("%s: n = %zu exceeds the key length %zu", name, n, key->key->n); return REEF_ERR_ARG; }
    if (key->wsplit_world > 1) { set_error("%s: the key ctx computes a window split of every MSM (reef_msm_ctx_set_window_split)", name); return REEF_ERR_ARG; }
    REEF_ON_DEVICE(key->key->device);
    CtxScope<C> scope(key);
    REEF_TRY(scope.enter());
    hipStream_t ks = key->stream;
    ScratchStream ss;
    REEF_TRY(ss.init());
    hipEvent_t *ev = nullptr;
    REEF_TRY(ss.events(&ev));
    REEF_TRY(ic_side_batch_key<C>(key, npts));
    const bool timed = key->timing;
    if (timed && !key->batch_ev[0])
        for (auto &e : key->batch_ev) REEF_HIP_TRY(hipEventCreate(&e));
    const u32 hb = k / 2, lo_bits = k - hb, ntab = (1u << hb) + (1u << lo_bits);
    // one buffer: [uploaded: points | scalars | challenge factors | w] [affine] [D] [G] [accept]
    const size_t o_pts = 0, o_sc = o_pts + npts * sizeof(jacobian256), o_fac = o_sc + npts * sizeof(fe256), o_w = o_fac + m * 2 * k * sizeof(fe256),
                 up_bytes = o_w + m * sizeof(fe256), o_aff = up_bytes, o_d = o_aff + npts * sizeof(affine256), o_g = o_d + sizeof(jacobian256),
                 o_out = o_g + sizeof(jacobian256), total = o_out + 32;
    void *d_s_ = nullptr, *d_tab_ = nullptr, *d_w_ = nullptr;
    REEF_TRY(ss.alloc(&d_s_, n * sizeof(fe256)));
    REEF_TRY(ss.alloc(&d_tab_, m * (size_t)ntab * sizeof(fe256)));
    REEF_TRY(ss.alloc(&d_w_, total));
    char *w = (char *)d_w_;
    std::vector<char> up(up_bytes);
    {
        jacobian256 *pts = (jacobian256 *)(up.data() + o_pts);
        fe256 *sc = (fe256 *)(up.data() + o_sc), *fac = (fe256 *)(up.data() + o_fac), *ws = (fe256 *)(up.data() + o_w);
        size_t at = 0;
        for (size_t i = 0; i < m; ++i) {
            const reef_ipa_proof &pr = proofs[i];
            const size_t cnt = prep[i].sc.size();
            pts[at] = ic_lift<C>(pr.q);
            memcpy(&pts[at + 1], pr.L, k * sizeof(jacobian256));
            memcpy(&pts[at + 1 + k], pr.R, k * sizeof(jacobian256));
            memcpy(&pts[at + 1 + 2 * k], pr.comm, sizeof(jacobian256));
            if (pr.h) pts[at + 2 + 2 * k] = ic_lift<C>(pr.h);
            memcpy(sc + at, prep[i].sc.data(), cnt * sizeof(fe256));
            memcpy(fac + i * 2 * k, prep[i].fac.data(), 2 * (size_t)k * sizeof(fe256));
            ws[i] = fe_to_table<F>(prep[i].w);
            at += cnt;
        }
    }
    fe256 *d_s = (fe256 *)d_s_, *d_tab = (fe256 *)d_tab_;
    jacobian256 *d_pts = (jacobian256 *)(w + o_pts), *d_D = (jacobian256 *)(w + o_d), *d_G = (jacobian256 *)(w + o_g);
    affine256 *d_aff = (affine256 *)(w + o_aff);
    u32 *d_acc = (u32 *)(w + o_out);

    // ---- the key ctx's stream: the upload, the m pairs of tables, S, the MSM over the key
    REEF_HIP_TRY(hipMemcpyAsync(w, up.data(), up_bytes, hipMemcpyHostToDevice, ks));
    REEF_HIP_TRY(hipEventRecord(ev[0], ks));
    if (timed) REEF_HIP_TRY(hipEventRecord(key->batch_ev[0], ks));
    hipLaunchKernelGGL(k_ic_tables_batch<F>, dim3((u32)ceil_div(m * (size_t)ntab, 256)), dim3(256), 0, ks, (const fe256 *)(w + o_fac), (const fe256 *)(w + o_w), hb,
                       lo_bits, (u32)m, d_tab);
    const u32 grid = (u32)ceil_div(n, SP_THREADS);
    if (lo_bits >= 6)
        hipLaunchKernelGGL((k_ic_s_batch<F, true>), dim3(grid), dim3(SP_THREADS), 0, ks, (const fe256 *)d_tab, hb, lo_bits, (u32)n, (u32)m, d_s);
    else
        hipLaunchKernelGGL((k_ic_s_batch<F, false>), dim3(grid), dim3(SP_THREADS), 0, ks, (const fe256 *)d_tab, hb, lo_bits, (u32)n, (u32)m, d_s);
    REEF_HIP_TRY(hipGetLastError());
    if (timed) REEF_HIP_TRY(hipEventRecord(key->batch_ev[1], ks));
    // ---- the second stream, beside them: the one-off points made affine, imported as the batch side key's table, one MSM
    {
        Ctx<C> *side = key->side_batch;
        hipStream_t s2 = (hipStream_t)v_ctx_stream<C>(side);
        if (!s2) return REEF_ERR_HIP;
        REEF_HIP_TRY(hipStreamWaitEvent(s2, ev[0], 0));
        std::lock_guard<std::mutex> sl(side->mu);
        CtxScope<C> sscope(side);
        REEF_TRY(sscope.enter());
        if (timed) REEF_HIP_TRY(hipEventRecord(key->batch_ev[2], s2));
        hipLaunchKernelGGL(k_normalize<C>, dim3(ceil_div(ceil_div(npts, NORM_PER), 256)), dim3(256), 0, s2, (const jacobian256 *)d_pts, (u32)npts, d_aff,
                           (fe256 *)nullptr);
        hipLaunchKernelGGL(k_import_key<C>, dim3(ceil_div(npts, 256)), dim3(256), 0, s2, (const affine256 *)d_aff, (u32)npts, side->key->tables);
        REEF_HIP_TRY(hipGetLastError());
        REEF_TRY(msm_device_scalars<C>(side, (const fe256 *)(w + o_sc), npts, false, (reef_jacobian *)d_D, REEF_DEVICE, d_D));
        if (timed) REEF_HIP_TRY(hipEventRecord(key->batch_ev[3], s2));
        REEF_HIP_TRY(hipEventRecord(ev[1], s2));
    }
    REEF_TRY(msm_device_scalars<C>(key, d_s, n, false, (reef_jacobian *)d_G, REEF_DEVICE, d_G));
    REEF_HIP_TRY(hipStreamWaitEvent(ks, ev[1], 0));
    hipLaunchKernelGGL(k_ic_final_batch<C>, dim3(1), dim3(64), 0, ks, (const jacobian256 *)d_D, (const jacobian256 *)d_G, d_acc);
    REEF_HIP_TRY(hipGetLastError());
    struct { u32 accept, pad[7]; } res;
    jacobian256 dg[2];
    REEF_HIP_TRY(hipMemcpyAsync(&res, d_acc, sizeof res, hipMemcpyDeviceToHost, ks));
    if (d_comb || g_comb) REEF_HIP_TRY(hipMemcpyAsync(dg, d_D, sizeof dg, hipMemcpyDeviceToHost, ks));
    if (s_comb) REEF_HIP_TRY(hipMemcpyAsync(s_comb, d_s, n * sizeof(fe256), s_loc == REEF_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ks));
    REEF_HIP_TRY(hipStreamSynchronize(ks));                     // the call's one wait
    key->batch_timed = timed;
    *accept_all = res.accept;
    if (d_comb) memcpy(d_comb, &dg[0], sizeof(jacobian256));
    if (g_comb) memcpy(g_comb, &dg[1], sizeof(jacobian256));
    return REEF_OK;
}

template <int C>
static reef_status v_ipa_check_batch(void *key_impl, size_t n, const reef_ipa_proof *proofs, size_t m, const reef_fe *rho, bool is_mont, uint32_t *accept_all,
                                     uint32_t *accept_each, reef_fe *b_hats, reef_fe *s_comb, int s_loc, reef_jacobian *d_comb, reef_jacobian *g_comb) {
    constexpr int F = 1 - C;
    const char *name = "reef_ipa_check_batch";
    Ctx<C> *key = (Ctx<C> *)key_impl;
    if (!key || !accept_all || (m && (!proofs || !rho))) { set_error("null argument"); return REEF_ERR_ARG; }
    if (m == 0) { *accept_all = 1; return REEF_OK; }
    u32 k = 0;
    REEF_TRY(ic_batch_shape(n, m, &k));
    if (s_comb && s_loc != REEF_HOST && s_loc != REEF_DEVICE) { set_error("%s: unknown location %d of s_comb", name, s_loc); return REEF_ERR_ARG; }
    if (s_comb && s_loc == REEF_DEVICE && ((uintptr_t)s_comb & 15)) { set_error("%s: a device s_comb must be 16-byte aligned", name); return REEF_ERR_ARG; }
    // ---- every scalar of every proof through the conversion layer, before anything is touched
    std::vector<IcBatchProof<F>> prep(m);
    size_t npts = 0;
    std::vector<fe> r, rinv;
    REEF_TRY(ic_batch_challenges<F>(proofs, m, k, is_mont, r, rinv));
    for (size_t i = 0; i < m; ++i) {
        REEF_TRY(ic_batch_prepare<F>(proofs[i], i, n, k, r.data() + i * k, rinv.data() + i * k, rho + i, is_mont, prep[i]));
        npts += prep[i].sc.size();
    }
    uint32_t all = 0;
    REEF_TRY(ipa_check_batch_device<C>(key, n, k, proofs, m, prep, npts, &all, s_comb, s_loc, d_comb, g_comb));
    *accept_all = all;
    if (b_hats)
        for (size_t i = 0; i < m; ++i) {
            const fe256 o = fe_to_caller<F>(prep[i].b_hat, is_mont);
            memcpy(b_hats + i, &o, sizeof o);
        }
    if (!accept_each) return REEF_OK;
    if (all) {
        for (size_t i = 0; i < m; ++i) accept_each[i] = 1;
        return REEF_OK;
    }
    // ---- the batch does not verify and the caller wants to know who: the single check on each proof, m MSMs over the key
    for (size_t i = 0; i < m; ++i) {
        const reef_ipa_proof &pr = proofs[i];
        IcB bs;
        bs.eq = true;
        bs.points = pr.points;
        bs.vars = pr.vars;
        bs.weights = pr.weights;
        bs.npoints = pr.npoints;
        REEF_TRY(ipa_check_run<C>(key_impl, n, pr.comm, pr.c, pr.q, pr.L, pr.R, pr.rs, pr.a_hat, bs, pr.h, pr.blind, is_mont, accept_each + i, nullptr, nullptr,
                                  nullptr, name));
    }
    return REEF_OK;
}

// How the last batch on this key ctx divided, with the key's timing switched on (reef_msm_ctx_enable_timing) when it ran: the
// tables and the S pass, the MSM over the key, the one-off points (normalise, import, MSM) on the second stream.
template <int C> static reef_status v_ipa_check_batch_timing(void *key_impl, float *s_pass_ms, float *key_msm_ms, float *side_ms) {
    Ctx<C> *key = (Ctx<C> *)key_impl;
    if (!key) { set_error("null argument"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(key->mu);
    if (!key->batch_timed || key->ev_last < 0) { set_error("no timed batch yet (reef_msm_ctx_enable_timing, then reef_ipa_check_batch)"); return REEF_ERR_ARG; }
    REEF_ON_DEVICE(key->key->device);
    if (s_pass_ms) REEF_HIP_TRY(hipEventElapsedTime(s_pass_ms, key->batch_ev[0], key->batch_ev[1]));
    if (side_ms) REEF_HIP_TRY(hipEventElapsedTime(side_ms, key->batch_ev[2], key->batch_ev[3]));
    if (key_msm_ms) {
        hipEvent_t *q = key->evr[key->ev_last];
        REEF_HIP_TRY(hipEventSynchronize(q[3]));
        REEF_HIP_TRY(hipEventElapsedTime(key_msm_ms, q[0], q[3]));
    }
    return REEF_OK;
}

template <int C> IpaCheckVTable make_ipa_check_vtable() {
    return IpaCheckVTable{v_ipa_check<C>, v_ipa_check_eq<C>, v_ipa_check_batch<C>, v_ipa_check_batch_timing<C>};
}

}  // namespace reef
