// Host side of the Hyrax consistency arguments of many proofs in lock-step (hyrax_batch_kernels.inc; include/reef_msm.h 3p); included
// after hyrax_engine.inc.  A batch borrows the resident document of a 3i ctx -- z, the row blinds, the factoring, the device, the lock
// and the event -- and keeps everything an argument writes in buffers of its own, so an argument in flight on the ctx itself goes on
// untouched.  Every call is one DeviceCall on the doc ctx (calls on a batch and on its doc serialise) and has one host wait for the
// whole batch: create -> eval_begin -> ipa_begin -> ipa_round x (right - 1) -> finish (proof_order.h: hyb_check).
namespace reef {

template <int C> struct HyraxBatch {
    static constexpr int F = 1 - C;
    HyraxCtx<C> *doc = nullptr;          // borrowed: outlives the batch
    int device = 0;                      // doc's, kept here so that the end of a batch reads nothing of doc
    size_t m_max = 0, m = 0;
    DevBuf a, b;                         // m_max rows of 2^right entries: a (canonical integers), b (internal form)
    DevBuf pts, eqs, part, dot, res;     // the points as uploaded; the eq tables of a group of points and the limbs of 1; bound-row partial
                                         // sums; 20 limb sums per proof; eval, lz_blind per proof
    DevBuf partial, out, chal, coef;     // block sums per proof; c_L, c_R per proof; r, r^-1 per round and proof; 2^k coefficients per proof
    DevBuf scal, jac, hbl;               // the 2 m x n scalars of L and R; the 2 m results; the h term's 2 m blinds
    DevBuf qraw, qtab, stage;            // q_0 .. q_{m-1}, h as uploaded and in key-table form; their nibble tables; read staging
    Ctx<C> *key = nullptr;               // the gens_v key ctx, from eval_begin to finish
    bool with_h = false;
    size_t npts = 0;                     // the points the nibble tables hold: m, and h when the term is on
    int phase = HY_NONE;
    u32 rounds = 0;                      // challenges taken
    size_t len = 0;                      // the length of every proof's a and b as they stand
    std::vector<fe256> hb, ch;           // host copies of what a call uploads
    std::vector<jacobian256> lr;
};

template <int C> static void hyrax_batch_free(HyraxBatch<C> *b) {
    if (!b) return;
    DeviceGuard dg(b->device);      // every call waited for its work before it returned
    for (DevBuf *d : {&b->a, &b->b, &b->pts, &b->eqs, &b->part, &b->dot, &b->res, &b->partial, &b->out, &b->chal, &b->coef, &b->scal, &b->jac, &b->hbl,
                      &b->qraw, &b->qtab, &b->stage})
        d->release();
    delete b;
}
template <int C> static reef_status hyb_expect(HyraxBatch<C> *b, const char *name) {
    const OrderVerdict v = hyb_check(name, b->phase, b->rounds, b->doc->right);
    if (!v.ok) { set_error("%s", v.text); return REEF_ERR_ARG; }
    return REEF_OK;
}

static constexpr size_t HYB_M_MAX = 4096, HYB_ENTRIES_MAX = (size_t)1 << 24, HYB_EQ_GROUP_ENTRIES = (size_t)1 << 20;

template <int C> static reef_status v_hyrax_batch_create(void **impl, void *doc_impl, size_t m_max) {
    HyraxCtx<C> *doc = (HyraxCtx<C> *)doc_impl;
    if (!impl || !doc) { set_error("null argument"); return REEF_ERR_ARG; }
    if (m_max > HYB_M_MAX) { set_error("reef_hyrax_batch_create: m_max = %zu exceeds %zu", m_max, HYB_M_MAX); return REEF_ERR_ARG; }
    if (m_max * (size_t)doc->cols > HYB_ENTRIES_MAX) {
        set_error("reef_hyrax_batch_create: m_max * 2^right = %zu * %u exceeds %zu entries", m_max, doc->cols, HYB_ENTRIES_MAX);
        return REEF_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(doc->mu);
    REEF_ON_DEVICE(doc->device);
    HyraxBatch<C> *b = new HyraxBatch<C>();
    b->doc = doc;
    b->device = doc->device;
    b->m_max = m_max;
    const size_t vec = std::max<size_t>(m_max, 1) * doc->cols * sizeof(fe256);
    reef_status st = b->a.ensure(vec);
    if (st == REEF_OK) st = b->b.ensure(vec);
    if (st == REEF_OK) st = b->part.ensure(std::max<size_t>((size_t)doc->chunks * doc->cols, doc->bchunks) * sizeof(fe256));
    if (st != REEF_OK) { hyrax_batch_free(b); return st; }
    *impl = b;
    return REEF_OK;
}
template <int C> static void v_hyrax_batch_destroy(void *impl) { hyrax_batch_free((HyraxBatch<C> *)impl); }

template <int C>
static reef_status v_hyrax_batch_eval_begin(void *impl, void *key_impl, const reef_fe *points, size_t m, bool is_mont, reef_fe *evals, reef_fe *lz_blinds) {
    constexpr int F = HyraxBatch<C>::F;
    HyraxBatch<C> *b = (HyraxBatch<C> *)impl;
    HyraxCtx<C> *c = b->doc;
    Ctx<C> *key = (Ctx<C> *)key_impl;
    if (m > b->m_max) { set_error("reef_hyrax_batch_eval_begin: m = %zu exceeds the batch's m_max = %zu", m, b->m_max); return REEF_ERR_ARG; }
    if (m == 0) return REEF_OK;
    if (!key || !points) { set_error("null argument"); return REEF_ERR_ARG; }
    const u32 nv = c->left + c->right;
    for (size_t t = 0; t < m; ++t)
        for (u32 j = 0; j < nv; ++j)
            if (!fe_valid(points + t * nv + j, F)) {
                set_error("reef_hyrax_batch_eval_begin: points[%zu][%u] is not below the modulus", t, j);
                return REEF_ERR_ARG;
            }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    size_t key_n = 0;
    REEF_TRY(key_matches(key, c->device, "reef_hyrax_batch_eval_begin", "Hyrax", &key_n));
    if (key_n != c->cols) {
        set_error("reef_hyrax_batch_eval_begin: the key holds %zu points, the argument needs exactly 2^(num_vars - left_vars) = %u", key_n, c->cols);
        return REEF_ERR_ARG;
    }
    u32 split = 1;
    {
        std::lock_guard<std::mutex> kl(key->mu);
        split = key->wsplit_world;
    }
    if (split > 1) { set_error("reef_hyrax_batch_eval_begin: the key has a window split set (its MSMs are partial sums)"); return REEF_ERR_ARG; }
    REEF_TRY(call.enter(&b->phase));
    const u32 rows = c->rows, cols = c->cols;
    const size_t G = std::min<size_t>(m, std::max<size_t>(1, HYB_EQ_GROUP_ENTRIES / ((size_t)rows + cols)));   // the points whose eq tables exist at once
    REEF_TRY(b->pts.ensure(m * nv * sizeof(fe256)));
    REEF_TRY(b->eqs.ensure((G * ((size_t)rows + cols) + 1) * sizeof(fe_limbs)));
    REEF_TRY(b->dot.ensure(m * 20 * sizeof(u64)));
    REEF_TRY(b->res.ensure(2 * m * sizeof(fe256)));
    hipStream_t st = c->stream;
    fe_limbs *Leq = b->eqs.template as<fe_limbs>(), *Req = Leq + G * rows, *one = Req + G * cols;
    unsigned long long *dot = b->dot.template as<unsigned long long>();
    fe256 *part = b->part.template as<fe256>(), *a = b->a.template as<fe256>(), *pts = b->pts.template as<fe256>();
    REEF_HIP_TRY(hipMemcpyAsync(pts, points, m * nv * sizeof(fe256), hipMemcpyHostToDevice, st));
    REEF_HIP_TRY(hipMemsetAsync(dot, 0, m * 20 * sizeof(u64), st));
    MlePoint none;
    memset(&none, 0, sizeof none);
    hipLaunchKernelGGL(k_mle_eq<F>, dim3(1), dim3(256), 0, st, none, 0u, 0u, 0, one);
    for (size_t g0 = 0; g0 < m; g0 += G) {
        const u32 g = (u32)std::min(G, m - g0);
        hipLaunchKernelGGL(k_hyb_eq<F>, dim3(ceil_div(rows, 256), g), dim3(256), 0, st, (const fe256 *)pts, nv, 0u, c->left, (int)is_mont, (u32)g0, Leq,
                           (fe256 *)nullptr, 0u);
        hipLaunchKernelGGL(k_hyb_eq<F>, dim3(ceil_div(cols, 256), g), dim3(256), 0, st, (const fe256 *)pts, nv, c->left, c->right, (int)is_mont, (u32)g0, Req,
                           b->b.template as<fe256>(), cols);
        for (u32 t = 0; t < g; ++t) {      // the document pass of one point after the other on the stream: no host wait between them
            const size_t i = g0 + t;
            const fe_limbs *L = Leq + (size_t)t * rows, *R = Req + (size_t)t * cols;
            if (c->has_blinds) {           // the blinds as a one-column table: sum_i L_i blind_i
                mle_launch_bound_any<C>(st, 32, c->rb.p, rows, rows, 1, c->brpc, c->bchunks, L, part);
                hipLaunchKernelGGL((k_mle_finish<F, false>), dim3(1), dim3(256), 0, st, (const fe256 *)part, c->bchunks, 1u, (const fe_limbs *)one, 0,
                                   (fe256 *)nullptr, dot + 20 * i + 10);
            }
            mle_launch_bound_any<C>(st, c->eb, c->z.p, c->n, rows, cols, c->rpc, c->chunks, L, part);
            if (c->eb == 32)
                hipLaunchKernelGGL((k_mle_finish<F, false>), dim3(ceil_div(cols, 256)), dim3(256), 0, st, (const fe256 *)part, c->chunks, cols, R, 0,
                                   a + i * cols, dot + 20 * i);
            else
                hipLaunchKernelGGL((k_mle_finish<F, true>), dim3(ceil_div(cols, 256)), dim3(256), 0, st, (const fe256 *)part, c->chunks, cols, R, 0,
                                   a + i * cols, dot + 20 * i);
        }
    }
    hipLaunchKernelGGL(k_hyb_eval_final<F>, dim3(ceil_div(2 * m, 256)), dim3(256), 0, st, (const unsigned long long *)dot, (u32)m, (int)(c->eb != 32),
                       b->res.template as<fe256>());
    REEF_HIP_TRY(hipGetLastError());
    std::vector<fe256> h(2 * m);
    REEF_HIP_TRY(hipMemcpyAsync(h.data(), b->res.p, 2 * m * sizeof(fe256), hipMemcpyDeviceToHost, st));
    REEF_HIP_TRY(hipStreamSynchronize(st));
    for (size_t t = 0; t < m; ++t) {
        const fe256 e = fe_to_caller<F>(fe_from_integer<F>(h[2 * t]), is_mont), l = fe_to_caller<F>(fe_from_integer<F>(h[2 * t + 1]), is_mont);
        if (evals) memcpy(evals + t, &e, sizeof e);
        if (lz_blinds) memcpy(lz_blinds + t, &l, sizeof l);
    }
    b->key = key;
    b->m = m;
    b->rounds = 0;
    b->len = cols;
    b->with_h = false;
    return call.done(HY_EVAL);
}

// L, R of the round the vectors stand at, for every proof: the 2 m x n scalars over the original key on the doc ctx's stream `st`, then --
// on the key ctx's stream, ordered after `st` by the doc's event -- one pass of the row pipeline with rows = 2 m, one launch for the
// blind terms, one copy of the 2 m points and the call's one wait.
template <int C> static reef_status hyb_cross(HyraxBatch<C> *b, hipStream_t st, reef_jacobian *L, reef_jacobian *R) {
    HyraxCtx<C> *c = b->doc;
    Ctx<C> *key = b->key;
    const size_t m = b->m, n = c->cols;
    const u32 k = b->rounds;
    REEF_TRY(b->coef.ensure((m << k) * sizeof(fe256)));
    REEF_TRY(b->scal.ensure(2 * m * n * sizeof(fe256)));
    REEF_TRY(b->jac.ensure(2 * m * sizeof(jacobian256)));
    hipLaunchKernelGGL(k_hyb_coef<C>, dim3(ceil_div((size_t)1 << k, 256), (u32)m), dim3(256), 0, st, (const fe256 *)b->chal.p, (u32)m, k,
                       b->coef.template as<fe256>());
    hipLaunchKernelGGL(k_hyb_expand<C>, dim3(ceil_div(n, 256), (u32)m), dim3(256), 0, st, (const fe256 *)b->a.p, (u32)n, (u32)b->len,
                       (const fe256 *)b->coef.p, k, (u32)n, b->scal.template as<fe256>());
    REEF_HIP_TRY(hipGetLastError());
    hipStream_t ks = (hipStream_t)v_ctx_stream<C>(key);
    if (!ks) return REEF_ERR_HIP;
    REEF_HIP_TRY(hipEventRecord(c->ev, st));
    REEF_HIP_TRY(hipStreamWaitEvent(ks, c->ev, 0));
    // full-width scalars (max_bits = 255: the route measures nothing and waits for nothing), results left on the device
    REEF_TRY(v_msm_rows<C>(key, (const reef_fe *)b->scal.p, 2 * m, n, REEF_DEVICE, false, 255, nullptr, nullptr, b->jac.template as<reef_jacobian>(),
                           REEF_DEVICE));
    std::lock_guard<std::mutex> kl(key->mu);
    CtxScope<C> scope(key);
    REEF_TRY(scope.enter());
    hipLaunchKernelGGL(k_hyb_blind<C>, dim3(ceil_div(2 * m * BLIND_LANES, 64)), dim3(64), 0, key->stream, b->jac.template as<jacobian256>(),
                       (const fe256 *)b->out.p, b->with_h ? (const fe256 *)b->hbl.p : (const fe256 *)nullptr, (const affine256 *)b->qtab.p,
                       (u32)b->npts, (u32)m, (u32)(2 * m));
    REEF_HIP_TRY(hipGetLastError());
    b->lr.resize(2 * m);
    REEF_HIP_TRY(hipMemcpyAsync(b->lr.data(), b->jac.p, 2 * m * sizeof(jacobian256), hipMemcpyDeviceToHost, key->stream));
    REEF_HIP_TRY(hipStreamSynchronize(key->stream));
    for (size_t t = 0; t < m; ++t) {
        memcpy(L + t, &b->lr[2 * t], sizeof(jacobian256));
        memcpy(R + t, &b->lr[2 * t + 1], sizeof(jacobian256));
    }
    return REEF_OK;
}
// The h term's 2 m blinds of the coming cross terms (canonical integers; nullptr: zeros) onto `st`
template <int C> static reef_status hyb_set_blinds(HyraxBatch<C> *b, hipStream_t st, const std::vector<fe256> *hb) {
    const size_t bytes = 2 * b->m * sizeof(fe256);
    REEF_TRY(b->hbl.ensure(bytes));
    if (!hb) { REEF_HIP_TRY(hipMemsetAsync(b->hbl.p, 0, bytes, st)); return REEF_OK; }
    b->hb = *hb;
    REEF_HIP_TRY(hipMemcpyAsync(b->hbl.p, b->hb.data(), bytes, hipMemcpyHostToDevice, st));
    return REEF_OK;
}
// The nibble tables of q_0 .. q_{m-1} and, when given, h on the key ctx's stream: one upload, one import, the small-key table builder
// over HYB_TAB_CHUNK points at a time (its scratch stays that of a key of so many points); waits.
template <int C> static reef_status hyb_build_tables(HyraxBatch<C> *b, const reef_affine *q, const reef_affine *h) {
    Ctx<C> *key = b->key;
    const size_t m = b->m, npts = m + (h ? 1 : 0);
    std::vector<reef_affine> host(npts);
    memcpy(host.data(), q, m * sizeof(reef_affine));
    if (h) host[m] = *h;
    std::lock_guard<std::mutex> kl(key->mu);
    CtxScope<C> scope(key);
    REEF_TRY(scope.enter());
    REEF_TRY(b->qraw.ensure(2 * npts * sizeof(affine256)));
    REEF_TRY(b->qtab.ensure(small_table_points(npts) * sizeof(affine256)));
    affine256 *raw = b->qraw.template as<affine256>(), *imp = raw + npts, *tab = b->qtab.template as<affine256>();
    REEF_HIP_TRY(hipMemcpyAsync(raw, host.data(), npts * sizeof(reef_affine), hipMemcpyHostToDevice, key->stream));
    hipLaunchKernelGGL(k_import_key<C>, dim3(ceil_div(npts, 256)), dim3(256), 0, key->stream, (const affine256 *)raw, (u32)npts, imp);
    for (size_t p0 = 0; p0 < npts; p0 += HYB_TAB_CHUNK)
        REEF_TRY(small_build<C>(key, imp + p0, std::min<size_t>(HYB_TAB_CHUNK, npts - p0), tab + small_table_points(p0)));
    REEF_HIP_TRY(hipStreamSynchronize(key->stream));
    b->npts = npts;
    return REEF_OK;
}

template <int C>
static reef_status v_hyrax_batch_ipa_begin(void *impl, const reef_affine *q, const reef_affine *h, const reef_fe *blinds, bool is_mont, reef_jacobian *L,
                                           reef_jacobian *R) {
    constexpr int F = HyraxBatch<C>::F;
    HyraxBatch<C> *b = (HyraxBatch<C> *)impl;
    HyraxCtx<C> *c = b->doc;
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(hyb_expect(b, "reef_hyrax_batch_ipa_begin"));
    if (!q || !L || !R) { set_error("null argument"); return REEF_ERR_ARG; }
    if (h && !blinds) { set_error("reef_hyrax_batch_ipa_begin: h given without the 2 m blinds of round 0"); return REEF_ERR_ARG; }
    const size_t m = b->m;
    std::vector<fe256> hb(h ? 2 * m : 0);
    if (h) REEF_TRY(fe_import_all<F>(blinds, 2 * m, is_mont, "reef_hyrax_batch_ipa_begin", "blinds", hb.data()));
    REEF_TRY(call.enter(&b->phase));
    REEF_TRY(hyb_build_tables(b, q, h));
    b->with_h = h != nullptr;
    hipStream_t st = c->stream;
    const u32 half = c->cols / 2, grid = sp_grid(half);
    REEF_TRY(b->partial.ensure(m * grid * 27 * sizeof(unsigned long long)));
    REEF_TRY(b->out.ensure(2 * m * sizeof(fe256)));
    REEF_TRY(b->chal.ensure(2 * (size_t)c->right * b->m_max * sizeof(fe256)));
    if (b->with_h) REEF_TRY(hyb_set_blinds(b, st, &hb));
    hipLaunchKernelGGL(k_hyb_sums<F>, dim3(grid, (u32)m), dim3(SP_THREADS), 0, st, (const fe256 *)b->a.p, (const fe256 *)b->b.p, c->cols, half,
                       b->partial.template as<unsigned long long>());
    hipLaunchKernelGGL(k_hyb_finish<F>, dim3((u32)m), dim3(SP_THREADS), 0, st, (const unsigned long long *)b->partial.p, grid, b->out.template as<fe256>());
    REEF_HIP_TRY(hipGetLastError());
    b->rounds = 0;
    REEF_TRY(hyb_cross(b, st, L, R));
    return call.done(HY_IPA);
}

// r[0 .. m) of a fold: below the modulus and non-zero, naming the proof otherwise; ch = r (m entries) then r^-1 (m), internal form
template <int C>
static reef_status hyb_challenges(HyraxBatch<C> *b, const reef_fe *r, bool is_mont, const char *name, std::vector<fe256> &ch) {
    constexpr int F = HyraxBatch<C>::F;
    if (!r) { set_error("null argument"); return REEF_ERR_ARG; }
    const size_t m = b->m;
    ch.resize(2 * m);
    for (size_t t = 0; t < m; ++t) {
        if (!fe_valid(r + t, F)) { set_error("%s: r[%zu] is not below the modulus", name, t); return REEF_ERR_ARG; }
        const fe ri = fe_import<F>(r + t, is_mont);
        if (fe_is_literal_zero(fe_canon<F>(ri))) { set_error("%s: r[%zu] is zero (it has no inverse)", name, t); return REEF_ERR_ARG; }
        ch[t] = fe_to_table<F>(ri);
        ch[m + t] = fe_to_table<F>(fe_inv<F>(ri));
    }
    return REEF_OK;
}
// ... onto `st` as the challenges of round b->rounds (k_hyb_coef's layout)
template <int C> static reef_status hyb_upload_challenges(HyraxBatch<C> *b, hipStream_t st, const std::vector<fe256> &ch, const fe256 **d_r) {
    b->ch = ch;
    fe256 *dst = b->chal.template as<fe256>() + 2 * (size_t)b->rounds * b->m;
    REEF_HIP_TRY(hipMemcpyAsync(dst, b->ch.data(), 2 * b->m * sizeof(fe256), hipMemcpyHostToDevice, st));
    *d_r = dst;
    return REEF_OK;
}

template <int C>
static reef_status v_hyrax_batch_ipa_round(void *impl, const reef_fe *r, const reef_fe *blinds, bool is_mont, reef_jacobian *L, reef_jacobian *R) {
    constexpr int F = HyraxBatch<C>::F;
    HyraxBatch<C> *b = (HyraxBatch<C> *)impl;
    HyraxCtx<C> *c = b->doc;
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(hyb_expect(b, "reef_hyrax_batch_ipa_round"));
    if (!L || !R) { set_error("null argument"); return REEF_ERR_ARG; }
    const size_t m = b->m;
    std::vector<fe256> ch, hb(blinds ? 2 * m : 0);
    REEF_TRY(hyb_challenges(b, r, is_mont, "reef_hyrax_batch_ipa_round", ch));
    if (blinds && !b->with_h) { set_error("reef_hyrax_batch_ipa_round: blinds given, but reef_hyrax_batch_ipa_begin took no h term"); return REEF_ERR_ARG; }
    if (blinds) REEF_TRY(fe_import_all<F>(blinds, 2 * m, is_mont, "reef_hyrax_batch_ipa_round", "blinds", hb.data()));
    REEF_TRY(call.enter(&b->phase));
    hipStream_t st = c->stream;
    if (b->with_h) REEF_TRY(hyb_set_blinds(b, st, blinds ? &hb : nullptr));   // NULL: zero blinds this round
    HybRound p;
    memset(&p, 0, sizeof p);
    REEF_TRY(hyb_upload_challenges(b, st, ch, &p.r));
    p.rinv = p.r + m;
    p.a = b->a.template as<fe256>();
    p.b = b->b.template as<fe256>();
    p.stride = c->cols;
    p.q = (u32)(b->len / 4);
    p.partial = b->partial.template as<unsigned long long>();
    const u32 grid = sp_grid(p.q);                            // never more blocks than ipa_begin sized partial for
    hipLaunchKernelGGL(k_hyb_round<F>, dim3(grid, (u32)m), dim3(SP_THREADS), 0, st, p);
    hipLaunchKernelGGL(k_hyb_finish<F>, dim3((u32)m), dim3(SP_THREADS), 0, st, (const unsigned long long *)b->partial.p, grid, b->out.template as<fe256>());
    REEF_HIP_TRY(hipGetLastError());
    b->len /= 2;
    ++b->rounds;
    REEF_TRY(hyb_cross(b, st, L, R));
    return call.done(HY_IPA);
}

template <int C> static reef_status v_hyrax_batch_finish(void *impl, const reef_fe *r_last, bool is_mont, reef_fe *a_hat, reef_fe *b_hat) {
    constexpr int F = HyraxBatch<C>::F;
    HyraxBatch<C> *b = (HyraxBatch<C> *)impl;
    HyraxCtx<C> *c = b->doc;
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(hyb_expect(b, "reef_hyrax_batch_finish"));
    if (!a_hat) { set_error("null argument"); return REEF_ERR_ARG; }
    const size_t m = b->m;
    std::vector<fe256> ch;
    REEF_TRY(hyb_challenges(b, r_last, is_mont, "reef_hyrax_batch_finish", ch));
    REEF_TRY(call.enter(&b->phase));
    hipStream_t st = c->stream;
    const fe256 *d_r = nullptr;
    REEF_TRY(hyb_upload_challenges(b, st, ch, &d_r));
    REEF_TRY(b->res.ensure(2 * m * sizeof(fe256)));
    hipLaunchKernelGGL(k_hyb_last<F>, dim3(ceil_div(m, 256)), dim3(256), 0, st, b->a.template as<fe256>(), b->b.template as<fe256>(), c->cols, (u32)m, d_r,
                       d_r + m, is_mont ? (int)SP_FORM_MONT : (int)SP_FORM_INTEGER, b->res.template as<fe256>());
    REEF_HIP_TRY(hipGetLastError());
    std::vector<fe256> h(2 * m);
    REEF_HIP_TRY(hipMemcpyAsync(h.data(), b->res.p, 2 * m * sizeof(fe256), hipMemcpyDeviceToHost, st));
    REEF_HIP_TRY(hipStreamSynchronize(st));
    memcpy(a_hat, h.data(), m * sizeof(fe256));
    if (b_hat) memcpy(b_hat, h.data() + m, m * sizeof(fe256));
    b->len = 1;
    b->key = nullptr;
    return call.done(HY_DONE);
}

// which: 0 a, 1 b of proof `proof`, the first `count` of their current length
template <int C> static reef_status v_hyrax_batch_read(void *impl, size_t proof, int which, size_t count, reef_fe *out, bool to_mont) {
    constexpr int F = HyraxBatch<C>::F;
    HyraxBatch<C> *b = (HyraxBatch<C> *)impl;
    HyraxCtx<C> *c = b->doc;
    if (count && !out) { set_error("null argument"); return REEF_ERR_ARG; }
    if (which != 0 && which != 1) { set_error("reef_hyrax_batch_read: which must be 0 (a) or 1 (b)"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(hyb_expect(b, "reef_hyrax_batch_read"));
    if (proof >= b->m) { set_error("reef_hyrax_batch_read: proof %zu asked, the batch holds %zu", proof, b->m); return REEF_ERR_ARG; }
    if (count > b->len) { set_error("reef_hyrax_batch_read: %zu entries asked, the vector has %zu", count, b->len); return REEF_ERR_ARG; }
    if (!count) return REEF_OK;
    REEF_TRY(call.enter());
    REEF_TRY(b->stage.ensure(count * sizeof(fe256)));
    const fe256 *src = (which == 0 ? b->a : b->b).template as<fe256>() + proof * c->cols;
    hipLaunchKernelGGL(k_fe_export<F>, dim3(ceil_div(count, 256)), dim3(256), 0, c->stream, src, (u64)count, (int)(which == 0), (int)to_mont,
                       b->stage.template as<fe256>());
    REEF_HIP_TRY(hipGetLastError());
    REEF_HIP_TRY(hipMemcpyAsync(out, b->stage.p, count * sizeof(fe256), hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    return REEF_OK;
}

template <int C> HyraxBatchVTable make_hyrax_batch_vtable() {
    return HyraxBatchVTable{v_hyrax_batch_create<C>, v_hyrax_batch_destroy<C>, v_hyrax_batch_eval_begin<C>, v_hyrax_batch_ipa_begin<C>,
                            v_hyrax_batch_ipa_round<C>, v_hyrax_batch_finish<C>, v_hyrax_batch_read<C>};
}

}  // namespace reef
