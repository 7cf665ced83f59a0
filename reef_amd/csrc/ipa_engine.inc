// The IPA rounds of the batched opening (3h: open_engine.inc, on a NIFS ctx) and of the Hyrax consistency argument (3i:
// hyrax_engine.inc); included after nifs_engine.inc.  IpaRun holds a, b, the cross terms over the resident key and the folds
// (open_kernels.inc): the owner fills a and b, then drives ipa_cross / ipa_round / ipa_last on its own stream, and releases it.
// With n_small set (reef_spartan_open_set_small_key / reef_hyrax_set_small_key) the rounds from length n_small on run over a folded key.
namespace reef {

template <int C> struct IpaRun {
    static constexpr int F = 1 - C;
    DevBuf a, b;                         // a (canonical integers: what the cross-term MSM reads) and b (internal form), n entries each
    DevBuf partial, out;                 // block sums; out: 0 c, 1 c_L, 2 c_R (canonical integers), 3 a_hat (the caller's form)
    DevBuf blinds, htab;                 // the optional second blind term: two canonical integers, its point's nibble table
    Ctx<C> *key = nullptr;               // the gens_v key ctx, from the owner's begin to the last fold
    size_t n = 0, len = 0;               // n; the length of a and b as they stand
    reef_affine q = {};                  // the point of the c_L, c_R blind term
    bool with_h = false;                 // L, R also take blinds[0] h, blinds[1] h (htab)
    fe256 hb[2] = {};                    // host copy of the blinds being uploaded
    std::vector<fe256> w1s, w2s;         // the IPA challenges so far: r^-1 and r, canonical integers (reef_fold's convention)
    size_t n_small = 0;                  // the length at which the rounds move to a folded key (0: never); the owner's setting at ipa_alloc
    Ctx<C> *folded = nullptr;            // the key of the n_small generators folded_at rounds away (reef_msm_ctx_create_folded), this run's own
    size_t folded_at = 0;                // the challenges the folded key holds: L, R over it take w1s, w2s from here on
    void drop_folded() {
        if (folded) v_ctx_destroy<C>(folded);
        folded = nullptr;
        folded_at = 0;
    }
    void release() {
        drop_folded();
        for (DevBuf *d : {&a, &b, &partial, &out, &blinds, &htab}) d->release();
    }
};
// the blocks of a reduction over n entries (the sum-check rounds of N5 and the folds here)
static u32 sp_grid(size_t n) { return (u32)std::max<size_t>(1, std::min<size_t>(SP_BLOCKS, ceil_div(n, SP_THREADS))); }
// the workspace for n entries; the rounds start over (no key, no folded key, no challenges, no h term) with the owner's n_small
template <int C> static reef_status ipa_alloc(IpaRun<C> *ip, size_t n, size_t n_small) {
    ip->drop_folded();
    ip->n_small = n_small;
    REEF_TRY(ip->a.ensure(n * sizeof(fe256)));
    REEF_TRY(ip->b.ensure(n * sizeof(fe256)));
    REEF_TRY(ip->partial.ensure(SP_BLOCKS * 27 * sizeof(unsigned long long)));
    REEF_TRY(ip->out.ensure(4 * sizeof(fe256)));
    REEF_TRY(ip->blinds.ensure(2 * sizeof(fe256)));
    ip->key = nullptr;
    ip->n = ip->len = n;
    ip->with_h = false;
    ip->w1s.clear();
    ip->w2s.clear();
    return REEF_OK;
}
// the sums of `grid` blocks -> out + slot (nv values, canonical integers); no wait
template <int C> static void ipa_sums(IpaRun<C> *ip, hipStream_t st, u32 grid, u32 nv, u32 slot) {
    hipLaunchKernelGGL(k_sp_finish<IpaRun<C>::F>, dim3(1), dim3(SP_THREADS), 0, st, (const unsigned long long *)ip->partial.p, grid, nv,
                       (int)SP_FORM_INTEGER, ip->out.template as<fe256>() + slot);
}
// out[0] (a canonical integer) to the host in the caller's form
template <int C> static reef_status ipa_fetch(IpaRun<C> *ip, hipStream_t st, bool is_mont, reef_fe *dst) {
    constexpr int F = IpaRun<C>::F;
    fe256 v;
    REEF_HIP_TRY(hipMemcpyAsync(&v, ip->out.p, sizeof v, hipMemcpyDeviceToHost, st));
    REEF_HIP_TRY(hipStreamSynchronize(st));
    const fe256 o = fe_to_caller<F>(fe_from_integer<F>(v), is_mont);
    memcpy(dst, &o, sizeof o);
    return REEF_OK;
}
// The second blind term's point h: its nibble table, built on the key ctx's stream (ip->key set); L, R take the term from now on
template <int C> static reef_status ipa_set_h(IpaRun<C> *ip, const reef_affine *h) {
    Ctx<C> *key = ip->key;
    std::lock_guard<std::mutex> kl(key->mu);
    CtxScope<C> scope(key);
    REEF_TRY(scope.enter());
    REEF_TRY(point_table_build<C>(key, h, ip->htab));
    ip->with_h = true;
    return REEF_OK;
}
// The second blind term's two blinds (canonical integers) onto `st`, ahead of the next ipa_cross
template <int C> static reef_status ipa_set_blinds(IpaRun<C> *ip, hipStream_t st, const fe256 *b2) {
    memcpy(ip->hb, b2, sizeof ip->hb);
    REEF_HIP_TRY(hipMemcpyAsync(ip->blinds.p, ip->hb, sizeof ip->hb, hipMemcpyHostToDevice, st));
    return REEF_OK;
}
// L, R of the round the vectors stand at: the cross-term MSMs over the resident gens_v key on the key ctx's stream, ordered after
// the owner's stream `st` by the event `ev`, with c_L q, c_R q (out[1], out[2]) added through q's nibble table, and blinds[0] h,
// blinds[1] h through h's when with_h.  One host wait.
template <int C> static reef_status ipa_cross(IpaRun<C> *ip, hipStream_t st, hipEvent_t ev, reef_jacobian *L, reef_jacobian *R) {
    Ctx<C> *key = ip->folded ? ip->folded : ip->key;          // after the switch: the folded key, and only the challenges drawn since
    hipStream_t ks = (hipStream_t)v_ctx_stream<C>(key);
    if (!ks) return REEF_ERR_HIP;
    REEF_HIP_TRY(hipEventRecord(ev, st));
    REEF_HIP_TRY(hipStreamWaitEvent(ks, ev, 0));
    std::lock_guard<std::mutex> kl(key->mu);
    CtxScope<C> scope(key);
    REEF_TRY(scope.enter());
    const size_t k0 = ip->folded ? ip->folded_at : 0, k = ip->w1s.size() - k0;
    return ipa_cross_run<C>(key, ip->a.template as<fe256>(), ip->len, false, k ? (const reef_fe *)(ip->w1s.data() + k0) : nullptr,
                            k ? (const reef_fe *)(ip->w2s.data() + k0) : nullptr, k, ip->out.template as<fe256>() + 1, &ip->q,
                            ip->with_h ? ip->blinds.template as<fe256>() : nullptr, ip->with_h ? ip->htab.template as<affine256>() : nullptr, L, R);
}
// One IPA round: a, b folded with r (internal form, non-zero) fused with the next round's c_L, c_R; then that round's L, R
template <int C> static reef_status ipa_round(IpaRun<C> *ip, hipStream_t st, hipEvent_t ev, const fe &ri, reef_jacobian *L, reef_jacobian *R) {
    constexpr int F = IpaRun<C>::F;
    const fe rinv = fe_inv<F>(ri);
    OpRound p;
    memset(&p, 0, sizeof p);
    p.a = ip->a.template as<fe256>();
    p.b = ip->b.template as<fe256>();
    p.q = (u32)(ip->len / 4);
    p.r = fe_to_table<F>(ri);
    p.rinv = fe_to_table<F>(rinv);
    p.partial = ip->partial.template as<unsigned long long>();
    const u32 grid = sp_grid(p.q);
    hipLaunchKernelGGL(k_op_round<F>, dim3(grid), dim3(SP_THREADS), 0, st, p);
    ipa_sums(ip, st, grid, 2, 1);                             // the next round's c_L, c_R
    REEF_HIP_TRY(hipGetLastError());
    ip->len /= 2;
    ip->w1s.push_back(fe_to_integer<F>(rinv));
    ip->w2s.push_back(fe_to_integer<F>(ri));
    if (ip->n_small && !ip->folded && ip->n > ip->n_small && ip->len == ip->n_small) {
        // the switch: the len generators these challenges lead to become a resident key of their own, made on the key ctx's stream and
        // waited for (it reads the key's tables and the challenges, nothing of this run's vectors); small enough, it gets nibble tables
        reef_msm_opts o = {};
        o.bucket_groups = 1;
        void *impl = nullptr;
        REEF_TRY(v_ctx_create_folded<C>(&impl, ip->key, (const reef_fe *)ip->w1s.data(), (const reef_fe *)ip->w2s.data(), ip->w1s.size(), &o));
        ip->folded = (Ctx<C> *)impl;
        ip->folded_at = ip->w1s.size();
    }
    return ipa_cross(ip, st, ev, L, R);
}
// The last fold with r: a_hat = a[0] (and b_hat = b[0] when asked) to the host in the caller's form; the key is let go
template <int C> static reef_status ipa_last(IpaRun<C> *ip, hipStream_t st, const fe &ri, bool is_mont, reef_fe *a_hat, reef_fe *b_hat) {
    constexpr int F = IpaRun<C>::F;
    hipLaunchKernelGGL(k_op_last<F>, dim3(1), dim3(64), 0, st, ip->a.template as<fe256>(), ip->b.template as<fe256>(), fe_to_table<F>(ri),
                       fe_to_table<F>(fe_inv<F>(ri)), is_mont ? (int)SP_FORM_MONT : (int)SP_FORM_INTEGER, ip->out.template as<fe256>() + 3);
    REEF_HIP_TRY(hipGetLastError());
    fe256 bv;
    REEF_HIP_TRY(hipMemcpyAsync(a_hat, ip->out.template as<fe256>() + 3, sizeof(fe256), hipMemcpyDeviceToHost, st));
    if (b_hat) REEF_HIP_TRY(hipMemcpyAsync(&bv, ip->b.p, sizeof bv, hipMemcpyDeviceToHost, st));
    REEF_HIP_TRY(hipStreamSynchronize(st));
    if (b_hat) {
        const fe256 o = fe_to_caller<F>(fe_from_table(bv), is_mont);
        memcpy(b_hat, &o, sizeof o);
    }
    ip->len = 1;
    ip->key = nullptr;
    ip->drop_folded();
    return REEF_OK;
}
// which: 0 a, 1 b: the first `count` (<= len) through `stage` to the host
template <int C> static reef_status ipa_read(IpaRun<C> *ip, hipStream_t st, DevBuf &stage, int which, size_t count, reef_fe *out, bool to_mont) {
    REEF_TRY(stage.ensure(count * sizeof(fe256)));
    const fe256 *src = (which == 0 ? ip->a : ip->b).template as<fe256>();
    hipLaunchKernelGGL(k_fe_export<IpaRun<C>::F>, dim3(ceil_div(count, 256)), dim3(256), 0, st, src, (u64)count, (int)(which == 0), (int)to_mont,
                       stage.template as<fe256>());
    REEF_HIP_TRY(hipGetLastError());
    REEF_HIP_TRY(hipMemcpyAsync(out, stage.p, count * sizeof(fe256), hipMemcpyDeviceToHost, st));
    REEF_HIP_TRY(hipStreamSynchronize(st));
    return REEF_OK;
}

}  // namespace reef
