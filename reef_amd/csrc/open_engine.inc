// Host side of the batched IPA opening of the final SNARK (open_kernels.inc; include/reef_msm.h 3h) on a NIFS ctx; included after
// spartan_engine.inc.  The state machine goes on from reef_spartan_inner_claims: open_begin -> open_fold -> open_ipa_begin ->
// open_ipa_round x (log2(n) - 1) -> open_finish.  W, E, u, X, T and the NIFS state are read, never written.
//
// The IPA rounds themselves (IpaRun: a, b, the cross terms over the resident key, the folds) are shared with the Hyrax consistency
// argument (hyrax_engine.inc, 3i): the owner fills a and b, then drives ipa_cross / ipa_round / ipa_last on its own stream.
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
};
template <int C> static void ipa_run_release(IpaRun<C> *ip) {
    if (!ip) return;
    for (DevBuf *b : {&ip->a, &ip->b, &ip->partial, &ip->out, &ip->blinds, &ip->htab}) b->release();
    delete ip;
}
// the workspace for n entries; the rounds start over (no key, no challenges, no h term)
template <int C> static reef_status ipa_alloc(IpaRun<C> *ip, size_t n) {
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
    Ctx<C> *key = ip->key;
    hipStream_t ks = (hipStream_t)v_ctx_stream<C>(key);
    if (!ks) return REEF_ERR_HIP;
    REEF_HIP_TRY(hipEventRecord(ev, st));
    REEF_HIP_TRY(hipStreamWaitEvent(ks, ev, 0));
    std::lock_guard<std::mutex> kl(key->mu);
    CtxScope<C> scope(key);
    REEF_TRY(scope.enter());
    const size_t k = ip->w1s.size();
    return ipa_cross_run<C>(key, ip->a.template as<fe256>(), ip->len, false, k ? (const reef_fe *)ip->w1s.data() : nullptr,
                            k ? (const reef_fe *)ip->w2s.data() : nullptr, k, ip->out.template as<fe256>() + 1, &ip->q,
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

// The opening call `name` is the one expected: open_begin after inner_claims (or to restart an opening), the rest in order
template <int C> static reef_status op_expect(NifsCtx<C> *c, const char *name) {
    SpartanState<C> *s = c->sp;
    const bool begin = strcmp(name, "reef_spartan_open_begin") == 0;
    if (begin && s && s->gen == c->gen && s->phase >= SP_DONE) return REEF_OK;
    if (!begin && s && s->gen == c->gen && s->phase == SP_DONE) {
        set_error("%s: out of order, the next call is reef_spartan_open_begin", name);
        return REEF_ERR_ARG;
    }
    return sp_expect(c, name);
}

template <int C> static reef_status v_open_begin(void *impl, void *key_impl, bool is_mont, reef_fe *cross_term) {
    constexpr int F = NifsCtx<C>::F;
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    Ctx<C> *key = (Ctx<C> *)key_impl;
    if (!key || !cross_term) { set_error("null argument"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    REEF_TRY(op_expect(c, "reef_spartan_open_begin"));
    SpartanState<C> *s = c->sp;
    const size_t n = std::max(s->ncp, s->nvp);
    size_t key_n = 0;
    REEF_TRY(key_matches(key, c->device, "reef_spartan_open_begin", "NIFS", &key_n));
    if (key_n != n) {
        set_error("reef_spartan_open_begin: the key holds %zu points, the opening needs exactly n = max(num_cons_pad, num_vars_pad) = %zu", key_n, n);
        return REEF_ERR_ARG;
    }
    REEF_ON_DEVICE(c->device);
    DeviceScope scope(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(scope.enter());
    s->phase = SP_NONE;                                       // a failure half way leaves nothing to continue
    REEF_TRY(s->e1.ensure(s->ncp * sizeof(fe256)));
    REEF_TRY(s->e2.ensure(s->nvp * sizeof(fe256)));
    if (!s->ip) s->ip = new IpaRun<C>();
    IpaRun<C> *ip = s->ip;
    REEF_TRY(ipa_alloc(ip, n));
    const fe256 *e1 = s->e1.template as<fe256>(), *e2 = s->e2.template as<fe256>();
    REEF_TRY(fe_eq_table<F>(c->stream, s->pts, s->rx.data(), s->ell_x, s->e1.template as<fe256>()));
    REEF_TRY(fe_eq_table<F>(c->stream, s->pts, s->ry.data() + 1, s->ell_y - 1, s->e2.template as<fe256>()));
    const u32 nE = (u32)std::min(c->num_cons, s->nvp), nW = (u32)std::min(c->num_vars, s->ncp);
    const u32 grid = sp_grid(std::max(nE, nW));
    hipLaunchKernelGGL(k_op_cross<F>, dim3(grid), dim3(SP_THREADS), 0, c->stream, (const fe256 *)c->E.p, e2, nE, (const fe256 *)c->z1.p, e1, nW,
                       ip->partial.template as<unsigned long long>());
    ipa_sums(ip, c->stream, grid, 1, 0);
    REEF_HIP_TRY(hipGetLastError());
    REEF_TRY(ipa_fetch(ip, c->stream, is_mont, cross_term));
    ip->key = key;
    s->on = n;
    s->rounds = 0;
    s->phase = SP_OPEN_BEGUN;
    return REEF_OK;
}

template <int C> static reef_status v_open_fold(void *impl, const reef_fe *r, bool is_mont, reef_fe *c_out) {
    constexpr int F = NifsCtx<C>::F;
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    fe ri;
    REEF_TRY(fe_challenge<F>(r, is_mont, "reef_spartan_open_fold", ri));
    if (!c_out) { set_error("null argument"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    REEF_TRY(op_expect(c, "reef_spartan_open_fold"));
    SpartanState<C> *s = c->sp;
    REEF_ON_DEVICE(c->device);
    DeviceScope scope(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(scope.enter());
    s->phase = SP_NONE;
    OpFold p;
    memset(&p, 0, sizeof p);
    p.E = c->E.template as<fe256>();
    p.W = c->z1.template as<fe256>();
    p.e1 = s->e1.template as<fe256>();
    p.e2 = s->e2.template as<fe256>();
    p.nE = (u32)c->num_cons;
    p.nW = (u32)c->num_vars;
    p.n1 = (u32)s->ncp;
    p.n2 = (u32)s->nvp;
    p.h = (u32)(s->on / 2);
    p.r = fe_to_table<F>(ri);
    IpaRun<C> *ip = s->ip;
    p.a = ip->a.template as<fe256>();
    p.b = ip->b.template as<fe256>();
    p.partial = ip->partial.template as<unsigned long long>();
    const u32 grid = sp_grid(p.h);
    hipLaunchKernelGGL(k_op_fold<F>, dim3(grid), dim3(SP_THREADS), 0, c->stream, p);
    ipa_sums(ip, c->stream, grid, 3, 0);                      // c, then round 0's c_L, c_R where ipa_cross reads them
    REEF_HIP_TRY(hipGetLastError());
    REEF_TRY(ipa_fetch(ip, c->stream, is_mont, c_out));
    ip->len = ip->n;
    s->phase = SP_OPEN_FOLDED;
    return REEF_OK;
}

template <int C> static reef_status v_open_ipa_begin(void *impl, const reef_affine *q, reef_jacobian *L, reef_jacobian *R) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    if (!q || !L || !R) { set_error("null argument"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    REEF_TRY(op_expect(c, "reef_spartan_open_ipa_begin"));
    SpartanState<C> *s = c->sp;
    REEF_ON_DEVICE(c->device);
    DeviceScope scope(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(scope.enter());
    s->phase = SP_NONE;
    IpaRun<C> *ip = s->ip;
    ip->q = *q;
    ip->w1s.clear();
    ip->w2s.clear();
    REEF_TRY(ipa_cross(ip, c->stream, c->ev, L, R));
    s->rounds = 0;
    s->phase = SP_OPEN_IPA;
    return REEF_OK;
}

template <int C> static reef_status v_open_ipa_round(void *impl, const reef_fe *r, bool is_mont, reef_jacobian *L, reef_jacobian *R) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    fe ri;
    REEF_TRY(fe_challenge<NifsCtx<C>::F>(r, is_mont, "reef_spartan_open_ipa_round", ri, true));
    if (!L || !R) { set_error("null argument"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    REEF_TRY(op_expect(c, "reef_spartan_open_ipa_round"));
    SpartanState<C> *s = c->sp;
    REEF_ON_DEVICE(c->device);
    DeviceScope scope(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(scope.enter());
    s->phase = SP_NONE;
    REEF_TRY(ipa_round(s->ip, c->stream, c->ev, ri, L, R));
    ++s->rounds;
    s->phase = SP_OPEN_IPA;
    return REEF_OK;
}

template <int C> static reef_status v_open_finish(void *impl, const reef_fe *r_last, bool is_mont, reef_fe *a_hat) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    fe ri;
    REEF_TRY(fe_challenge<NifsCtx<C>::F>(r_last, is_mont, "reef_spartan_open_finish", ri, true));
    if (!a_hat) { set_error("null argument"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    REEF_TRY(op_expect(c, "reef_spartan_open_finish"));
    SpartanState<C> *s = c->sp;
    REEF_ON_DEVICE(c->device);
    DeviceScope scope(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(scope.enter());
    s->phase = SP_NONE;
    REEF_TRY(ipa_last(s->ip, c->stream, ri, is_mont, a_hat, nullptr));
    s->phase = SP_OPEN_DONE;
    return REEF_OK;
}

// which: 0 a, 1 b, the first `count` of their current length
template <int C> static reef_status v_open_read(void *impl, int which, size_t count, reef_fe *out, bool to_mont) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    if (count && !out) { set_error("null argument"); return REEF_ERR_ARG; }
    if (which != 0 && which != 1) { set_error("reef_spartan_open_read: which must be 0 (a) or 1 (b)"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    SpartanState<C> *s = c->sp;
    if (!s || s->gen != c->gen || s->phase < SP_OPEN_FOLDED) {
        const char *want = s && s->gen == c->gen && s->phase == SP_OPEN_BEGUN ? "reef_spartan_open_fold"
                           : s && s->gen == c->gen && s->phase == SP_DONE   ? "reef_spartan_open_begin"
                           : s && s->gen == c->gen                          ? sp_expected(s->phase, s->rounds, s->ell_x, s->ell_y)
                                                                            : "reef_spartan_begin";
        set_error("reef_spartan_open_read: a and b exist from reef_spartan_open_fold on; the next call is %s", want);
        return REEF_ERR_ARG;
    }
    if (count > s->ip->len) { set_error("reef_spartan_open_read: %zu entries asked, the vector has %zu", count, s->ip->len); return REEF_ERR_ARG; }
    if (!count) return REEF_OK;
    REEF_ON_DEVICE(c->device);
    DeviceScope scope(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(scope.enter());
    return ipa_read(s->ip, c->stream, c->stage, which, count, out, to_mont);
}

template <int C> OpenVTable make_open_vtable() {
    return OpenVTable{v_open_begin<C>, v_open_fold<C>, v_open_ipa_begin<C>, v_open_ipa_round<C>, v_open_finish<C>, v_open_read<C>};
}

}  // namespace reef
