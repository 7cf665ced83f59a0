// Host side of the batched IPA opening of the final SNARK (open_kernels.inc; include/reef_msm.h 3h) on a NIFS ctx; included after
// spartan_engine.inc.  The state machine goes on from reef_spartan_inner_claims: open_begin -> open_fold -> open_ipa_begin ->
// open_ipa_round x (log2(n) - 1) -> open_finish.  W, E, u, X, T and the NIFS state are read, never written.
namespace reef {

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
// a non-zero challenge below the modulus (the IPA folds with r^-1)
template <int C> static reef_status op_challenge(const reef_fe *r, bool is_mont, const char *name, fe &out) {
    REEF_TRY(sp_challenge<C>(r, is_mont, name, out));
    if (fe_is_literal_zero(fe_canon<NifsCtx<C>::F>(out))) { set_error("%s: r is zero (it has no inverse)", name); return REEF_ERR_ARG; }
    return REEF_OK;
}

// L, R of the round the vectors stand at: the cross-term MSMs over the resident gens_v key on the key ctx's stream, ordered after
// the NIFS stream's kernels by an event, with c_L q, c_R q (s->out[1], s->out[2]) added through q's nibble table.  One host wait.
template <int C> static reef_status op_cross(NifsCtx<C> *c, reef_jacobian *L, reef_jacobian *R) {
    SpartanState<C> *s = c->sp;
    Ctx<C> *key = (Ctx<C> *)s->key;
    hipStream_t ks = (hipStream_t)v_ctx_stream<C>(key);
    if (!ks) return REEF_ERR_HIP;
    REEF_HIP_TRY(hipEventRecord(c->ev, c->stream));
    REEF_HIP_TRY(hipStreamWaitEvent(ks, c->ev, 0));
    std::lock_guard<std::mutex> kl(key->mu);
    CtxScope<C> scope(key);
    REEF_TRY(scope.enter());
    const size_t k = s->w1s.size();
    return ipa_cross_run<C>(key, s->oa.template as<fe256>(), s->olen, false, k ? (const reef_fe *)s->w1s.data() : nullptr,
                            k ? (const reef_fe *)s->w2s.data() : nullptr, k, s->out.template as<fe256>() + 1, &s->q, L, R);
}
// the sums of `grid` blocks -> s->out + slot (nv values, canonical integers); no wait
template <int C> static void op_finish(NifsCtx<C> *c, u32 grid, u32 nv, u32 slot) {
    SpartanState<C> *s = c->sp;
    hipLaunchKernelGGL(k_sp_finish<NifsCtx<C>::F>, dim3(1), dim3(SP_THREADS), 0, c->stream, (const unsigned long long *)s->partial.p, grid, nv,
                       (int)SP_FORM_INTEGER, s->out.template as<fe256>() + slot);
}
// s->out[0] (a canonical integer) to the host in the caller's form
template <int C> static reef_status op_fetch(NifsCtx<C> *c, bool is_mont, reef_fe *dst) {
    constexpr int F = NifsCtx<C>::F;
    fe256 v;
    REEF_HIP_TRY(hipMemcpyAsync(&v, c->sp->out.p, sizeof v, hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    const fe256 o = fe_to_caller<F>(fe_from_integer<F>(v), is_mont);
    memcpy(dst, &o, sizeof o);
    return REEF_OK;
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
    int key_dev = 0;
    size_t key_n = 0;
    {
        std::lock_guard<std::mutex> kl(key->mu);
        key_dev = key->key->device;
        key_n = key->key->n;
    }
    if (key_dev != c->device) { set_error("reef_spartan_open_begin: the key lives on device %d, the NIFS ctx on device %d", key_dev, c->device); return REEF_ERR_ARG; }
    if (key_n != n) {
        set_error("reef_spartan_open_begin: the key holds %zu points, the opening needs exactly n = max(num_cons_pad, num_vars_pad) = %zu", key_n, n);
        return REEF_ERR_ARG;
    }
    REEF_ON_DEVICE(c->device);
    NifsScope<C> scope(c);
    REEF_TRY(scope.enter());
    s->phase = SP_NONE;                                       // a failure half way leaves nothing to continue
    REEF_TRY(s->e1.ensure(s->ncp * sizeof(fe256)));
    REEF_TRY(s->e2.ensure(s->nvp * sizeof(fe256)));
    REEF_TRY(s->oa.ensure(n * sizeof(fe256)));
    REEF_TRY(s->ob.ensure(n * sizeof(fe256)));
    REEF_TRY(s->partial.ensure(SP_BLOCKS * 27 * sizeof(unsigned long long)));
    REEF_TRY(s->out.ensure(4 * sizeof(fe256)));
    const fe256 *e1 = s->e1.template as<fe256>(), *e2 = s->e2.template as<fe256>();
    REEF_TRY(sp_eq_table(c, s->rx.data(), s->ell_x, s->e1.template as<fe256>()));
    REEF_TRY(sp_eq_table(c, s->ry.data() + 1, s->ell_y - 1, s->e2.template as<fe256>()));
    const u32 nE = (u32)std::min(c->num_cons, s->nvp), nW = (u32)std::min(c->num_vars, s->ncp);
    const u32 grid = sp_grid(std::max(nE, nW));
    hipLaunchKernelGGL(k_op_cross<F>, dim3(grid), dim3(SP_THREADS), 0, c->stream, (const fe256 *)c->E.p, e2, nE, (const fe256 *)c->z1.p, e1, nW,
                       s->partial.template as<unsigned long long>());
    op_finish(c, grid, 1, 0);
    REEF_HIP_TRY(hipGetLastError());
    REEF_TRY(op_fetch(c, is_mont, cross_term));
    s->key = key_impl;
    s->on = s->olen = n;
    s->rounds = 0;
    s->phase = SP_OPEN_BEGUN;
    return REEF_OK;
}

template <int C> static reef_status v_open_fold(void *impl, const reef_fe *r, bool is_mont, reef_fe *c_out) {
    constexpr int F = NifsCtx<C>::F;
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    fe ri;
    REEF_TRY(sp_challenge<C>(r, is_mont, "reef_spartan_open_fold", ri));
    if (!c_out) { set_error("null argument"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    REEF_TRY(op_expect(c, "reef_spartan_open_fold"));
    SpartanState<C> *s = c->sp;
    REEF_ON_DEVICE(c->device);
    NifsScope<C> scope(c);
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
    p.a = s->oa.template as<fe256>();
    p.b = s->ob.template as<fe256>();
    p.partial = s->partial.template as<unsigned long long>();
    const u32 grid = sp_grid(p.h);
    hipLaunchKernelGGL(k_op_fold<F>, dim3(grid), dim3(SP_THREADS), 0, c->stream, p);
    op_finish(c, grid, 3, 0);                                 // c, then round 0's c_L, c_R where op_cross reads them
    REEF_HIP_TRY(hipGetLastError());
    REEF_TRY(op_fetch(c, is_mont, c_out));
    s->olen = s->on;
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
    NifsScope<C> scope(c);
    REEF_TRY(scope.enter());
    s->phase = SP_NONE;
    s->q = *q;
    s->w1s.clear();
    s->w2s.clear();
    REEF_TRY(op_cross(c, L, R));
    s->rounds = 0;
    s->phase = SP_OPEN_IPA;
    return REEF_OK;
}

template <int C> static reef_status v_open_ipa_round(void *impl, const reef_fe *r, bool is_mont, reef_jacobian *L, reef_jacobian *R) {
    constexpr int F = NifsCtx<C>::F;
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    fe ri;
    REEF_TRY(op_challenge<C>(r, is_mont, "reef_spartan_open_ipa_round", ri));
    if (!L || !R) { set_error("null argument"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    REEF_TRY(op_expect(c, "reef_spartan_open_ipa_round"));
    SpartanState<C> *s = c->sp;
    REEF_ON_DEVICE(c->device);
    NifsScope<C> scope(c);
    REEF_TRY(scope.enter());
    s->phase = SP_NONE;
    const fe rinv = fe_inv<F>(ri);
    OpRound p;
    memset(&p, 0, sizeof p);
    p.a = s->oa.template as<fe256>();
    p.b = s->ob.template as<fe256>();
    p.q = (u32)(s->olen / 4);
    p.r = fe_to_table<F>(ri);
    p.rinv = fe_to_table<F>(rinv);
    p.partial = s->partial.template as<unsigned long long>();
    const u32 grid = sp_grid(p.q);
    hipLaunchKernelGGL(k_op_round<F>, dim3(grid), dim3(SP_THREADS), 0, c->stream, p);
    op_finish(c, grid, 2, 1);                                 // the next round's c_L, c_R
    REEF_HIP_TRY(hipGetLastError());
    s->olen /= 2;
    s->w1s.push_back(fe_to_integer<F>(rinv));
    s->w2s.push_back(fe_to_integer<F>(ri));
    REEF_TRY(op_cross(c, L, R));
    ++s->rounds;
    s->phase = SP_OPEN_IPA;
    return REEF_OK;
}

template <int C> static reef_status v_open_finish(void *impl, const reef_fe *r_last, bool is_mont, reef_fe *a_hat) {
    constexpr int F = NifsCtx<C>::F;
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    fe ri;
    REEF_TRY(op_challenge<C>(r_last, is_mont, "reef_spartan_open_finish", ri));
    if (!a_hat) { set_error("null argument"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    REEF_TRY(op_expect(c, "reef_spartan_open_finish"));
    SpartanState<C> *s = c->sp;
    REEF_ON_DEVICE(c->device);
    NifsScope<C> scope(c);
    REEF_TRY(scope.enter());
    s->phase = SP_NONE;
    hipLaunchKernelGGL(k_op_last<F>, dim3(1), dim3(64), 0, c->stream, s->oa.template as<fe256>(), s->ob.template as<fe256>(), fe_to_table<F>(ri),
                       fe_to_table<F>(fe_inv<F>(ri)), is_mont ? (int)SP_FORM_MONT : (int)SP_FORM_INTEGER, s->out.template as<fe256>() + 3);
    REEF_HIP_TRY(hipGetLastError());
    REEF_HIP_TRY(hipMemcpyAsync(a_hat, s->out.template as<fe256>() + 3, sizeof(fe256), hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    s->olen = 1;
    s->key = nullptr;
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
    if (count > s->olen) { set_error("reef_spartan_open_read: %zu entries asked, the vector has %zu", count, s->olen); return REEF_ERR_ARG; }
    if (!count) return REEF_OK;
    REEF_ON_DEVICE(c->device);
    NifsScope<C> scope(c);
    REEF_TRY(scope.enter());
    REEF_TRY(c->stage.ensure(count * sizeof(fe256)));
    const fe256 *src = (which == 0 ? s->oa : s->ob).template as<fe256>();
    hipLaunchKernelGGL(k_fe_export<NifsCtx<C>::F>, dim3(ceil_div(count, 256)), dim3(256), 0, c->stream, src, (u64)count, (int)(which == 0), (int)to_mont,
                       c->stage.template as<fe256>());
    REEF_HIP_TRY(hipGetLastError());
    REEF_HIP_TRY(hipMemcpyAsync(out, c->stage.p, count * sizeof(fe256), hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    return REEF_OK;
}

template <int C> OpenVTable make_open_vtable() {
    return OpenVTable{v_open_begin<C>, v_open_fold<C>, v_open_ipa_begin<C>, v_open_ipa_round<C>, v_open_finish<C>, v_open_read<C>};
}

}  // namespace reef
