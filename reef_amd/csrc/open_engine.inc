// Host side of the batched IPA opening of the final SNARK (open_kernels.inc; include/reef_msm.h 3h) on a NIFS ctx; included after
// spartan_engine.inc.  The state machine goes on from reef_spartan_inner_claims: open_begin -> open_fold -> open_ipa_begin ->
// open_ipa_round x (log2(n) - 1) -> open_finish (the order: proof_order.h).  W, E, u, X, T and the NIFS state are read, never written.
// The IPA rounds themselves are IpaRun's (ipa_engine.inc).
namespace reef {

template <int C> static reef_status v_open_begin(void *impl, void *key_impl, bool is_mont, reef_fe *cross_term) {
    constexpr int F = NifsCtx<C>::F;
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    Ctx<C> *key = (Ctx<C> *)key_impl;
    if (!key || !cross_term) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(sp_expect(c, "reef_spartan_open_begin"));
    SpartanState<C> *s = c->sp;
    const size_t n = std::max(s->ncp, s->nvp);
    size_t key_n = 0;
    REEF_TRY(key_matches(key, c->device, "reef_spartan_open_begin", "NIFS", &key_n));
    if (key_n != n) {
        set_error("reef_spartan_open_begin: the key holds %zu points, the opening needs exactly n = max(num_cons_pad, num_vars_pad) = %zu", key_n, n);
        return REEF_ERR_ARG;
    }
    REEF_TRY(call.enter(&s->phase));
    REEF_TRY(s->e1.ensure(s->ncp * sizeof(fe256)));
    REEF_TRY(s->e2.ensure(s->nvp * sizeof(fe256)));
    IpaRun<C> *ip = &s->ip;
    REEF_TRY(ipa_alloc(ip, n, c->open_n_small));
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
    return call.done(SP_OPEN_BEGUN);
}

template <int C> static reef_status v_open_fold(void *impl, const reef_fe *r, bool is_mont, reef_fe *c_out) {
    constexpr int F = NifsCtx<C>::F;
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    fe ri;
    REEF_TRY(fe_challenge<F>(r, is_mont, "reef_spartan_open_fold", ri));
    if (!c_out) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(sp_expect(c, "reef_spartan_open_fold"));
    SpartanState<C> *s = c->sp;
    REEF_TRY(call.enter(&s->phase));
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
    IpaRun<C> *ip = &s->ip;
    p.a = ip->a.template as<fe256>();
    p.b = ip->b.template as<fe256>();
    p.partial = ip->partial.template as<unsigned long long>();
    const u32 grid = sp_grid(p.h);
    hipLaunchKernelGGL(k_op_fold<F>, dim3(grid), dim3(SP_THREADS), 0, c->stream, p);
    ipa_sums(ip, c->stream, grid, 3, 0);                      // c, then round 0's c_L, c_R where ipa_cross reads them
    REEF_HIP_TRY(hipGetLastError());
    REEF_TRY(ipa_fetch(ip, c->stream, is_mont, c_out));
    ip->len = ip->n;
    return call.done(SP_OPEN_FOLDED);
}

template <int C> static reef_status v_open_ipa_begin(void *impl, const reef_affine *q, reef_jacobian *L, reef_jacobian *R) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    if (!q || !L || !R) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(sp_expect(c, "reef_spartan_open_ipa_begin"));
    SpartanState<C> *s = c->sp;
    REEF_TRY(call.enter(&s->phase));
    IpaRun<C> *ip = &s->ip;
    ip->q = *q;
    ip->w1s.clear();
    ip->w2s.clear();
    REEF_TRY(ipa_cross(ip, c->stream, c->ev, L, R));
    s->rounds = 0;
    return call.done(SP_OPEN_IPA);
}

template <int C> static reef_status v_open_ipa_round(void *impl, const reef_fe *r, bool is_mont, reef_jacobian *L, reef_jacobian *R) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    fe ri;
    REEF_TRY(fe_challenge<NifsCtx<C>::F>(r, is_mont, "reef_spartan_open_ipa_round", ri, true));
    if (!L || !R) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(sp_expect(c, "reef_spartan_open_ipa_round"));
    SpartanState<C> *s = c->sp;
    REEF_TRY(call.enter(&s->phase));
    REEF_TRY(ipa_round(&s->ip, c->stream, c->ev, ri, L, R));
    ++s->rounds;
    return call.done(SP_OPEN_IPA);
}

template <int C> static reef_status v_open_finish(void *impl, const reef_fe *r_last, bool is_mont, reef_fe *a_hat) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    fe ri;
    REEF_TRY(fe_challenge<NifsCtx<C>::F>(r_last, is_mont, "reef_spartan_open_finish", ri, true));
    if (!a_hat) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(sp_expect(c, "reef_spartan_open_finish"));
    SpartanState<C> *s = c->sp;
    REEF_TRY(call.enter(&s->phase));
    REEF_TRY(ipa_last(&s->ip, c->stream, ri, is_mont, a_hat, nullptr));
    return call.done(SP_OPEN_DONE);
}

// which: 0 a, 1 b, the first `count` of their current length
template <int C> static reef_status v_open_read(void *impl, int which, size_t count, reef_fe *out, bool to_mont) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    if (count && !out) { set_error("null argument"); return REEF_ERR_ARG; }
    if (which != 0 && which != 1) { set_error("reef_spartan_open_read: which must be 0 (a) or 1 (b)"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(sp_expect(c, "reef_spartan_open_read"));
    SpartanState<C> *s = c->sp;
    if (count > s->ip.len) { set_error("reef_spartan_open_read: %zu entries asked, the vector has %zu", count, s->ip.len); return REEF_ERR_ARG; }
    if (!count) return REEF_OK;
    REEF_TRY(call.enter());
    return ipa_read(&s->ip, c->stream, c->stage, which, count, out, to_mont);
}

// n_small (0 or a power of two: api.cpp checks) holds for the openings begun after the call; no device work
template <int C> static reef_status v_open_set_small_key(void *impl, size_t n_small) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    std::lock_guard<std::mutex> lk(c->mu);
    c->open_n_small = n_small;
    return REEF_OK;
}

template <int C> OpenVTable make_open_vtable() {
    return OpenVTable{v_open_begin<C>, v_open_fold<C>, v_open_ipa_begin<C>, v_open_ipa_round<C>, v_open_finish<C>, v_open_read<C>, v_open_set_small_key<C>};
}

}  // namespace reef
