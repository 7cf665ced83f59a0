// Host side of row N5 (the sum-checks of RelaxedR1CSSNARK::prove: spartan_kernels.inc) on a NIFS ctx; included after nifs_engine.inc,
// proof_order.h (the SP_* phases and the call order, the opening's included) and ipa_engine.inc.
// A prover-side state machine: begin -> outer_round x (ell_x - 1) -> outer_claims -> inner_begin -> inner_round x (ell_y - 1) ->
// inner_claims, with ell_x = log2(num_cons_pad), ell_y = log2(2 num_vars_pad).  The running instance is read, never written.
// Beside it, in no order and on no state of the prove: the verifier's matrix evaluations (3k: v_spartan_eval_matrices; at many points in
// one pass, 3o: v_spartan_eval_matrices_batch).
namespace reef {

template <int C> struct SpartanState {
    int phase = SP_NONE;
    u64 gen = 0;                         // the ctx's gen at begin: any later change of the matrices or the running instance voids the prove
    size_t ncp = 0, nvp = 0;             // padded sizes
    u32 ell_x = 0, ell_y = 0, rounds = 0;   // rounds: challenges taken in the current sum-check
    std::vector<fe> rx, ry;              // the challenges (internal form)
    DevBuf eq, az, bz, cz, d;            // outer tables (ncp entries); cz and E are never bound
    DevBuf abc, z;                       // inner tables (2 nvp entries)
    DevBuf pts, partial, out;            // eq factors, block sums, results
    // the batched IPA opening (open_engine.inc)
    DevBuf e1, e2;                       // eq(r_x), eq(r_y[1..])
    size_t on = 0;                       // n
    IpaRun<C> ip;                        // a, b and the rounds
};
template <int C> static void spartan_release(SpartanState<C> *s) {
    if (!s) return;
    for (DevBuf *b : {&s->eq, &s->az, &s->bz, &s->cz, &s->d, &s->abc, &s->z, &s->pts, &s->partial, &s->out, &s->e1, &s->e2}) b->release();
    s->ip.release();
    delete s;
}

static u32 sp_log2(size_t n) {
    u32 l = 0;
    while ((size_t)1 << l < n) ++l;
    return l;
}
// The call `name` (of N5 or of the opening) may come now (proof_order.h: REEF_ERR_ARG naming the next call otherwise)
template <int C> static reef_status sp_expect(NifsCtx<C> *c, const char *name) {
    SpartanState<C> *s = c->sp;
    const SpOrder o = s ? SpOrder{s->phase, s->rounds, s->ell_x, s->ell_y, sp_log2(s->on)} : SpOrder{};
    const OrderVerdict v = sp_check(name, s ? &o : nullptr, s && s->gen != c->gen);
    if (v.reset) s->phase = SP_NONE;
    if (!v.ok) { set_error("%s", v.text); return REEF_ERR_ARG; }
    return REEF_OK;
}

// one round (bind with r when bind, then the sums of the next round: nv values) -> evals (HOST) in the caller's form
template <int C, int CUBIC>
static reef_status sp_round(NifsCtx<C> *c, fe256 *const *tabs, u32 h, bool bind, const fe &r, bool is_mont, reef_fe *evals) {
    constexpr int F = NifsCtx<C>::F;
    constexpr u32 NV = CUBIC ? 3 : 2;
    SpartanState<C> *s = c->sp;
    SpRound a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < (CUBIC ? 4 : 2); ++k) a.t[k] = tabs[k];
    a.h = h;
    a.bind = bind;
    a.r = fe_to_table<F>(r);
    a.partial = s->partial.template as<unsigned long long>();
    const u32 grid = sp_grid(h);
    hipLaunchKernelGGL((k_sp_round<F, CUBIC>), dim3(grid), dim3(SP_THREADS), 0, c->stream, a);
    hipLaunchKernelGGL(k_sp_finish<F>, dim3(1), dim3(SP_THREADS), 0, c->stream, (const unsigned long long *)a.partial, grid, NV,
                       is_mont ? (int)SP_FORM_MONT : (int)SP_FORM_INTEGER, s->out.template as<fe256>());
    REEF_HIP_TRY(hipGetLastError());
    REEF_HIP_TRY(hipMemcpyAsync(evals, s->out.p, NV * sizeof(fe256), hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    return REEF_OK;
}
// dot products x . y0 (and x . y1) over n entries -> s->out + slot (nv values, `form`); no wait
template <int C> static reef_status sp_dots(NifsCtx<C> *c, const fe256 *x, const fe256 *y0, const fe256 *y1, size_t n, int form, u32 slot) {
    constexpr int F = NifsCtx<C>::F;
    SpartanState<C> *s = c->sp;
    unsigned long long *partial = s->partial.template as<unsigned long long>();
    const u32 grid = sp_grid(n);
    hipLaunchKernelGGL(k_sp_dot<F>, dim3(grid), dim3(SP_THREADS), 0, c->stream, x, y0, y1, (u32)n, partial);
    hipLaunchKernelGGL(k_sp_finish<F>, dim3(1), dim3(SP_THREADS), 0, c->stream, (const unsigned long long *)partial, grid, y1 ? 2u : 1u, form,
                       s->out.template as<fe256>() + slot);
    REEF_HIP_TRY(hipGetLastError());
    return REEF_OK;
}

// the pad rule of reef_spartan_begin, in the words of the call `name`
template <int C> static reef_status sp_check_pads(NifsCtx<C> *c, const char *name, size_t num_cons_pad, size_t num_vars_pad) {
    auto pow2 = [](size_t n) { return n >= 2 && n <= ((size_t)1 << 24) && (n & (n - 1)) == 0; };
    if (!pow2(num_cons_pad) || !pow2(num_vars_pad) || num_cons_pad < c->num_cons || num_vars_pad < c->num_vars || c->num_io >= num_vars_pad) {
        set_error("%s: need powers of two 2 <= num_cons_pad, num_vars_pad <= 2^24 with num_cons_pad >= num_cons (%zu), "
                  "num_vars_pad >= num_vars (%zu) and num_vars_pad > num_io (%zu); got %zu, %zu", name, c->num_cons, c->num_vars, c->num_io, num_cons_pad,
                  num_vars_pad);
        return REEF_ERR_ARG;
    }
    return REEF_OK;
}

template <int C>
static reef_status v_spartan_begin(void *impl, size_t num_cons_pad, size_t num_vars_pad, const reef_fe *tau, bool is_mont, reef_fe *evals) {
    constexpr int F = NifsCtx<C>::F;
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    if (!tau || !evals) { set_error("null argument"); return REEF_ERR_ARG; }
    REEF_TRY(sp_check_pads(c, "reef_spartan_begin", num_cons_pad, num_vars_pad));
    const u32 ell_x = sp_log2(num_cons_pad);
    std::vector<fe> t(ell_x);
    REEF_TRY(fe_import_all<F>(tau, ell_x, is_mont, "reef_spartan_begin", "tau", t.data()));
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    if (!c->running || !c->has[0] || !c->has[1] || !c->has[2]) {
        set_error("reef_spartan_begin: set the matrices A, B, C and the running instance first (reef_nifs_set_matrix, reef_nifs_set_running)");
        return REEF_ERR_ARG;
    }
    if (!c->sp) c->sp = new SpartanState<C>();
    SpartanState<C> *s = c->sp;
    REEF_TRY(call.enter(&s->phase));
    REEF_TRY(nifs_prepare(c));
    for (DevBuf *b : {&s->eq, &s->az, &s->bz, &s->cz, &s->d}) REEF_TRY(b->ensure(num_cons_pad * sizeof(fe256)));
    REEF_TRY(s->partial.ensure(SP_BLOCKS * 27 * sizeof(unsigned long long)));
    REEF_TRY(s->out.ensure(4 * sizeof(fe256)));
    // AZ, BZ, CZ, D by row; the padding rows stay zero
    fe256 *tabs[5] = {s->eq.template as<fe256>(), s->az.template as<fe256>(), s->bz.template as<fe256>(), s->d.template as<fe256>(),
                      s->cz.template as<fe256>()};
    for (int k = 1; k < 5; ++k) REEF_HIP_TRY(hipMemsetAsync(tabs[k], 0, num_cons_pad * sizeof(fe256), c->stream));
    NifsArgs a = nifs_args(c);
    a.out[0] = tabs[1];
    a.out[1] = tabs[2];
    a.out[2] = tabs[4];
    a.out[3] = tabs[3];
    REEF_TRY((nifs_line_pass<C, NIFS_MODE_SPARTAN>(a, c->rows, c->stream)));
    REEF_TRY(fe_eq_table<F>(c->stream, s->pts, t.data(), ell_x, tabs[0]));
    s->ncp = num_cons_pad;
    s->nvp = num_vars_pad;
    s->ell_x = ell_x;
    s->ell_y = sp_log2(2 * num_vars_pad);
    s->rounds = 0;
    s->rx.clear();
    s->ry.clear();
    s->gen = c->gen;
    REEF_TRY((sp_round<C, 1>(c, tabs, (u32)(num_cons_pad / 2), false, fe_zero(), is_mont, evals)));
    return call.done(SP_OUTER);
}

template <int C> static fe256 *const *sp_outer_tabs(SpartanState<C> *s, fe256 *(&t)[4]) {
    t[0] = s->eq.template as<fe256>();
    t[1] = s->az.template as<fe256>();
    t[2] = s->bz.template as<fe256>();
    t[3] = s->d.template as<fe256>();
    return t;
}
template <int C> static fe256 *const *sp_inner_tabs(SpartanState<C> *s, fe256 *(&t)[4]) {
    t[0] = s->abc.template as<fe256>();
    t[1] = s->z.template as<fe256>();
    t[2] = t[3] = nullptr;
    return t;
}
template <int C> static reef_status v_spartan_outer_round(void *impl, const reef_fe *r, bool is_mont, reef_fe *evals) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    fe ri;
    REEF_TRY(fe_challenge<NifsCtx<C>::F>(r, is_mont, "reef_spartan_outer_round", ri));
    if (!evals) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(sp_expect(c, "reef_spartan_outer_round"));
    SpartanState<C> *s = c->sp;
    REEF_TRY(call.enter(&s->phase));
    fe256 *t[4];
    const u32 h = (u32)(s->ncp >> (s->rounds + 2));          // pairs of the next round
    REEF_TRY((sp_round<C, 1>(c, sp_outer_tabs(s, t), h, true, ri, is_mont, evals)));
    s->rx.push_back(ri);
    ++s->rounds;
    return call.done(SP_OUTER);
}

template <int C> static reef_status v_spartan_outer_claims(void *impl, const reef_fe *r_last, bool is_mont, reef_fe *claims) {
    constexpr int F = NifsCtx<C>::F;
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    fe ri;
    REEF_TRY(fe_challenge<NifsCtx<C>::F>(r_last, is_mont, "reef_spartan_outer_claims", ri));
    if (!claims) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(sp_expect(c, "reef_spartan_outer_claims"));
    SpartanState<C> *s = c->sp;
    REEF_TRY(call.enter(&s->phase));
    const int form = is_mont ? SP_FORM_MONT : SP_FORM_INTEGER;
    fe256 *t[4];
    SpRound a;
    memset(&a, 0, sizeof a);
    a.t[0] = sp_outer_tabs(s, t)[1];                          // AZ, BZ
    a.t[1] = t[2];
    a.r = fe_to_table<F>(ri);
    hipLaunchKernelGGL(k_sp_bind_last<F>, dim3(1), dim3(64), 0, c->stream, a, 2u, form, s->out.template as<fe256>());
    REEF_HIP_TRY(hipGetLastError());
    s->rx.push_back(ri);
    REEF_TRY(fe_eq_table<F>(c->stream, s->pts, s->rx.data(), s->ell_x, s->eq.template as<fe256>()));   // eq(r_x) over the bound eq(tau): not needed any more
    REEF_TRY(sp_dots(c, s->eq.template as<fe256>(), s->cz.template as<fe256>(), c->E.template as<fe256>(), c->num_cons, form, 2));
    REEF_HIP_TRY(hipMemcpyAsync(claims, s->out.p, 4 * sizeof(fe256), hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    s->rounds = 0;
    return call.done(SP_OUTER_DONE);
}

template <int C> static reef_status v_spartan_inner_begin(void *impl, const reef_fe *r, bool is_mont, reef_fe *evals) {
    constexpr int F = NifsCtx<C>::F;
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    fe ri;
    REEF_TRY(fe_challenge<NifsCtx<C>::F>(r, is_mont, "reef_spartan_inner_begin", ri));
    if (!evals) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(sp_expect(c, "reef_spartan_inner_begin"));
    SpartanState<C> *s = c->sp;
    REEF_TRY(call.enter(&s->phase));
    REEF_TRY(nifs_segments(c, c->h_colptr, c->nz, c->cols));
    const size_t n2 = 2 * s->nvp;
    REEF_TRY(s->abc.ensure(n2 * sizeof(fe256)));
    REEF_TRY(s->z.ensure(n2 * sizeof(fe256)));
    fe256 *abc = s->abc.template as<fe256>(), *z = s->z.template as<fe256>();
    const fe256 *z1 = c->z1.template as<fe256>();
    // z = W || 0 || u || X || 0 (R1CSShape::pad [R]: column c >= num_vars moves to c + num_vars_pad - num_vars)
    REEF_HIP_TRY(hipMemsetAsync(abc, 0, n2 * sizeof(fe256), c->stream));
    REEF_HIP_TRY(hipMemsetAsync(z, 0, n2 * sizeof(fe256), c->stream));
    if (c->num_vars) REEF_HIP_TRY(hipMemcpyAsync(z, z1, c->num_vars * sizeof(fe256), hipMemcpyDeviceToDevice, c->stream));
    REEF_HIP_TRY(hipMemcpyAsync(z + s->nvp, z1 + c->num_vars, (1 + c->num_io) * sizeof(fe256), hipMemcpyDeviceToDevice, c->stream));
    // ABC by column over the CSC copy: the lines are the nz columns, "z" is eq(r_x)
    NifsArgs a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < 3; ++k) a.m[k] = NifsMat{c->colptr[k].template as<u32>(), c->cent[k].template as<uint2>(), c->cside[k].template as<fe256>()};
    a.z1 = a.z2 = s->eq.template as<fe256>();
    a.num_cons = (u32)c->nz;
    a.num_vars = (u32)c->num_vars;
    a.k254 = c->k254;
    a.long_rows = c->cols.long_rows.template as<u32>();
    a.nlong = c->cols.nlong;
    a.out[0] = abc;
    a.r1 = fe_to_table<F>(ri);
    a.r2 = fe_to_table<F>(fe_mul<F>(ri, ri));
    a.shift = (u32)(s->nvp - c->num_vars);
    REEF_TRY((nifs_line_pass<C, NIFS_MODE_ABC>(a, c->cols, c->stream)));
    fe256 *t[4];
    REEF_TRY((sp_round<C, 0>(c, sp_inner_tabs(s, t), (u32)s->nvp, false, fe_zero(), is_mont, evals)));
    s->rounds = 0;
    return call.done(SP_INNER);
}

template <int C> static reef_status v_spartan_inner_round(void *impl, const reef_fe *r, bool is_mont, reef_fe *evals) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    fe ri;
    REEF_TRY(fe_challenge<NifsCtx<C>::F>(r, is_mont, "reef_spartan_inner_round", ri));
    if (!evals) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(sp_expect(c, "reef_spartan_inner_round"));
    SpartanState<C> *s = c->sp;
    REEF_TRY(call.enter(&s->phase));
    fe256 *t[4];
    const u32 h = (u32)((2 * s->nvp) >> (s->rounds + 2));
    REEF_TRY((sp_round<C, 0>(c, sp_inner_tabs(s, t), h, true, ri, is_mont, evals)));
    s->ry.push_back(ri);
    ++s->rounds;
    return call.done(SP_INNER);
}

template <int C> static reef_status v_spartan_inner_claims(void *impl, const reef_fe *r_last, bool is_mont, reef_fe *claims) {
    constexpr int F = NifsCtx<C>::F;
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    fe ri;
    REEF_TRY(fe_challenge<NifsCtx<C>::F>(r_last, is_mont, "reef_spartan_inner_claims", ri));
    if (!claims) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(sp_expect(c, "reef_spartan_inner_claims"));
    SpartanState<C> *s = c->sp;
    REEF_TRY(call.enter(&s->phase));
    const int form = is_mont ? SP_FORM_MONT : SP_FORM_INTEGER;
    fe256 *t[4];
    SpRound a;
    memset(&a, 0, sizeof a);
    a.t[0] = sp_inner_tabs(s, t)[0];                          // ABC, z
    a.t[1] = t[1];
    a.r = fe_to_table<F>(ri);
    hipLaunchKernelGGL(k_sp_bind_last<F>, dim3(1), dim3(64), 0, c->stream, a, 2u, form, s->out.template as<fe256>());
    REEF_HIP_TRY(hipGetLastError());
    s->ry.push_back(ri);
    // eval_W = W~(r_y[1..]) over num_vars_pad entries: eq(r_y[1..]) in the eq table (ncp >= 2 entries, grown to nvp if need be)
    REEF_TRY(s->eq.ensure(s->nvp * sizeof(fe256)));
    REEF_TRY(fe_eq_table<F>(c->stream, s->pts, s->ry.data() + 1, s->ell_y - 1, s->eq.template as<fe256>()));
    if (c->num_vars) REEF_TRY(sp_dots(c, s->eq.template as<fe256>(), c->z1.template as<fe256>(), nullptr, c->num_vars, form, 2));
    else REEF_HIP_TRY(hipMemsetAsync(s->out.template as<fe256>() + 2, 0, sizeof(fe256), c->stream));
    REEF_HIP_TRY(hipMemcpyAsync(claims, s->out.p, 3 * sizeof(fe256), hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    return call.done(SP_DONE);
}

// The verifier's matrix evaluations (3k): A~, B~, C~ at (r_x, r_y) from the CSR alone -- no running instance, no prove: the phase, the
// tables and gen of a prove or an opening on this ctx are neither read nor written, and the workspace is the call's own (c->evw).
// One pass over the rows (k_sp_eval_short; long rows by k_nifs_rows_long's segments and k_sp_eval_long) and one k_sp_finish: one wait.
template <int C>
static reef_status v_spartan_eval_matrices(void *impl, size_t num_cons_pad, size_t num_vars_pad, const reef_fe *r_x, const reef_fe *r_y, bool is_mont,
                                           reef_fe *evals) {
    constexpr int F = NifsCtx<C>::F;
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    if (!r_x || !r_y || !evals) { set_error("null argument"); return REEF_ERR_ARG; }
    REEF_TRY(sp_check_pads(c, "reef_spartan_eval_matrices", num_cons_pad, num_vars_pad));
    const u32 ell_x = sp_log2(num_cons_pad), ell_y = sp_log2(2 * num_vars_pad);
    std::vector<fe> p(ell_x + ell_y);
    REEF_TRY(fe_import_all<F>(r_x, ell_x, is_mont, "reef_spartan_eval_matrices", "r_x", p.data()));
    REEF_TRY(fe_import_all<F>(r_y, ell_y, is_mont, "reef_spartan_eval_matrices", "r_y", p.data() + ell_x));
    std::vector<fe256> f(2 * p.size());                       // {1 - p_j, p_j}: r_x's factors, then r_y's
    for (size_t j = 0; j < p.size(); ++j) {
        f[2 * j] = fe_to_table<F>(fe_sub<F, 2>(fe_one<F>(), p[j]));
        f[2 * j + 1] = fe_to_table<F>(p[j]);
    }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    if (!c->has[0] || !c->has[1] || !c->has[2]) {
        set_error("reef_spartan_eval_matrices: set the matrices A, B and C first (reef_nifs_set_matrix)");
        return REEF_ERR_ARG;
    }
    REEF_TRY(call.enter());
    REEF_TRY(nifs_prepare(c));
    auto &w = c->evw;
    const u32 nblocks = (u32)ceil_div(c->num_cons, SP_THREADS), nlong = c->rows.nlong;
    REEF_TRY(w.pts.ensure(f.size() * sizeof(fe256)));
    REEF_TRY(w.ex.ensure(c->num_cons * sizeof(fe256)));        // only rows < num_cons and columns < nz are ever read: partial eq tables
    REEF_TRY(w.zy.ensure(c->nz * sizeof(fe256)));
    REEF_TRY(w.partial.ensure(((size_t)nblocks + nlong) * 27 * sizeof(unsigned long long)));   // a row per block, then a row per long row
    REEF_TRY(w.out.ensure(3 * sizeof(fe256)));
    const fe256 *pts = w.pts.template as<fe256>();
    fe256 *ex = w.ex.template as<fe256>(), *zy = w.zy.template as<fe256>();
    unsigned long long *partial = w.partial.template as<unsigned long long>();
    REEF_HIP_TRY(hipMemcpyAsync(w.pts.p, f.data(), f.size() * sizeof(fe256), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_sp_eq<F>, dim3(nblocks), dim3(256), 0, c->stream, pts, ell_x, (u32)c->num_cons, ex);
    hipLaunchKernelGGL(k_sp_eq_cols<F>, dim3(ceil_div(c->nz, 256)), dim3(256), 0, c->stream, pts + 2 * ell_x, ell_y, (u32)c->nz, (u32)c->num_vars,
                       (u32)(num_vars_pad - c->num_vars), zy);
    NifsArgs a = nifs_args(c);
    a.z1 = a.z2 = zy;
    hipLaunchKernelGGL(k_sp_eval_short<F>, dim3(nblocks), dim3(SP_THREADS), 0, c->stream, a, (const fe256 *)ex, partial);
    if (nlong) {
        const u32 *seg_row = c->rows.seg_row.template as<u32>(), *seg_first = c->rows.seg_first.template as<u32>();
        fe_limbs *part = c->rows.part.template as<fe_limbs>();
        hipLaunchKernelGGL((k_nifs_rows_long<F, NIFS_MODE_SPARTAN>), dim3(c->rows.nseg), dim3(256), 0, c->stream, a, seg_row, seg_first, part);
        hipLaunchKernelGGL(k_sp_eval_long<F>, dim3(nlong), dim3(64), 0, c->stream, a, seg_first, (const fe_limbs *)part, (const fe256 *)ex,
                           partial + (size_t)nblocks * 27);
    }
    hipLaunchKernelGGL(k_sp_finish<F>, dim3(1), dim3(SP_THREADS), 0, c->stream, (const unsigned long long *)partial, nblocks + nlong, 3u,
                       is_mont ? (int)SP_FORM_MONT : (int)SP_FORM_INTEGER, w.out.template as<fe256>());
    REEF_HIP_TRY(hipGetLastError());
    REEF_HIP_TRY(hipMemcpyAsync(evals, w.out.p, 3 * sizeof(fe256), hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));             // the one wait; f goes out of scope
    return REEF_OK;
}

// The same at m points in one pass (3o): every point's factors go up in one copy, the points are walked in groups of G whose eq tables fit
// the workspace budget (c->evb), the groups follow each other on the stream, every group writes its results into one device array of 3 m
// values, and that array comes back in one copy: one wait.  A group is four launches, six with long rows, however many points it holds
// (spartan_kernels.inc: the point or the pair of points in blockIdx.y; a group of ONE point has no pair to share entries with and takes
// the single call's row kernels in the same three places).  Its buffers are the batch's own: c->evw and c->rows.part, which the
// single call and a prove use, are not touched.
static constexpr size_t SP_BATCH_MAX = 4096;                    // 3m's limit on a batch
static constexpr size_t SP_BATCH_BUDGET = (size_t)1 << 30;      // the default budget: a choice, not a measurement (3o)
template <int C>
static reef_status v_spartan_eval_matrices_batch(void *impl, size_t num_cons_pad, size_t num_vars_pad, const reef_fe *r_x, const reef_fe *r_y, size_t m,
                                                 bool is_mont, reef_fe *evals) {
    constexpr int F = NifsCtx<C>::F;
    constexpr const char *name = "reef_spartan_eval_matrices_batch";
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    if (m == 0) return REEF_OK;
    if (m > SP_BATCH_MAX) { set_error("%s: m = %zu points, at most %zu in one call", name, m, SP_BATCH_MAX); return REEF_ERR_ARG; }
    if (!r_x || !r_y || !evals) { set_error("null argument"); return REEF_ERR_ARG; }
    REEF_TRY(sp_check_pads(c, name, num_cons_pad, num_vars_pad));
    const u32 ell_x = sp_log2(num_cons_pad), ell_y = sp_log2(2 * num_vars_pad), ell = ell_x + ell_y;
    std::vector<fe256> f(m * 2 * ell);                        // per point {1 - p_j, p_j}: r_x's factors, then r_y's
    {
        std::vector<fe> p(ell);
        char what[48];
        for (size_t t = 0; t < m; ++t) {
            snprintf(what, sizeof what, "point %zu's r_x", t);
            REEF_TRY(fe_import_all<F>(r_x + t * ell_x, ell_x, is_mont, name, what, p.data()));
            snprintf(what, sizeof what, "point %zu's r_y", t);
            REEF_TRY(fe_import_all<F>(r_y + t * ell_y, ell_y, is_mont, name, what, p.data() + ell_x));
            for (size_t j = 0; j < ell; ++j) {
                f[2 * (t * ell + j)] = fe_to_table<F>(fe_sub<F, 2>(fe_one<F>(), p[j]));
                f[2 * (t * ell + j) + 1] = fe_to_table<F>(p[j]);
            }
        }
    }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    if (!c->has[0] || !c->has[1] || !c->has[2]) {
        set_error("%s: set the matrices A, B and C first (reef_nifs_set_matrix)", name);
        return REEF_ERR_ARG;
    }
    REEF_TRY(call.enter());
    REEF_TRY(nifs_prepare(c));
    auto &w = c->evb;
    // groups: G points' tables inside the budget, an even number of them (whole pairs) when more than one; one point always goes
    const size_t per_point = (c->num_cons + c->nz) * sizeof(fe256), budget = w.budget ? w.budget : SP_BATCH_BUDGET;
    size_t G = std::max<size_t>(1, budget / per_point);
    if (G > 1) G &= ~(size_t)1;
    G = std::min(G, m);
    const u32 nblocks = (u32)ceil_div(c->num_cons, SP_THREADS), nlong = c->rows.nlong, nseg = c->rows.nseg, rows = nblocks + nlong;
    if (w.tab.cap > std::max(budget, per_point)) w.tab.release();   // a budget lowered since the workspace was made
    REEF_TRY(w.tab.ensure_exact(G * per_point));
    REEF_TRY(w.pts.ensure(f.size() * sizeof(fe256)));
    REEF_TRY(w.partial.ensure(G * rows * 27 * sizeof(unsigned long long)));
    REEF_TRY(w.part.ensure(std::max<size_t>(1, (G + 1) / 2 * nseg) * 6 * sizeof(fe_limbs)));
    REEF_TRY(w.out.ensure(3 * m * sizeof(fe256)));
    REEF_HIP_TRY(hipMemcpyAsync(w.pts.p, f.data(), f.size() * sizeof(fe256), hipMemcpyHostToDevice, c->stream));
    NifsArgs a = nifs_args(c);
    a.z1 = a.z2 = nullptr;                                    // the column tables come with the pair (SpBatch)
    const u32 *seg_row = c->rows.seg_row.template as<u32>(), *seg_first = c->rows.seg_first.template as<u32>();
    const int form = is_mont ? (int)SP_FORM_MONT : (int)SP_FORM_INTEGER;
    size_t ngroups = 0;
    for (size_t first = 0; first < m; first += G, ++ngroups) {
        const u32 np = (u32)std::min(G, m - first), pairs = (np + 1) / 2;
        SpBatch g;
        g.f = w.pts.template as<fe256>() + first * 2 * ell;
        g.ex = w.tab.template as<fe256>();
        g.zy = g.ex + G * c->num_cons;
        g.partial = w.partial.template as<unsigned long long>();
        g.part = w.part.template as<fe_limbs>();
        g.npts = np;
        g.fstride = 2 * ell;
        g.ell_x = ell_x;
        g.ell_y = ell_y;
        g.nz = (u32)c->nz;
        g.rows = rows;
        g.nseg = nseg;
        hipLaunchKernelGGL(k_sp_eq_batch<F>, dim3(nblocks, np), dim3(256), 0, c->stream, g, (u32)c->num_cons);
        hipLaunchKernelGGL(k_sp_eq_cols_batch<F>, dim3(ceil_div(c->nz, 256), np), dim3(256), 0, c->stream, g, (u32)c->num_vars,
                           (u32)(num_vars_pad - c->num_vars));
        if (np == 1) {                                        // a group of one: the single call's row kernels on the batch's buffers, launch for launch
            NifsArgs a1 = a;
            a1.z1 = a1.z2 = g.zy;
            hipLaunchKernelGGL(k_sp_eval_short<F>, dim3(nblocks), dim3(SP_THREADS), 0, c->stream, a1, (const fe256 *)g.ex, g.partial);
            if (nlong) {
                hipLaunchKernelGGL((k_nifs_rows_long<F, NIFS_MODE_SPARTAN>), dim3(nseg), dim3(256), 0, c->stream, a1, seg_row, seg_first, g.part);
                hipLaunchKernelGGL(k_sp_eval_long<F>, dim3(nlong), dim3(64), 0, c->stream, a1, seg_first, (const fe_limbs *)g.part, (const fe256 *)g.ex,
                                   g.partial + (size_t)nblocks * 27);
            }
        } else {
            hipLaunchKernelGGL(k_sp_eval_short_pair<F>, dim3(nblocks, pairs), dim3(SP_THREADS), 0, c->stream, a, g);
            if (nlong) {
                hipLaunchKernelGGL(k_sp_rows_long_pair<F>, dim3(nseg, pairs), dim3(256), 0, c->stream, a, seg_row, seg_first, g);
                hipLaunchKernelGGL(k_sp_eval_long_pair<F>, dim3(nlong, pairs), dim3(64), 0, c->stream, a, seg_first, g);
            }
        }
        hipLaunchKernelGGL(k_sp_finish_batch<F>, dim3(np), dim3(SP_THREADS), 0, c->stream, (const unsigned long long *)g.partial, rows, form,
                           w.out.template as<fe256>() + 3 * first);
        REEF_HIP_TRY(hipGetLastError());
    }
    REEF_HIP_TRY(hipMemcpyAsync(evals, w.out.p, 3 * m * sizeof(fe256), hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));             // the one wait; f goes out of scope
    w.groups = ngroups;
    w.per_group = G;
    return REEF_OK;
}
template <int C> static reef_status v_spartan_set_eval_workspace(void *impl, size_t bytes) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    std::lock_guard<std::mutex> lk(c->mu);
    c->evb.budget = bytes;
    return REEF_OK;
}
template <int C> static reef_status v_spartan_eval_batch_last_info(void *impl, size_t *groups, size_t *points_per_group, size_t *workspace_bytes) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->evb.groups) { set_error("reef_spartan_eval_matrices_batch_last_info: no batch has run on this ctx"); return REEF_ERR_ARG; }
    if (groups) *groups = c->evb.groups;
    if (points_per_group) *points_per_group = c->evb.per_group;
    if (workspace_bytes) *workspace_bytes = c->evb.tab.cap;
    return REEF_OK;
}

template <int C> SpartanVTable make_spartan_vtable() {
    return SpartanVTable{v_spartan_begin<C>, v_spartan_outer_round<C>, v_spartan_outer_claims<C>, v_spartan_inner_begin<C>, v_spartan_inner_round<C>,
                         v_spartan_inner_claims<C>, v_spartan_eval_matrices<C>, v_spartan_eval_matrices_batch<C>, v_spartan_set_eval_workspace<C>,
                         v_spartan_eval_batch_last_info<C>};
}

}  // namespace reef
