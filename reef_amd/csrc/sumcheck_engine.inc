// Host side of the sum-check vector kernels (row N2); included after engine.inc.  What a call decides -- switches, grids, row lists, the
// route of a round -- is sumcheck_plan.h's, pure and tested on the host; this file holds the ctx, the launches and the state changes.
#include "sumcheck_plan.h"
namespace reef {

template <int C> struct ScCtx : DeviceCtx {   // device: where the tables live; no event
    static constexpr int F = 1 - C;      // scalar field of curve C
    size_t len = 0;                      // 2^ell entries per table
    size_t valid_t = 0, valid_e = 0;     // live entries of T / EQ: len after a set / reset / gen_eq, pow after a fold (a fold writes [0, pow) only)
    DevBuf r1acc;                        // R1_GROUPS x R1_SLOTS accumulators of the rank-one / structured sums kernels: zero between rounds (k_sc_r1_final)
    DevBuf T, T0, E, partial, out3, stage, fac, qs, misc;   // T0: pristine copy of T (a fold consumes T)
    u32 nblocks = 0;
    bool fresh = false;                  // T has not been folded since it was set / reset: its content is T0
    bool has_table = false;              // T0 holds a table: reef_sc_set_table(ctx, 0, ..) or reef_sc_set_table_parts has run
    DevBuf lk;                           // reef_sc_lookup: the indices, then the answers of a host caller
    // EQ as gen_eq_table made it and the folds left it: FH (x) FL + point masses, never written out while the rounds fold FH
    // bits (sumcheck_kernels.inc, "rank-one").  fac holds FH (2^r1_hi0 entries, folded in place) followed by FL.
    bool r1 = false;
    u32 r1_lo = 0, r1_hi = 0, r1_hi0 = 0;    // column bits, FH bits still unfolded, FH bits at the start
    u32 r1_nq = 0;
    DevBuf r1rows, r1mq, r1mw;           // row factors of the next sums (3 x 2^(r1_hi - 1) fe_limbs), masses (index, weight)
    size_t r1_prev_pow = 0;              // out3 (device) holds the coefficients of the round with this pow, tables untouched since (0: no)
    // structure of the pristine table (sumcheck_kernels.inc, "a pristine table with structure"): row classes for the matrix
    // view of gen_eq_table's split (2^(ell - ell/2) rows), the 4-byte copy of its entries, the row lists of round one
    bool st_ok = false;
    DevBuf st_s32, st_flags, st_lists, st_k, st_sumfl;   // st_k: KA, KC (fe_limbs) and the S masks of the first fold
    ScRowLists st;                       // the row lists of round one and of the first fold, deferred or not (sumcheck_plan.h): stretches of st_lists
    bool defer_on = false;               // the rows of st.f8x have not been written: the next call is their second fold, or they are flushed
    fe256 defer_r1 = {};
    size_t defer_pow = 0;                // the pow of that next call
    u32 defer_hq = 0;
    fe256 parts_fill[2 * SC_MAX_PARTS] = {};   // reef_sc_set_table_parts: the FILL values (integer, table form) on their way to the device
    fe256 *pinned3 = nullptr;            // pinned host landing zone for the three coefficients
    // gen_eq_table's inputs (last_q, rs, qs) go through pinned staging in ONE asynchronous copy: two halves used in turn, each
    // with the event of its last copy (a half is reused two calls later; a step's own rounds have long waited for the stream by then)
    unsigned char *pin_in = nullptr;
    size_t pin_in_cap = 0;               // bytes per half
    hipEvent_t pin_ev[2] = {nullptr, nullptr};
    int pin_next = 0;
    DevBuf gacc;                         // 27 limb totals + the ticket counter of the one-launch rounds (zero between rounds)
    u32 seq = 0;                         // sequence number of the last one-launch round (the kernel posts it after the coefficients)
    // The tuning switches (environment) are read when the ctx is created, when a table is set and when a step starts
    // (gen_eq_table) -- never per round: a step runs under ONE setting, and no getenv sits on the per-round path (ADVICE r3).
    ScSwitches sw;
};
// sumcheck_plan.h has what each switch means and its bounds; this is the one place of row N2 that reads the environment.
template <int C> static void sc_read_switches(ScCtx<C> *c) {
    ScSwitchText t = {};
    t.one_launch = exp_env("REEF_SC_ONE_LAUNCH");
    t.rank1 = exp_env("REEF_SC_RANK1");
    t.structured = exp_env("REEF_SC_STRUCT");
    t.identity = exp_env("REEF_SC_IDENTITY");
    t.defer = exp_env("REEF_SC_DEFER");
    t.r1_min_pow = exp_env("REEF_SC_RANK1_MIN_POW");
    t.floor_blocks = exp_env("REEF_SC_FLOOR");
    t.one_launch_max = exp_env("REEF_SC_ONE_LAUNCH_MAX");
    t.split_max = exp_env("REEF_SC_SPLIT_MAX");
    t.split_blocks = exp_env("REEF_SC_SPLIT_BLOCKS");
    t.items = exp_env("REEF_SC_ITEMS");
    t.order = getenv("REEF_SC_FENCE");
    t.set_sub = exp_env("REEF_SC_SET_SUB");
    t.blocks_cap = exp_env("REEF_SC_BLOCKS");
    c->sw = sc_parse_switches(t);
}
// what the decisions of a round read of the ctx
template <int C> static ScState sc_state(const ScCtx<C> *c) {
    ScState s;
    s.len = c->len; s.valid_t = c->valid_t; s.valid_e = c->valid_e; s.nblocks = c->nblocks;
    s.r1 = c->r1; s.r1_hi = c->r1_hi; s.r1_hi0 = c->r1_hi0; s.r1_lo = c->r1_lo; s.r1_nq = c->r1_nq; s.r1_prev_pow = c->r1_prev_pow;
    s.fresh = c->fresh; s.st_ok = c->st_ok; s.defer_on = c->defer_on; s.defer_pow = c->defer_pow; s.defer_hq = c->defer_hq;
    s.st = c->st;
    return s;
}
static inline dim3 sc_dim3(ScGrid g) { return dim3(g.x, g.y); }

template <int C> static void sc_free(ScCtx<C> *c) {
    if (!c) return;
    retire_device_ctx(c);
    for (DevBuf *b : {&c->T, &c->T0, &c->E, &c->partial, &c->out3, &c->stage, &c->fac, &c->qs, &c->misc, &c->r1rows, &c->r1mq, &c->r1mw, &c->gacc, &c->st_s32, &c->st_flags, &c->st_lists, &c->st_k, &c->st_sumfl, &c->r1acc, &c->lk}) b->release();
    if (c->pinned3) (void)hipHostFree(c->pinned3);
    if (c->pin_in) (void)hipHostFree(c->pin_in);
    for (auto &e : c->pin_ev) if (e) (void)hipEventDestroy(e);
    delete c;
}

// A sum-check ctx takes a pool stream when a call finds it idle and stays on it through the rounds of a step (they hand their
// results over through polled memory, not through a wait for the stream); the calls that end with a wait for the stream --
// set_table, gen_eq_table, read, sync -- let it go again if the stream has nothing left (common.h: OnExit::RELEASE_IF_IDLE / STAY).

template <int C> static reef_status v_sc_create(void **impl, size_t len) {
    if (!impl || len == 0 || (len & (len - 1)) || len > (1ull << 28)) { set_error("table length must be a power of two <= 2^28"); return REEF_ERR_ARG; }
    int device = 0;                      // the tables live on the caller's current device
    if (hipGetDevice(&device) != hipSuccess) { set_error("hipGetDevice failed"); return REEF_ERR_HIP; }
    return create_device_ctx<ScCtx<C>>(impl, device, "reef_sc_create", false, sc_free<C>, [&](ScCtx<C> *c) -> reef_status {
        sc_read_switches<C>(c);
        c->len = len;
        c->valid_t = c->valid_e = len;
        REEF_TRY(c->lease.enter(c->device, &c->stream));
        c->nblocks = sc_nblocks(len, c->sw.blocks_cap);
        for (DevBuf *b : {&c->T, &c->T0, &c->E}) REEF_TRY(b->ensure(len * sizeof(fe256)));
        REEF_TRY(c->partial.ensure((size_t)c->nblocks * 27 * sizeof(u64)));
        REEF_TRY(c->out3.ensure(3 * sizeof(fe256)));
        const hipError_t e = hipHostMalloc((void **)&c->pinned3, 4 * sizeof(fe256), hipHostMallocDefault);
        if (e != hipSuccess) { set_error("hipHostMalloc: %s", hipGetErrorString(e)); return REEF_ERR_HIP; }
        memset(c->pinned3, 0, 4 * sizeof(fe256));
        REEF_TRY(c->gacc.ensure(28 * sizeof(u64)));
        REEF_TRY(c->r1acc.ensure(R1_GROUPS * R1_SLOTS * sizeof(u64)));
        if (hipMemsetAsync(c->r1acc.p, 0, R1_GROUPS * R1_SLOTS * sizeof(u64), c->stream) != hipSuccess ||
            hipMemsetAsync(c->gacc.p, 0, 28 * sizeof(u64), c->stream) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
            set_error("hipMemset failed");
            return REEF_ERR_HIP;
        }
        c->lease.idle();                     // waited for above: the ctx takes a stream again when its first call comes
        return REEF_OK;
    });
}
template <int C> static void v_sc_destroy(void *impl) { sc_free((ScCtx<C> *)impl); }

// The kernel posts the call's sequence number (c->seq) to pinned memory after the coefficients: poll briefly (a round that is
// still streaming gigabytes is waited for the ordinary way), 12 -> 6.6 us per launch-and-wait.
template <int C> static reef_status sc_wait_posted(ScCtx<C> *c) {
    REEF_HIP_TRY(hipGetLastError());
    volatile u32 *flag = reinterpret_cast<volatile u32 *>(c->pinned3 + 3);
    const auto t0 = std::chrono::steady_clock::now();
    u32 spins = 0;
    while (*flag != c->seq) {
        if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(200)) break;
    }
    if (*flag != c->seq) REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    if (*flag != c->seq) { set_error("sum-check round did not post its result"); return REEF_ERR_HIP; }
    return REEF_OK;
}
// the dense sums kernels were launched with `blocks` blocks; hand the coefficients to the caller
template <int C> static reef_status sc_dense_finish(ScCtx<C> *c, bool one, u32 blocks, reef_fe *out3_host) {
    if (!one)                              // more than a few blocks: a second kernel adds their sums up and posts the result like the one-launch rounds do
        hipLaunchKernelGGL(k_sc_coeffs_final<ScCtx<C>::F>, dim3(1), dim3(1024), 0, c->stream, c->partial.template as<unsigned long long>(), blocks,
                           c->pinned3, ++c->seq);
    REEF_HIP_TRY(hipGetLastError());
    REEF_TRY(sc_wait_posted<C>(c));
    memcpy(out3_host, c->pinned3, 3 * sizeof(fe256));
    return REEF_OK;
}

// ---- rank-one EQ ----
template <int C> struct R1View {
    fe256 *fh, *fl;
    fe_limbs *f0, *f1, *fd;
    explicit R1View(ScCtx<C> *c) {
        fh = c->fac.template as<fe256>();
        fl = fh + ((size_t)1 << c->r1_hi0);
        const size_t half = c->r1_hi0 ? (size_t)1 << (c->r1_hi0 - 1) : 1;
        f0 = c->r1rows.template as<fe_limbs>();
        f1 = f0 + half;
        fd = f1 + half;
    }
};
// EQ written out where the dense kernels expect it (the live 2^(r1_hi + r1_lo) entries); leaves rank-one mode unless `keep`
template <int C> static reef_status sc_r1_materialize(ScCtx<C> *c, bool keep = false) {
    constexpr int F = ScCtx<C>::F;
    const R1View<C> v(c);
    const u32 ell_cur = c->r1_hi + c->r1_lo;
    const size_t n = (size_t)1 << ell_cur;
    hipLaunchKernelGGL(k_sc_eq_table<F>, dim3(sc_fold_blocks(n)), dim3(256), 0, c->stream, (const fe256 *)v.fh,
                       (const fe256 *)v.fl, ell_cur, c->r1_lo, c->E.template as<fe256>());
    if (c->r1_nq)
        hipLaunchKernelGGL(k_sc_r1_masses<F>, dim3(ceil_div(c->r1_nq, 256)), dim3(256), 0, c->stream, (const u32 *)c->r1mq.template as<u32>(),
                           (const fe256 *)c->r1mw.template as<fe256>(), c->r1_nq, c->E.template as<fe256>());
    REEF_HIP_TRY(hipGetLastError());
    if (!keep) c->r1 = false;
    return REEF_OK;
}
// FH folded with r (or not: r == nullptr), masses moved, row factors of the next sums tabulated; hc = FH rows before
template <int C> static reef_status sc_r1_prep(ScCtx<C> *c, const fe256 *r, size_t pow) {
    constexpr int F = ScCtx<C>::F;
    const R1View<C> v(c);
    const u32 hc = 1u << c->r1_hi;
    const u32 rows_after = r ? hc >> 1 : hc;
    const u32 hn_next = rows_after >> 1;
    fe256 rr = {};
    if (r) rr = *r;
    hipLaunchKernelGGL(k_sc_r1_prep<F>, dim3(sc_r1_prep_blocks(c->r1_hi, r != nullptr, c->r1_nq)), dim3(256), 0, c->stream, v.fh, hc, r ? 1 : 0, rr, hn_next, v.f0, v.f1, v.fd,
                       c->r1mq.template as<u32>(), c->r1mw.template as<fe256>(), c->r1_nq, (u32)pow);
    REEF_HIP_TRY(hipGetLastError());
    if (r) c->r1_hi -= 1;
    return REEF_OK;
}
// the sums kernels of a rank-one round have left their limb sums in r1acc; hand the coefficients of the round with `pow` to the caller
template <int C> static reef_status sc_r1_finish(ScCtx<C> *c, size_t pow, reef_fe *out3_host, const fe256 *ident_r = nullptr) {
    constexpr int F = ScCtx<C>::F;
    fe256 rr = {};
    if (ident_r) rr = *ident_r;
    hipLaunchKernelGGL(k_sc_r1_final<F>, dim3(1), dim3(1024), 0, c->stream, c->r1acc.template as<unsigned long long>(),
                       (const fe256 *)(c->fresh ? c->T0 : c->T).template as<fe256>(), (u32)pow, (const u32 *)c->r1mq.template as<u32>(),
                       (const fe256 *)c->r1mw.template as<fe256>(), c->r1_nq, ident_r ? 1 : 0, rr, c->out3.template as<fe256>(), c->pinned3, ++c->seq);
    c->r1_prev_pow = pow;
    REEF_TRY(sc_wait_posted<C>(c));
    memcpy(out3_host, c->pinned3, 3 * sizeof(fe256));
    return REEF_OK;
}

// The row structure of the table just set, in three parts: sc_struct_open decides whether this table gets one (only tables the
// rank-one rounds serve) and presets the row flags, a kernel clears them and writes the 4-byte copy -- k_sc_classify from the caller's
// integers (reef_sc_set_table), k_sc_set_parts while it writes the table (reef_sc_set_table_parts) -- and sc_struct_lists builds the
// row lists of round one from the flags.  The structure is only kept when at least half the rows are K or S.
template <int C> static reef_status sc_struct_open(ScCtx<C> *c, u32 *lo_bits, u32 *rows) {
    c->st_ok = false;
    c->defer_on = false;                 // the table is replaced
    *rows = 0;
    sc_read_switches<C>(c);
    *lo_bits = sc_lo_bits(c->len);
    const u32 H = sc_struct_rows(c->len, c->sw);
    if (!H) return REEF_OK;
    REEF_TRY(c->st_s32.ensure(c->len * sizeof(u32)));
    REEF_TRY(c->st_flags.ensure((size_t)H * sizeof(u32)));
    {
        std::vector<u32> three(H, 3u);
        REEF_HIP_TRY(hipMemcpyAsync(c->st_flags.p, three.data(), (size_t)H * sizeof(u32), hipMemcpyHostToDevice, c->stream));
        REEF_HIP_TRY(hipStreamSynchronize(c->stream));     // `three` is a local
    }
    *rows = H;
    return REEF_OK;
}
template <int C> static reef_status sc_struct_lists(ScCtx<C> *c, u32 H) {
    std::vector<u32> flags(H);
    REEF_HIP_TRY(hipMemcpyAsync(flags.data(), c->st_flags.p, (size_t)H * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<u32> lists;
    if (!sc_build_row_lists(flags.data(), H, &c->st, &lists)) return REEF_OK;
    const u32 hq = H / 4;
    REEF_TRY(c->st_lists.ensure(lists.size() * sizeof(u32)));
    REEF_HIP_TRY(hipMemcpyAsync(c->st_lists.p, lists.data(), lists.size() * sizeof(u32), hipMemcpyHostToDevice, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    REEF_TRY(c->st_k.ensure((size_t)hq * (11 * sizeof(fe_limbs) + sizeof(u32)) + 64));   // KA, KC, masks; K2A, K2C and the 2 x 4 scaled factor rows of the deferred fold
    REEF_TRY(c->st_sumfl.ensure(sizeof(fe256)));
    c->st_ok = true;
    return REEF_OK;
}
// reef_sc_set_table: `src_int` are the caller's integers on the device, n of them, zero beyond
template <int C> static reef_status sc_struct_build(ScCtx<C> *c, const fe256 *src_int, size_t n) {
    u32 lo = 0, H = 0;
    REEF_TRY(sc_struct_open<C>(c, &lo, &H));
    if (!H) return REEF_OK;
    hipLaunchKernelGGL(k_sc_classify, dim3(ceil_div(c->len, 256)), dim3(256), 0, c->stream, src_int, (u32)n, (u32)c->len, lo, c->st_flags.template as<u32>(),
                       c->st_s32.template as<u32>());
    REEF_HIP_TRY(hipGetLastError());
    return sc_struct_lists<C>(c, H);
}
// k_sc_r1_fold_coeffs_cs (any of its forms) over one row list: the rows' fold from their 4-byte sources and their share of the next
// sums; hn: pair rows after the fold, which KA, KC and the S masks in st_k are laid out by
template <int C, class K>
static void sc_launch_cs(ScCtx<C> *c, const R1View<C> &v, K kernel, ScGrid g, u32 hn, const ScList &L, const fe256 &r, unsigned long long *out) {
    fe_limbs *ka = c->st_k.template as<fe_limbs>(), *kc = ka + hn;
    u32 *smask = reinterpret_cast<u32 *>(kc + hn);
    hipLaunchKernelGGL(kernel, sc_dim3(g), dim3(256), 0, c->stream, (const u32 *)c->st_s32.template as<u32>(), c->T.template as<fe256>(), c->r1_lo, hn,
                       c->st_lists.template as<u32>() + L.off, L.n, r, (const fe_limbs *)ka, (const fe_limbs *)kc, (const u32 *)smask, (const fe_limbs *)v.f0,
                       (const fe_limbs *)v.f1, (const fe_limbs *)v.fd, (const fe256 *)v.fl, out);
}

// The deferred first fold (k_sc_r1_fold_coeffs_cs<.., WRITE = false>) written out after all: any call that is not the second fold
// of the step finds the table as if nothing had been deferred.  The sums the kernel leaves go to scratch.
template <int C> static reef_status sc_defer_flush(ScCtx<C> *c) {
    if (!c->defer_on) return REEF_OK;
    c->defer_on = false;
    const R1View<C> v(c);
    REEF_TRY(c->stage.ensure((size_t)R1_GROUPS * R1_SLOTS * sizeof(u64)));   // scratch accumulators: nobody reads these sums
    sc_launch_cs<C>(c, v, k_sc_r1_fold_coeffs_cs<ScCtx<C>::F, true, true>, sc_list_grid(c->r1_lo, c->st.f8x.n), c->defer_hq, c->st.f8x, c->defer_r1,
                    c->stage.template as<unsigned long long>());
    REEF_HIP_TRY(hipGetLastError());
    return REEF_OK;
}

// which: 0 = T, 1 = EQ.  Integers in, zero-padded to the table length (the "nldoc" padding of
// r1cs.rs:2323-2330).
template <int C> static reef_status v_sc_set(void *impl, int which, const reef_fe *vals, size_t n, int loc) {
    ScCtx<C> *c = (ScCtx<C> *)impl;
    if (!c || (n && !vals) || n > c->len || which < 0 || which > 1) { set_error("bad argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::RELEASE_IF_IDLE);
    REEF_TRY(call.enter());
    if (which == 1) REEF_TRY(sc_defer_flush<C>(c));
    else c->defer_on = false;               // T is replaced
    (which == 0 ? c->valid_t : c->valid_e) = c->len;
    c->r1_prev_pow = 0;
    // whatever an earlier round left in the shared accumulators (a round that failed between its sums and its final kernel) is gone
    REEF_HIP_TRY(hipMemsetAsync(c->gacc.p, 0, 28 * sizeof(u64), c->stream));
    REEF_HIP_TRY(hipMemsetAsync(c->r1acc.p, 0, R1_GROUPS * R1_SLOTS * sizeof(u64), c->stream));
    fe256 *dst = (which == 0 ? c->T0 : c->E).template as<fe256>();   // the table goes to its pristine copy; folds write T
    const fe256 *src = (const fe256 *)vals;
    if (loc != REEF_DEVICE && n) {
        REEF_TRY(c->stage.ensure(n * sizeof(fe256)));
        REEF_HIP_TRY(hipMemcpyAsync(c->stage.p, vals, n * sizeof(fe256), hipMemcpyHostToDevice, c->stream));
        src = c->stage.template as<fe256>();
    }
    if (n) hipLaunchKernelGGL(k_fe_import<ScCtx<C>::F>, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, src, (u64)n, 0, dst);
    if (n < c->len) REEF_HIP_TRY(hipMemsetAsync(dst + n, 0, (c->len - n) * sizeof(fe256), c->stream));
    if (which == 0) c->fresh = c->has_table = true;
    else c->r1 = false;                  // a table given by the caller is a dense table
    REEF_HIP_TRY(hipGetLastError());
    if (which == 0) REEF_TRY(sc_struct_build<C>(c, src, n));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    return REEF_OK;
}

// T from parts (include/reef_msm.h 3b): field elements, one value repeated, document symbols -- what the caller knows the table to be,
// not 32 bytes per entry.  Host parts are staged packed (count x element size, every part's start padded to 32 bytes; a FILL is two
// fe256: its integer and its table form); k_sc_set_parts writes T0, the 4-byte copy and the row flags in one pass.  Ends in the
// state v_sc_set(which = 0) leaves for the same values.
template <int C> static reef_status v_sc_set_parts(void *impl, const reef_sc_part *parts, size_t nparts) {
    static_assert(REEF_SC_MAX_PARTS == SC_MAX_PARTS && REEF_SC_PART_FE == SC_PART_FE && REEF_SC_PART_SYMBOLS == SC_PART_SYMBOLS && REEF_SC_PART_FILL == SC_PART_FILL,
                  "the header's part kinds are the kernel's");
    ScCtx<C> *c = (ScCtx<C> *)impl;
    if (!c) { set_error("null argument"); return REEF_ERR_ARG; }
    if (nparts > REEF_SC_MAX_PARTS) { set_error("reef_sc_set_table_parts: %zu parts, at most %d", nparts, (int)REEF_SC_MAX_PARTS); return REEF_ERR_ARG; }
    if (nparts && !parts) { set_error("reef_sc_set_table_parts: parts is NULL"); return REEF_ERR_ARG; }
    size_t total = 0, stage_bytes = 0, at[REEF_SC_MAX_PARTS] = {};      // at[p]: where part p is staged
    for (size_t p = 0; p < nparts; ++p) {
        const reef_sc_part &q = parts[p];
        if (q.kind != REEF_SC_PART_FE && q.kind != REEF_SC_PART_SYMBOLS && q.kind != REEF_SC_PART_FILL) {
            set_error("reef_sc_set_table_parts: part %zu has the unknown kind %u", p, q.kind);
            return REEF_ERR_ARG;
        }
        if (q.kind == REEF_SC_PART_SYMBOLS && q.elem_bytes != 1 && q.elem_bytes != 2 && q.elem_bytes != 4) {
            set_error("reef_sc_set_table_parts: part %zu has symbols of %u bytes (1, 2 or 4)", p, q.elem_bytes);
            return REEF_ERR_ARG;
        }
        if (q.count && !q.data) { set_error("reef_sc_set_table_parts: part %zu has %zu entries and no data", p, q.count); return REEF_ERR_ARG; }
        const bool on_device = q.kind != REEF_SC_PART_FILL && q.loc == REEF_DEVICE;
        if (q.count && on_device && q.kind == REEF_SC_PART_SYMBOLS && reinterpret_cast<uintptr_t>(q.data) % q.elem_bytes) {
            set_error("reef_sc_set_table_parts: part %zu: device symbols of %u bytes at an address that is no multiple of it", p, q.elem_bytes);
            return REEF_ERR_ARG;
        }
        if (q.count > c->len - total) { set_error("reef_sc_set_table_parts: the parts hold more than the table's %zu entries", c->len); return REEF_ERR_ARG; }
        total += q.count;
        if (q.count && !on_device) {
            at[p] = stage_bytes;
            const size_t bytes = q.kind == REEF_SC_PART_FILL ? 2 * sizeof(fe256) : q.count * (q.kind == REEF_SC_PART_FE ? sizeof(fe256) : (size_t)q.elem_bytes);
            stage_bytes += (bytes + 31) & ~(size_t)31;
        }
    }
    DeviceCall call(c, OnExit::RELEASE_IF_IDLE);
    REEF_TRY(call.enter());
    c->defer_on = false;                    // T is replaced
    c->valid_t = c->len;
    c->r1_prev_pow = 0;
    REEF_HIP_TRY(hipMemsetAsync(c->gacc.p, 0, 28 * sizeof(u64), c->stream));       // as v_sc_set
    REEF_HIP_TRY(hipMemsetAsync(c->r1acc.p, 0, R1_GROUPS * R1_SLOTS * sizeof(u64), c->stream));
    if (stage_bytes) REEF_TRY(c->stage.ensure(stage_bytes));
    ScPartsArg a = {};
    size_t start = 0;
    for (size_t p = 0; p < SC_MAX_PARTS; ++p) {
        a.start[p] = (u32)start;
        if (p >= nparts || !parts[p].count) continue;
        const reef_sc_part &q = parts[p];
        a.kind_eb[p] = q.kind | (q.kind == REEF_SC_PART_SYMBOLS ? q.elem_bytes << 8 : 0u);
        start += q.count;
        if (q.kind != REEF_SC_PART_FILL && q.loc == REEF_DEVICE) { a.ptr[p] = (const unsigned char *)q.data; continue; }
        unsigned char *dst = c->stage.template as<unsigned char>() + at[p];
        a.ptr[p] = dst;
        if (q.kind == REEF_SC_PART_FILL) {
            fe256 *pair = c->parts_fill + 2 * p;                                    // lives in the ctx: the copy reads it after this loop
            memcpy(&pair[0], q.data, sizeof(fe256));
            pair[1] = fe_to_table<ScCtx<C>::F>(fe_from_caller<ScCtx<C>::F>(pair[0], false));
            REEF_HIP_TRY(hipMemcpyAsync(dst, pair, 2 * sizeof(fe256), hipMemcpyHostToDevice, c->stream));
        } else {
            const size_t bytes = q.count * (q.kind == REEF_SC_PART_FE ? sizeof(fe256) : (size_t)q.elem_bytes);
            REEF_HIP_TRY(hipMemcpyAsync(dst, q.data, bytes, hipMemcpyHostToDevice, c->stream));
        }
    }
    a.start[SC_MAX_PARTS] = (u32)start;
    u32 lo = 0, H = 0;
    REEF_TRY(sc_struct_open<C>(c, &lo, &H));
    u32 sub = 0;
    const u32 blocks = sc_set_parts_blocks(c->len, c->sw, &sub);
    hipLaunchKernelGGL(k_sc_set_parts<ScCtx<C>::F>, dim3(blocks), dim3(256), 0, c->stream, a, (u32)c->len, lo, sub,
                       c->T0.template as<fe256>(), H ? c->st_flags.template as<u32>() : nullptr, H ? c->st_s32.template as<u32>() : nullptr);
    REEF_HIP_TRY(hipGetLastError());
    c->fresh = c->has_table = true;
    if (H) REEF_TRY(sc_struct_lists<C>(c, H));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    return REEF_OK;
}

template <int C> static reef_status v_sc_read(void *impl, int which, size_t count, reef_fe *out_host) {
    ScCtx<C> *c = (ScCtx<C> *)impl;
    if (!c || !out_host || count > c->len || which < 0 || which > 1) { set_error("bad argument"); return REEF_ERR_ARG; }
    if (count == 0) return REEF_OK;
    DeviceCall call(c, OnExit::RELEASE_IF_IDLE);
    REEF_TRY(call.enter());
    REEF_TRY(sc_defer_flush<C>(c));        // rows whose first fold was deferred are written out: this is not their second fold
    const size_t live = which == 0 ? c->valid_t : c->valid_e;
    if (count > live) {
        set_error("read of %zu entries, but only %zu are live after the last fold (a fold writes entries [0, pow))", count, live);
        return REEF_ERR_ARG;
    }
    REEF_TRY(c->stage.ensure(count * sizeof(fe256)));
    if (which == 1 && c->r1) REEF_TRY(sc_r1_materialize<C>(c, true));   // a look at EQ: written out for the reader, the rounds go on without it
    const fe256 *src = (which == 0 ? (c->fresh ? c->T0 : c->T) : c->E).template as<fe256>();
    hipLaunchKernelGGL(k_fe_export<ScCtx<C>::F>, dim3(ceil_div(count, 256)), dim3(256), 0, c->stream, src, (u64)count, 0, 0,
                       c->stage.template as<fe256>());
    REEF_HIP_TRY(hipGetLastError());
    REEF_HIP_TRY(hipMemcpyAsync(out_host, c->stage.p, count * sizeof(fe256), hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    return REEF_OK;
}

// out[j] = T[idx[j]] of the table as last set -- the v_i of a step's lookups (r1cs.rs:2066-2077) once the document lives on the device
// only.  Reads the pristine copy and touches nothing a round depends on: no flush of a deferred fold, no change to fresh / valid / the
// rank-one state, buffers of its own.  It ends with a wait for the stream like reef_sc_read, which leaves the rounds that follow
// the kernels and the operands they would have had without it.
template <int C> static reef_status v_sc_lookup(void *impl, const uint64_t *idx, size_t k, reef_fe *out, int out_loc) {
    ScCtx<C> *c = (ScCtx<C> *)impl;
    if (!c) { set_error("null argument"); return REEF_ERR_ARG; }
    if (k == 0) return REEF_OK;
    if (!idx || !out) { set_error("reef_sc_lookup: %s is NULL", !idx ? "idx" : "out"); return REEF_ERR_ARG; }
    if (k > ((size_t)1 << 31)) { set_error("reef_sc_lookup: %zu indices, at most 2^31 per call", k); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::RELEASE_IF_IDLE);
    if (!c->has_table) { set_error("reef_sc_lookup: no table has been set on this ctx"); return REEF_ERR_ARG; }
    for (size_t j = 0; j < k; ++j)
        if (idx[j] >= c->len) {
            set_error("reef_sc_lookup: idx[%zu] = %llu is not below the table length %zu", j, (unsigned long long)idx[j], c->len);
            return REEF_ERR_ARG;
        }
    REEF_TRY(call.enter());
    const bool to_host = out_loc != REEF_DEVICE;
    const size_t idx_bytes = (k * sizeof(u64) + 31) & ~(size_t)31;
    REEF_TRY(c->lk.ensure(idx_bytes + (to_host ? k * sizeof(fe256) : 0)));
    REEF_HIP_TRY(hipMemcpyAsync(c->lk.p, idx, k * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    fe256 *dst = to_host ? reinterpret_cast<fe256 *>(c->lk.template as<unsigned char>() + idx_bytes) : (fe256 *)out;
    hipLaunchKernelGGL(k_sc_lookup<ScCtx<C>::F>, dim3((u32)ceil_div(k, 256)), dim3(256), 0, c->stream, (const fe256 *)c->T0.template as<fe256>(), (u64)c->len,
                       (const u64 *)c->lk.template as<u64>(), (u32)k, dst);
    REEF_HIP_TRY(hipGetLastError());
    if (to_host) REEF_HIP_TRY(hipMemcpyAsync(out, dst, k * sizeof(fe256), hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    return REEF_OK;
}

// ---- The rounds.  An entry point checks its arguments, asks sc_round_plan (sumcheck_plan.h) which route the round takes and with which
// grids, and hands over to the route's launch function below; the state changes are theirs, in their order among the launches.

// the plan of this call from the state `s`, a deferred fold written out where the plan says so; REEF_ERR_ARG: too few live entries
template <int C> static reef_status sc_plan_call(ScCtx<C> *c, ScCall call, size_t pow, const ScState &s, ScRoundPlan *p) {
    const reef_status rs = sc_round_plan(call, pow, s, c->sw, p);
    if (p->flush) REEF_TRY(sc_defer_flush<C>(c));
    if (rs != REEF_OK)
        set_error("%s with pow = %zu needs %zu live entries per table; T has %zu, EQ has %zu", call == SC_COEFFS ? "round" : "fold", pow, 2 * pow, c->valid_t, c->valid_e);
    return rs;
}
// The kernels of a fused rank-one round come with the sum t1 e1 (template argument S11) and without: the sum-check identity gives it
// where the coefficients of THIS round are still in out3 and r is its challenge (REEF_SC_IDENTITY=0: all three sums are accumulated).
template <class K> static K sc_s11(bool ident, K with_sum, K without) { return ident ? without : with_sum; }
// k_sc_r1_fold_coeffs over a row list (list == nullptr: over all hn rows): fold and the next sums in one pass over T
template <int C>
static void sc_launch_general(ScCtx<C> *c, const R1View<C> &v, const ScRoundPlan &p, ScGrid g, const u32 *list, u32 nlist, const fe256 &rr) {
    constexpr int F = ScCtx<C>::F;
    hipLaunchKernelGGL((sc_s11(p.ident, k_sc_r1_fold_coeffs<F, true>, k_sc_r1_fold_coeffs<F, false>)), sc_dim3(g), dim3(256), 0, c->stream,
                       (const fe256 *)(c->fresh ? c->T0 : c->T).template as<fe256>(), c->T.template as<fe256>(), c->r1_lo, p.hn, list, nlist, rr,
                       (const fe_limbs *)v.f0, (const fe_limbs *)v.f1, (const fe_limbs *)v.fd, (const fe256 *)v.fl, c->r1acc.template as<unsigned long long>());
}
// k_sc_coeffs over `pairs` pairs of the tables as they stand, and the coefficients to the caller
template <int C> static reef_status sc_dense_sums(ScCtx<C> *c, const ScRoundPlan &p, size_t pairs, reef_fe *out3_host) {
    const bool one = p.one_launch;
    hipLaunchKernelGGL(k_sc_coeffs<ScCtx<C>::F>, dim3(p.blocks), dim3(256), 0, c->stream, (const fe256 *)(c->fresh ? c->T0 : c->T).template as<fe256>(),
                       (const fe256 *)c->E.template as<fe256>(), (u32)pairs, c->partial.template as<unsigned long long>(),
                       one ? c->gacc.template as<unsigned long long>() : nullptr, c->pinned3, one ? ++c->seq : 0u, c->sw.order);
    return sc_dense_finish<C>(c, one, p.blocks, out3_host);
}
// FH folded with r, then T (EQ's share of the fold is k_sc_r1_prep)
template <int C> static reef_status sc_r1_fold(ScCtx<C> *c, const ScRoundPlan &p, size_t pow, const fe256 &rr) {
    REEF_TRY(sc_r1_prep<C>(c, &rr, pow));
    hipLaunchKernelGGL(k_sc_r1_fold<ScCtx<C>::F>, dim3(p.fold_blocks), dim3(256), 0, c->stream, (const fe256 *)(c->fresh ? c->T0 : c->T).template as<fe256>(),
                       c->T.template as<fe256>(), (u32)pow, rr);
    c->fresh = false;
    c->valid_t = c->valid_e = pow;
    return REEF_OK;
}

// SC_SUMS_STRUCT: per side, the S rows and the W rows; then the constant rows of both sides in one launch
template <int C> static reef_status sc_sums_struct(ScCtx<C> *c, const ScRoundPlan &p, size_t pow, reef_fe *out3_host) {
    constexpr int F = ScCtx<C>::F;
    const R1View<C> v(c);
    const u32 hn = p.hn;
    const u32 *lists = c->st_lists.template as<u32>();
    unsigned long long *part = c->r1acc.template as<unsigned long long>();
    const fe256 *T0 = c->T0.template as<fe256>();
    ScConstSets sets = {};
    for (u32 side = 0; side < 2; ++side) {
        const fe_limbs *fa = side ? v.f1 : v.f0;
        const ScList &W = c->st.sum[side][0], &S = c->st.sum[side][1], &K = c->st.sum[side][2];
        if (S.n)
            hipLaunchKernelGGL((k_sc_r1s_rows<F, false>), sc_dim3(p.g_sum[side][1]), dim3(256), 0, c->stream, T0, (const u32 *)c->st_s32.template as<u32>(), c->r1_lo,
                               side ? hn : 0u, side, lists + S.off, S.n, fa, (const fe_limbs *)v.fd, (const fe256 *)v.fl, part);
        if (W.n)
            hipLaunchKernelGGL((k_sc_r1s_rows<F, true>), sc_dim3(p.g_sum[side][0]), dim3(256), 0, c->stream, T0, (const u32 *)c->st_s32.template as<u32>(), c->r1_lo,
                               side ? hn : 0u, side, lists + W.off, W.n, fa, (const fe_limbs *)v.fd, (const fe256 *)v.fl, part);
        sets.row_off[side] = side ? hn : 0u; sets.side[side] = side; sets.nlist[side] = K.n; sets.list[side] = lists + K.off;
        sets.fa[side] = fa; sets.fd[side] = v.fd;
    }
    if (p.const_blocks)
        hipLaunchKernelGGL(k_sc_r1s_const<F>, dim3(p.const_blocks, 2), dim3(256), 0, c->stream, T0, c->r1_lo, sets, (const fe256 *)c->st_sumfl.template as<fe256>(), part);
    REEF_HIP_TRY(hipGetLastError());
    return sc_r1_finish<C>(c, pow, out3_host);
}
template <int C> static reef_status sc_sums_r1(ScCtx<C> *c, const ScRoundPlan &p, size_t pow, reef_fe *out3_host) {
    const R1View<C> v(c);
    hipLaunchKernelGGL(k_sc_r1_coeffs<ScCtx<C>::F>, sc_dim3(p.grid), dim3(256), 0, c->stream, (const fe256 *)(c->fresh ? c->T0 : c->T).template as<fe256>(), c->r1_lo,
                       p.hn, p.rows_per_chunk, (const fe_limbs *)v.f0, (const fe_limbs *)v.f1, (const fe_limbs *)v.fd, (const fe256 *)v.fl,
                       c->r1acc.template as<unsigned long long>());
    return sc_r1_finish<C>(c, pow, out3_host);
}

// linear_mle_product, first half: out = (xsq, x, con)
template <int C> static reef_status v_sc_coeffs(void *impl, size_t pow, reef_fe *out3_host) {
    ScCtx<C> *c = (ScCtx<C> *)impl;
    if (!c || !out3_host || pow == 0 || 2 * pow > c->len) { set_error("bad argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::STAY);
    REEF_TRY(call.enter());
    ScRoundPlan p;
    REEF_TRY(sc_plan_call<C>(c, SC_COEFFS, pow, sc_state<C>(c), &p));
    switch (p.route) {
    case SC_SUMS_STRUCT: return sc_sums_struct<C>(c, p, pow, out3_host);
    case SC_SUMS_R1: return sc_sums_r1<C>(c, p, pow, out3_host);
    default: break;
    }
    c->r1_prev_pow = 0;
    if (p.materialize) REEF_TRY(sc_r1_materialize<C>(c));
    return sc_dense_sums<C>(c, p, pow, out3_host);
}

// linear_mle_product, second half
template <int C> static reef_status v_sc_fold(void *impl, size_t pow, const reef_fe *r) {
    ScCtx<C> *c = (ScCtx<C> *)impl;
    if (!c || !r || pow == 0 || 2 * pow > c->len) { set_error("bad argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::STAY);
    REEF_TRY(call.enter());
    c->r1_prev_pow = 0;                  // the tables change: no coefficients on the device describe them any more
    ScRoundPlan p;
    REEF_TRY(sc_plan_call<C>(c, SC_FOLD, pow, sc_state<C>(c), &p));
    fe256 rr;
    memcpy(&rr, r, sizeof rr);
    if (p.route == SC_FOLD_R1) {
        REEF_TRY(sc_r1_fold<C>(c, p, pow, rr));
        REEF_HIP_TRY(hipGetLastError());
        if (p.materialize) REEF_TRY(sc_r1_materialize<C>(c));      // the FH bits are used up: 2^lo entries, dense from here
        return REEF_OK;
    }
    if (p.materialize) REEF_TRY(sc_r1_materialize<C>(c));
    c->valid_t = c->valid_e = pow;
    hipLaunchKernelGGL(k_sc_fold<ScCtx<C>::F>, dim3(p.fold_blocks), dim3(256), 0, c->stream, (const fe256 *)(c->fresh ? c->T0 : c->T).template as<fe256>(),
                       c->T.template as<fe256>(), c->E.template as<fe256>(), (u32)pow, rr);
    c->fresh = false;
    REEF_HIP_TRY(hipGetLastError());
    return REEF_OK;   // ordered before the next call on the ctx's stream
}

// SC_FC_DEFER, after k_sc_r1_kprep: sums of the next round from the structure.  The rows of st.f8x are not written (their second fold
// will write a quarter-size table from the sources): their share of the sums comes straight from the pristine rows, block by block, with
// the scaled row factors -- 18 multiply-adds per 4-byte entry, no t' anywhere.  The other fast rows and the general ones as in SC_FC_STRUCT.
template <int C> static void sc_fc_defer(ScCtx<C> *c, const ScRoundPlan &p, const R1View<C> &v, size_t pow, const fe256 &rr) {
    constexpr int F = ScCtx<C>::F;
    const u32 hn = p.hn;
    const u32 *lists = c->st_lists.template as<u32>();
    fe_limbs *ka = c->st_k.template as<fe_limbs>(), *kc = ka + hn;
    u32 *smask = reinterpret_cast<u32 *>(kc + hn);
    unsigned long long *part = c->r1acc.template as<unsigned long long>();
    fe_limbs *fa4 = reinterpret_cast<fe_limbs *>(smask + hn) + hn, *fd4 = fa4 + 4 * (size_t)hn;   // after K2A, K2C
    hipLaunchKernelGGL(k_sc_r2s_factors<F>, dim3(p.prep_blocks), dim3(256), 0, c->stream, (const fe_limbs *)v.f0, (const fe_limbs *)v.f1, (const fe_limbs *)v.fd, hn,
                       rr, fa4, fd4);
    const fe256 *T0 = c->T0.template as<fe256>();
    ScConstSets sets = {};
    for (u32 b = 0; b < 4; ++b) {
        const ScList &S = c->st.d8[b][0], &K = c->st.d8[b][1];
        const fe_limbs *fab = fa4 + (size_t)b * hn, *fdb = fd4 + (size_t)b * hn;
        if (S.n)
            hipLaunchKernelGGL((k_sc_r1s_rows<F, false>), sc_dim3(p.g_d8[b]), dim3(256), 0, c->stream, T0, (const u32 *)c->st_s32.template as<u32>(), c->r1_lo, b * hn,
                               b & 1u, lists + S.off, S.n, fab, fdb, (const fe256 *)v.fl, part);
        sets.row_off[b] = b * hn; sets.side[b] = b & 1u; sets.nlist[b] = K.n; sets.list[b] = lists + K.off;
        sets.fa[b] = fab; sets.fd[b] = fdb;
    }
    if (p.const_blocks)
        hipLaunchKernelGGL(k_sc_r1s_const<F>, dim3(p.const_blocks, 4), dim3(256), 0, c->stream, T0, c->r1_lo, sets, (const fe256 *)c->st_sumfl.template as<fe256>(), part);
    if (c->st.frest.n)
        sc_launch_cs<C>(c, v, sc_s11(p.ident, k_sc_r1_fold_coeffs_cs<F, true, true>, k_sc_r1_fold_coeffs_cs<F, false, true>), p.g_frest, hn, c->st.frest, rr, part);
    if (c->st.gen.n) sc_launch_general<C>(c, v, p, p.g_gen, lists + c->st.gen.off, c->st.gen.n, rr);
    if (p.points_blocks)                     // the few entries of t' the masses of the next round read
        hipLaunchKernelGGL(k_sc_defer_points<F>, dim3(p.points_blocks), dim3(256), 0, c->stream, (const u32 *)c->st_s32.template as<u32>(), c->T.template as<fe256>(),
                           c->r1_lo, hn, (u32)(pow / 2), (const u32 *)c->r1mq.template as<u32>(), c->r1_nq, rr, (const fe_limbs *)ka, (const fe_limbs *)kc,
                           (const u32 *)smask);
    c->defer_on = true;
    c->defer_r1 = rr;
    c->defer_pow = pow / 2;
    c->defer_hq = hn;
}
// SC_FC_STRUCT, SC_FC_DEFER: rows whose four sources are constant or small: 4-byte reads; the few others through the general kernel
template <int C> static void sc_fc_struct(ScCtx<C> *c, const ScRoundPlan &p, const R1View<C> &v, size_t pow, const fe256 &rr) {
    constexpr int F = ScCtx<C>::F;
    const u32 hn = p.hn;
    fe_limbs *ka = c->st_k.template as<fe_limbs>(), *kc = ka + hn;
    u32 *smask = reinterpret_cast<u32 *>(kc + hn);
    hipLaunchKernelGGL(k_sc_r1_kprep<F>, dim3(p.prep_blocks), dim3(256), 0, c->stream, (const fe256 *)c->T0.template as<fe256>(),
                       (const u32 *)c->st_flags.template as<u32>(), c->r1_lo, hn, rr, ka, kc, smask);
    if (p.route == SC_FC_DEFER) return sc_fc_defer<C>(c, p, v, pow, rr);
    if (c->st.fast.n)
        sc_launch_cs<C>(c, v, sc_s11(p.ident, k_sc_r1_fold_coeffs_cs<F, true>, k_sc_r1_fold_coeffs_cs<F, false>), p.g_fast, hn, c->st.fast, rr,
                        c->r1acc.template as<unsigned long long>());
    if (c->st.gen.n) sc_launch_general<C>(c, v, p, p.g_gen, c->st_lists.template as<u32>() + c->st.gen.off, c->st.gen.n, rr);
}
// SC_FC_SECOND: the first fold was deferred for the rows of st.f8x and this call is their SECOND fold -- straight from the 4-byte
// sources.  hn = an eighth of the pristine rows = half of defer_hq: g < hn; st.f8 from the sources, st.g8 from the dense rows
template <int C> static void sc_fc_second(ScCtx<C> *c, const ScRoundPlan &p, const R1View<C> &v, const fe256 &rr) {
    constexpr int F = ScCtx<C>::F;
    c->defer_on = false;
    const u32 hn = p.hn, hq = p.hq;
    const u32 *lists = c->st_lists.template as<u32>();
    fe_limbs *ka = c->st_k.template as<fe_limbs>(), *kc = ka + hq;
    u32 *smask = reinterpret_cast<u32 *>(kc + hq);
    fe_limbs *k2a = reinterpret_cast<fe_limbs *>(smask + hq), *k2c = k2a + hn;
    hipLaunchKernelGGL(k_sc_r2_kprep<F>, dim3(p.prep_blocks), dim3(256), 0, c->stream, (const fe_limbs *)ka, (const fe_limbs *)kc, hn, rr, k2a, k2c);
    hipLaunchKernelGGL((sc_s11(p.ident, k_sc_r2_fold_coeffs_cs<F, true>, k_sc_r2_fold_coeffs_cs<F, false>)), sc_dim3(p.g_f8), dim3(256), 0, c->stream,
                       (const u32 *)c->st_s32.template as<u32>(), c->T.template as<fe256>(), c->r1_lo, hq, lists + c->st.f8.off, c->st.f8.n, c->defer_r1, rr,
                       (const fe_limbs *)k2a, (const fe_limbs *)k2c, (const u32 *)smask, (const fe_limbs *)v.f0, (const fe_limbs *)v.f1, (const fe_limbs *)v.fd,
                       (const fe256 *)v.fl, c->r1acc.template as<unsigned long long>());
    if (c->st.g8.n) sc_launch_general<C>(c, v, p, p.g_gen, lists + c->st.g8.off, c->st.g8.n, rr);
}
// SC_FC_R1 and the three above: the next round stays rank-one: fold and its sums in one pass over T
template <int C> static reef_status sc_fc_rank1(ScCtx<C> *c, const ScRoundPlan &p, size_t pow, const fe256 &rr, reef_fe *out3_host) {
    REEF_TRY(sc_r1_prep<C>(c, &rr, pow));
    const R1View<C> v(c);
    switch (p.route) {
    case SC_FC_STRUCT:
    case SC_FC_DEFER: sc_fc_struct<C>(c, p, v, pow, rr); break;
    case SC_FC_SECOND: sc_fc_second<C>(c, p, v, rr); break;
    default: sc_launch_general<C>(c, v, p, p.grid, nullptr, 0, rr);
    }
    c->fresh = false;
    c->valid_t = c->valid_e = pow;
    return sc_r1_finish<C>(c, pow / 2, out3_host, p.ident ? &rr : nullptr);
}

// fold with `pow` and return the coefficients of the next round (pow/2) from the same pass
template <int C> static reef_status v_sc_fold_coeffs(void *impl, size_t pow, const reef_fe *r, reef_fe *out3_host) {
    ScCtx<C> *c = (ScCtx<C> *)impl;
    if (!c || !r || !out3_host || pow < 2 || 2 * pow > c->len) { set_error("bad argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::STAY);
    REEF_TRY(call.enter());
    const ScState s = sc_state<C>(c);    // with r1_prev_pow: do the coefficients on the device describe the tables this call folds?
    c->r1_prev_pow = 0;
    ScRoundPlan p;
    REEF_TRY(sc_plan_call<C>(c, SC_FOLD_COEFFS, pow, s, &p));
    fe256 rr;
    memcpy(&rr, r, sizeof rr);
    switch (p.route) {
    case SC_FC_R1: case SC_FC_STRUCT: case SC_FC_DEFER: case SC_FC_SECOND: return sc_fc_rank1<C>(c, p, pow, rr, out3_host);
    case SC_FC_LAST_R1:                  // fold T, write the live entries of EQ out, and take the next sums with the dense kernel
        REEF_TRY(sc_r1_fold<C>(c, p, pow, rr));
        REEF_TRY(sc_r1_materialize<C>(c));
        return sc_dense_sums<C>(c, p, pow / 2, out3_host);
    default: break;
    }
    if (p.materialize) REEF_TRY(sc_r1_materialize<C>(c));
    c->valid_t = c->valid_e = pow;
    const fe256 *Tsrc = (const fe256 *)(c->fresh ? c->T0 : c->T).template as<fe256>();
    const bool one = p.one_launch;
    if (p.route == SC_FC_SPLIT)
        hipLaunchKernelGGL(k_sc_fold_coeffs_split<ScCtx<C>::F>, dim3(p.blocks), dim3(256), 0, c->stream, Tsrc, c->T.template as<fe256>(), c->E.template as<fe256>(),
                           (u32)pow, rr, c->gacc.template as<unsigned long long>(), c->pinned3, ++c->seq, c->sw.order);
    else
        hipLaunchKernelGGL(k_sc_fold_coeffs<ScCtx<C>::F>, dim3(p.blocks), dim3(256), 0, c->stream, Tsrc, c->T.template as<fe256>(), c->E.template as<fe256>(), (u32)pow,
                           rr, c->partial.template as<unsigned long long>(), one ? c->gacc.template as<unsigned long long>() : nullptr, c->pinned3,
                           one ? ++c->seq : 0u, c->sw.order);
    c->fresh = false;
    return sc_dense_finish<C>(c, one, p.blocks, out3_host);
}

// gen_eq_table into the ctx's EQ table: rs has nq + 1 entries, last_q has ell = log2(len) entries
template <int C>
static reef_status v_sc_gen_eq(void *impl, const reef_fe *rs, const uint32_t *qs, size_t nq, const reef_fe *last_q, size_t ell) {
    ScCtx<C> *c = (ScCtx<C> *)impl;
    if (!c || !rs || (nq && !qs) || !last_q || ((size_t)1 << ell) != c->len) { set_error("bad argument (ell must be log2 of the table length)"); return REEF_ERR_ARG; }
    for (size_t k = 0; k < nq; ++k)
        if (qs[k] >= c->len) { set_error("qs[%zu] out of range", k); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::RELEASE_IF_IDLE);
    REEF_TRY(call.enter());
    REEF_TRY(sc_defer_flush<C>(c));        // rows whose first fold was deferred are written out: this is not their second fold
    c->valid_e = c->len;
    sc_read_switches<C>(c);                  // a step runs under one setting of the switches
    const u32 lo_bits = (u32)(ell / 2), hi_bits = (u32)ell - lo_bits;
    c->r1_prev_pow = 0;
    REEF_HIP_TRY(hipMemsetAsync(c->gacc.p, 0, 28 * sizeof(u64), c->stream));   // the one-launch rounds leave it at zero; a step starts from zero whatever happened before
    REEF_HIP_TRY(hipMemsetAsync(c->r1acc.p, 0, R1_GROUPS * R1_SLOTS * sizeof(u64), c->stream));   // so do the sums kernels' accumulator sets (k_sc_r1_final zeroes them; a round that failed half-way did not: ADVICE r4)
    const size_t nfac = ((size_t)1 << hi_bits) + ((size_t)1 << lo_bits);
    REEF_TRY(c->fac.ensure(nfac * sizeof(fe256)));
    const size_t in_bytes = (ell + nq + 1) * sizeof(fe256) + (nq + 1) * sizeof(u32);
    REEF_TRY(c->misc.ensure(in_bytes));
    fe256 *d_lq = c->misc.template as<fe256>();
    fe256 *d_rs = d_lq + ell;
    u32 *d_qs = reinterpret_cast<u32 *>(d_rs + nq + 1);
    {
        if (in_bytes > c->pin_in_cap) {
            for (auto &e : c->pin_ev) if (e) REEF_HIP_TRY(hipEventSynchronize(e));
            if (c->pin_in) (void)hipHostFree(c->pin_in);
            c->pin_in = nullptr;
            c->pin_in_cap = 0;
            REEF_HIP_TRY(hipHostMalloc((void **)&c->pin_in, 2 * (in_bytes + 1024), hipHostMallocDefault));
            c->pin_in_cap = in_bytes + 1024;
        }
        const int half = c->pin_next;
        c->pin_next ^= 1;
        if (!c->pin_ev[half]) REEF_HIP_TRY(hipEventCreateWithFlags(&c->pin_ev[half], hipEventDisableTiming));
        else REEF_HIP_TRY(hipEventSynchronize(c->pin_ev[half]));     // the copy that last read this half (two calls ago)
        unsigned char *st = c->pin_in + (size_t)half * c->pin_in_cap;
        if (ell) memcpy(st, last_q, ell * sizeof(fe256));
        memcpy(st + ell * sizeof(fe256), rs, (nq + 1) * sizeof(fe256));
        if (nq) memcpy(st + (ell + nq + 1) * sizeof(fe256), qs, nq * sizeof(u32));
        REEF_HIP_TRY(hipMemcpyAsync(d_lq, st, in_bytes, hipMemcpyHostToDevice, c->stream));
        REEF_HIP_TRY(hipEventRecord(c->pin_ev[half], c->stream));
    }
    fe256 rs_last;
    memcpy(&rs_last, rs + nq, sizeof rs_last);
    fe256 *fac_hi = c->fac.template as<fe256>(), *fac_lo = fac_hi + ((size_t)1 << hi_bits);
    hipLaunchKernelGGL(k_sc_eq_factors<ScCtx<C>::F>, dim3(ceil_div(nfac, 256)), dim3(256), 0, c->stream, d_lq, (u32)ell, lo_bits, rs_last, fac_hi,
                       fac_lo);
    c->r1 = false;
    if (sc_eq_rank1(c->len, c->sw)) {
        // EQ stays FH (x) FL + masses (sumcheck_kernels.inc): nothing of 2^ell entries is written here
        c->r1_lo = lo_bits;
        c->r1_hi = c->r1_hi0 = hi_bits;
        c->r1_nq = (u32)nq;
        REEF_TRY(c->r1rows.ensure(((size_t)3 << (hi_bits - 1)) * sizeof(fe_limbs)));
        REEF_TRY(c->r1mq.ensure((nq + 1) * sizeof(u32)));
        REEF_TRY(c->r1mw.ensure((nq + 1) * sizeof(fe256)));
        // masses, and the sum of FL (what the constant rows of a structured table are multiplied by: one) whenever EQ is rank-one --
        // the structure may be found by a set_table that comes AFTER this call, and the results must not depend on the order (ADVICE r3)
        REEF_TRY(c->st_sumfl.ensure(sizeof(fe256)));
        hipLaunchKernelGGL(k_sc_r1_mass_init<ScCtx<C>::F>, dim3(std::max<u32>(1u, ceil_div(nq, 256))), dim3(256), 0, c->stream, (const fe256 *)d_rs, (const u32 *)d_qs,
                           (u32)nq, c->r1mw.template as<fe256>(), c->r1mq.template as<u32>(), c->st_sumfl.template as<fe256>());
        c->r1 = true;
        REEF_TRY(sc_r1_prep<C>(c, nullptr, c->len / 2));
    } else {
        hipLaunchKernelGGL(k_sc_eq_table<ScCtx<C>::F>, dim3(sc_fold_blocks(c->len)), dim3(256), 0, c->stream, fac_hi, fac_lo,
                           (u32)ell, lo_bits, c->E.template as<fe256>());
        if (nq) hipLaunchKernelGGL(k_sc_eq_points<ScCtx<C>::F>, dim3(ceil_div(nq, 64)), dim3(64), 0, c->stream, d_rs, (const u32 *)d_qs, (u32)nq,
                                   c->E.template as<fe256>());
    }
    REEF_HIP_TRY(hipGetLastError());
    return REEF_OK;   // nothing to wait for: the caller's arrays were copied to pinned staging above, the kernels are in stream order
}

// T <- the table as it was set (start of the next folding step; the reference clones it per step, r1cs.rs:2320)
template <int C> static reef_status v_sc_reset(void *impl) {
    ScCtx<C> *c = (ScCtx<C> *)impl;
    if (!c) { set_error("null argument"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(c->mu);
    c->valid_t = c->len;
    c->defer_on = false;   // the step starts over from the pristine table
    c->fresh = true;   // no copy: the first fold of the step reads the pristine table and writes the working one
    c->r1_prev_pow = 0;
    return REEF_OK;
}

template <int C> static reef_status v_sc_sync(void *impl) {
    ScCtx<C> *c = (ScCtx<C> *)impl;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->lease.counted) return REEF_OK;
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    c->lease.idle();
    return REEF_OK;
}

}  // namespace reef
