// Host side of the sum-check vector kernels (row N2); included after engine.inc.
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
    struct StList { u32 off = 0, n = 0; };
    StList st_sum[2][3];                 // round-one sums: [side][class W, S, K] -> pair rows h < H/2
    StList st_fast, st_gen;              // first fold: h < H/4 whose four sources are all K or S / the others
    // first fold deferred by one round (sumcheck_kernels.inc): g < H/8 with both quadruples g, g + H/8 fast (st_f8), the same rows
    // as a list of quadruples (st_f8x), the fast quadruples that are not among them (st_frest), the g that are not in st_f8 (st_g8)
    StList st_f8, st_f8x, st_frest, st_g8;
    StList st_d8[4][2];                  // the rows of st_f8x by source block b (row h + b * H/4) and class: [b][0] S rows, [b][1] K rows
    bool defer_on = false;               // the rows of st_f8x have not been written: the next call is their second fold, or they are flushed
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
    struct Switches {
        bool one_launch = true, rank1 = true, structured = true, identity = true, defer = true;
        size_t r1_min_pow = (size_t)1 << 21;
        u32 floor_blocks = 256;
        u32 one_launch_max = 64;         // REEF_SC_ONE_LAUNCH_MAX: a round of at most this many blocks finishes its sums itself (the last block to arrive)
        size_t split_max = (size_t)1 << 14;   // REEF_SC_SPLIT_MAX: rounds of at most this many pairs spread an item over four waves (0: never)
        u32 split_blocks = 64;             // REEF_SC_SPLIT_BLOCKS: the most workgroups of such a round (every one adds 27 words to the shared sums: 256 of them cost the 2^14-pair round 7 us)
        u32 items = 8;                   // pairs a thread of a dense round takes at least (its three lazy reductions and the block's sums are per thread)
        u32 order = 2;                   // REEF_SC_FENCE: how a multi-block one-launch round orders its additions before the ticket (sumcheck_kernels.inc: SC_ORDER_*)
        u32 set_sub = 8;                 // REEF_SC_SET_SUB: the most 128-entry tiles a wave of k_sc_set_parts takes (two entries per lane and tile)
    } sw;
};
// REEF_SC_ONE_LAUNCH=0: the sums of a round are finished by a second kernel and copied back (rounds 1-2 form), for A/B runs.
// REEF_SC_RANK1=0: gen_eq_table writes the EQ table out, as rounds 1-2 did.  REEF_SC_STRUCT=0: the first round of a step reads
// the pristine table as dense field elements whatever it holds.  REEF_SC_IDENTITY=0: all three sums of a fused rank-one round
// are accumulated.  REEF_SC_RANK1_MIN_POW: rounds below this many entries per half are launch-latency-bound; there the dense fused
// kernel (one launch and the final sums) is shorter than the rank-one round (row factors, pass, final sums), so EQ is written out
// once the tables have shrunk to it (measured: 2^21-entry tables 1.18 ms dense, 1.27 ms rank-one; 2^24: 2.31 / 2.02; 2^26: 5.67 / 3.68).
template <int C> static void sc_read_switches(ScCtx<C> *c) {
    auto off = [](const char *name) { const char *e = exp_env(name); return e && e[0] == '0'; };
    c->sw.one_launch = !off("REEF_SC_ONE_LAUNCH");
    c->sw.rank1 = !off("REEF_SC_RANK1");
    c->sw.structured = !off("REEF_SC_STRUCT");
    c->sw.identity = !off("REEF_SC_IDENTITY");
    c->sw.defer = !off("REEF_SC_DEFER");         // REEF_SC_DEFER=0: the first fold of a structured table is written out at once (round 3 form)
    const char *e = exp_env("REEF_SC_RANK1_MIN_POW");
    c->sw.r1_min_pow = (e && *e) ? (size_t)std::max<long long>(1, atoll(e)) : (size_t)1 << 21;
    e = exp_env("REEF_SC_ITEMS");
    c->sw.items = (e && *e) ? (u32)std::min<long long>(64, std::max<long long>(1, atoll(e))) : 8u;
    e = exp_env("REEF_SC_SPLIT_MAX");
    c->sw.split_max = (e && *e) ? (size_t)std::max<long long>(0, atoll(e)) : (size_t)1 << 14;
    e = exp_env("REEF_SC_SPLIT_BLOCKS");
    c->sw.split_blocks = (e && *e) ? (u32)std::min<long long>(1024, std::max<long long>(1, atoll(e))) : 64u;
    e = exp_env("REEF_SC_ONE_LAUNCH_MAX");
    c->sw.one_launch_max = (e && *e) ? (u32)std::min<long long>(8192, std::max<long long>(1, atoll(e))) : 64u;
    e = getenv("REEF_SC_FENCE");             // 2 (default since round 6): acq_rel ticket; 1: __threadfence before the ticket; 0: returning atomics + s_waitcnt only
    c->sw.order = (e && *e) ? (u32)std::min<long long>(2, std::max<long long>(0, atoll(e))) : 2u;
    e = exp_env("REEF_SC_SET_SUB");
    c->sw.set_sub = (e && *e) ? (u32)std::min<long long>(64, std::max<long long>(1, atoll(e))) : 8u;
    e = exp_env("REEF_SC_FLOOR");
    c->sw.floor_blocks = (e && *e) ? (u32)std::min<long long>(8192, std::max<long long>(1, atoll(e))) : 256u;
}
// Blocks of a dense round over `work` pairs: a thread pays ~7 products of fixed work (three lazy reductions, the wave's sums)
// against ~5 per pair, so a mid-sized round is spread over fewer, longer threads (2^20 pairs: 109 -> 74 us with 8 pairs each).
template <int C> static u32 sc_dense_blocks(const ScCtx<C> *c, size_t work) {
    const size_t one_each = std::max<size_t>(1, ceil_div(work, 256));      // a pair per thread: the shortest chain
    const size_t longer = std::max<size_t>(c->sw.floor_blocks, ceil_div(work, (size_t)256 * c->sw.items));   // never fewer blocks than CUs for it
    return (u32)std::min<size_t>(c->nblocks, std::min(one_each, longer));
}

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
        size_t cap = 2048;                   // REEF_SC_BLOCKS: the most blocks a round is spread over (A/B runs)
        if (const char *e = exp_env("REEF_SC_BLOCKS")) if (*e) cap = (size_t)std::min<long long>(8192, std::max<long long>(1, atoll(e)));
        c->nblocks = (u32)std::min<size_t>(cap, std::max<size_t>(1, len / 2 / 256));
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

// One-launch rounds only for rounds of a few blocks: 2048 blocks adding 27 limbs each to the same 27 words serialise (2^20-entry
// round: 58 -> 103 us), a small round saves its second kernel and its copy (46 -> 37 us per round, 16 of the 21 rounds of a 2^21 step).
template <int C> static bool sc_one_launch(const ScCtx<C> *c, u32 blocks) { return c->sw.one_launch && blocks <= c->sw.one_launch_max; }
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
// a round with `pow` can stay rank-one: both tables have exactly 2*pow live entries and the bit it folds is an FH bit
template <int C> static bool sc_r1_round(const ScCtx<C> *c, size_t pow) {
    return c->r1 && c->r1_hi >= 1 && c->valid_e == 2 * pow && c->valid_t == 2 * pow && pow >= c->sw.r1_min_pow;
}
// EQ written out where the dense kernels expect it (the live 2^(r1_hi + r1_lo) entries); leaves rank-one mode unless `keep`
template <int C> static reef_status sc_r1_materialize(ScCtx<C> *c, bool keep = false) {
    constexpr int F = ScCtx<C>::F;
    const R1View<C> v(c);
    const u32 ell_cur = c->r1_hi + c->r1_lo;
    const size_t n = (size_t)1 << ell_cur;
    hipLaunchKernelGGL(k_sc_eq_table<F>, dim3((u32)std::min<size_t>(4096, ceil_div(n, 256))), dim3(256), 0, c->stream, (const fe256 *)v.fh,
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
    const u32 threads = std::max<u32>(std::max<u32>(hn_next, r ? c->r1_nq : 0u), 1u);
    hipLaunchKernelGGL(k_sc_r1_prep<F>, dim3(ceil_div(threads, 256)), dim3(256), 0, c->stream, v.fh, hc, r ? 1 : 0, rr, hn_next, v.f0, v.f1, v.fd,
                       c->r1mq.template as<u32>(), c->r1mw.template as<fe256>(), c->r1_nq, (u32)pow);
    REEF_HIP_TRY(hipGetLastError());
    if (r) c->r1_hi -= 1;
    return REEF_OK;
}
// grid of the column kernels for `hn` pair rows: blocks over the columns x row groups, at most 1024 blocks (every block
// leaves 36 limb sums for k_sc_r1_final to add up: 2048 of them cost it 25 us)
template <int C> static reef_status sc_r1_grid(ScCtx<C> *c, u32 hn, dim3 *grid, u32 *rows_per_chunk) {
    const u32 gx = ceil_div((size_t)1 << c->r1_lo, 256);
    const u32 chunks = std::max<u32>(1u, std::min<u32>(hn, std::max<u32>(1u, 1024u / gx)));
    *rows_per_chunk = ceil_div(hn, chunks);
    *grid = dim3(gx, ceil_div(hn, *rows_per_chunk));
    return REEF_OK;
}
template <int C> static reef_status sc_r1_finish(ScCtx<C> *c, u32 blocks, size_t pow, reef_fe *out3_host, const fe256 *ident_r = nullptr) {
    constexpr int F = ScCtx<C>::F;
    fe256 rr = {};
    if (ident_r) rr = *ident_r;
    (void)blocks;
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
    size_t ell = 0;
    while (((size_t)1 << ell) < c->len) ++ell;
    const u32 lo = (u32)(ell / 2), hi = (u32)ell - lo;
    *lo_bits = lo;
    if (!c->sw.rank1 || !c->sw.structured || hi < 2 || c->len / 2 < c->sw.r1_min_pow) return REEF_OK;
    const u32 H = 1u << hi;
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
    auto cls = [&](u32 row) { return (flags[row] & 2u) ? 2u : (flags[row] & 1u) ? 1u : 0u; };   // K, S, W
    size_t plain = 0;
    for (u32 r = 0; r < H; ++r) plain += cls(r) != 0;
    if (2 * plain < H) return REEF_OK;
    std::vector<u32> lists;
    const u32 hn = H / 2, hq = H / 4;
    for (u32 side = 0; side < 2; ++side)
        for (u32 k = 0; k < 3; ++k) {
            c->st_sum[side][k].off = (u32)lists.size();
            for (u32 h = 0; h < hn; ++h)
                if (cls(h + side * hn) == k) lists.push_back(h);
            c->st_sum[side][k].n = (u32)lists.size() - c->st_sum[side][k].off;
        }
    auto fast = [&](u32 h) { return cls(h) && cls(h + hq) && cls(h + 2 * hq) && cls(h + 3 * hq); };
    c->st_fast.off = (u32)lists.size();
    for (u32 h = 0; h < hq; ++h)
        if (fast(h)) lists.push_back(h);
    c->st_fast.n = (u32)lists.size() - c->st_fast.off;
    c->st_gen.off = (u32)lists.size();
    for (u32 h = 0; h < hq; ++h)
        if (!fast(h)) lists.push_back(h);
    c->st_gen.n = (u32)lists.size() - c->st_gen.off;
    {
        const u32 h8 = hq / 2;
        auto fast8 = [&](u32 g) { return h8 && fast(g) && fast(g + h8); };
        c->st_f8.off = (u32)lists.size();
        for (u32 g = 0; g < h8; ++g)
            if (fast8(g)) lists.push_back(g);
        c->st_f8.n = (u32)lists.size() - c->st_f8.off;
        c->st_f8x.off = (u32)lists.size();
        for (u32 h = 0; h < hq; ++h)
            if (h8 && fast8(h % h8)) lists.push_back(h);
        c->st_f8x.n = (u32)lists.size() - c->st_f8x.off;
        c->st_frest.off = (u32)lists.size();
        for (u32 h = 0; h < hq; ++h)
            if (fast(h) && !(h8 && fast8(h % h8))) lists.push_back(h);
        c->st_frest.n = (u32)lists.size() - c->st_frest.off;
        c->st_g8.off = (u32)lists.size();
        for (u32 g = 0; g < h8; ++g)
            if (!fast8(g)) lists.push_back(g);
        c->st_g8.n = (u32)lists.size() - c->st_g8.off;
        for (u32 b = 0; b < 4; ++b)
            for (u32 k = 0; k < 2; ++k) {                  // cls: 1 = S, 2 = K
                c->st_d8[b][k].off = (u32)lists.size();
                for (u32 h = 0; h < hq; ++h)
                    if (h8 && fast8(h % h8) && cls(h + b * hq) == k + 1) lists.push_back(h);
                c->st_d8[b][k].n = (u32)lists.size() - c->st_d8[b][k].off;
            }
    }
    lists.push_back(0);
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
// the first round of a step on a structured table: tables are whole (2*pow = len), T is pristine, EQ is rank-one with all its FH bits
template <int C> static bool sc_struct_round(const ScCtx<C> *c, size_t pow) {
    return c->st_ok && c->fresh && 2 * pow == c->len && c->r1_hi == c->r1_hi0 && c->sw.structured;
}
// grid of a list-driven column kernel: blocks over the columns x row groups (at most 2048 blocks, at most 256 rows per thread)
template <int C> static dim3 sc_list_grid(const ScCtx<C> *c, u32 nlist) {
    const u32 gx = ceil_div((size_t)1 << c->r1_lo, 256);
    const u32 gy = std::max<u32>(1u, std::min<u32>(nlist, std::max<u32>(std::max<u32>(1u, 1024u / gx), ceil_div(nlist, 256))));
    return dim3(gx, gy);
}
// round-one sums of a structured table: per side, the S rows, the W rows and the K rows; returns the number of partial blocks
template <int C> static reef_status sc_struct_sums(ScCtx<C> *c, u32 *blocks_out) {
    constexpr int F = ScCtx<C>::F;
    const R1View<C> v(c);
    const u32 hn = 1u << (c->r1_hi - 1);
    const u32 *lists = c->st_lists.template as<u32>();
    size_t total = 0;
    for (u32 side = 0; side < 2; ++side) {
        for (u32 k = 0; k < 2; ++k) {
            const dim3 g = sc_list_grid<C>(c, c->st_sum[side][k].n);
            if (c->st_sum[side][k].n) total += (size_t)g.x * g.y;
        }
        total += std::max(ceil_div(c->st_sum[0][2].n, 256), ceil_div(c->st_sum[1][2].n, 256));   // the merged launch: the larger set's blocks, per side
    }
    (void)total;
    unsigned long long *part = c->r1acc.template as<unsigned long long>();
    const fe256 *T0 = c->T0.template as<fe256>();
    u32 at = 0;
    for (u32 side = 0; side < 2; ++side) {
        const fe_limbs *fa = side ? v.f1 : v.f0;
        const auto &W = c->st_sum[side][0], &S = c->st_sum[side][1];
        if (S.n) {
            const dim3 g = sc_list_grid<C>(c, S.n);
            hipLaunchKernelGGL((k_sc_r1s_rows<F, false>), g, dim3(256), 0, c->stream, T0, (const u32 *)c->st_s32.template as<u32>(), c->r1_lo, side ? hn : 0u, side,
                               lists + S.off, S.n, fa, (const fe_limbs *)v.fd, (const fe256 *)v.fl, part);
            at += g.x * g.y;
        }
        if (W.n) {
            const dim3 g = sc_list_grid<C>(c, W.n);
            hipLaunchKernelGGL((k_sc_r1s_rows<F, true>), g, dim3(256), 0, c->stream, T0, (const u32 *)c->st_s32.template as<u32>(), c->r1_lo, side ? hn : 0u, side,
                               lists + W.off, W.n, fa, (const fe_limbs *)v.fd, (const fe256 *)v.fl, part);
            at += g.x * g.y;
        }
    }
    {                                                         // the constant rows of both sides: one launch
        ScConstSets sets = {};
        u32 kb = 0;
        for (u32 side = 0; side < 2; ++side) {
            const auto &K = c->st_sum[side][2];
            sets.row_off[side] = side ? hn : 0u; sets.side[side] = side; sets.nlist[side] = K.n; sets.list[side] = lists + K.off;
            sets.fa[side] = side ? v.f1 : v.f0; sets.fd[side] = v.fd;
            kb = std::max(kb, ceil_div(K.n, 256));
        }
        if (kb) {
            hipLaunchKernelGGL(k_sc_r1s_const<F>, dim3(kb, 2), dim3(256), 0, c->stream, T0, c->r1_lo, sets, (const fe256 *)c->st_sumfl.template as<fe256>(),
                               part);
            at += 2 * kb;
        }
    }
    REEF_HIP_TRY(hipGetLastError());
    *blocks_out = at;
    return REEF_OK;
}

// The deferred first fold (k_sc_r1_fold_coeffs_cs<.., WRITE = false>) written out after all: any call that is not the second fold
// of the step finds the table as if nothing had been deferred.  The sums the kernel leaves go to scratch.
template <int C> static reef_status sc_defer_flush(ScCtx<C> *c) {
    if (!c->defer_on) return REEF_OK;
    c->defer_on = false;
    const u32 hq = c->defer_hq;
    const R1View<C> v(c);
    const u32 *lists = c->st_lists.template as<u32>();
    fe_limbs *ka = c->st_k.template as<fe_limbs>(), *kc = ka + hq;
    u32 *smask = reinterpret_cast<u32 *>(kc + hq);
    const dim3 g = sc_list_grid<C>(c, c->st_f8x.n);
    REEF_TRY(c->stage.ensure((size_t)R1_GROUPS * R1_SLOTS * sizeof(u64)));   // scratch accumulators: nobody reads these sums
    hipLaunchKernelGGL((k_sc_r1_fold_coeffs_cs<ScCtx<C>::F, true, true>), g, dim3(256), 0, c->stream, (const u32 *)c->st_s32.template as<u32>(),
                       c->T.template as<fe256>(), c->r1_lo, hq, lists + c->st_f8x.off, c->st_f8x.n, c->defer_r1, (const fe_limbs *)ka, (const fe_limbs *)kc,
                       (const u32 *)smask, (const fe_limbs *)v.f0, (const fe_limbs *)v.f1, (const fe_limbs *)v.fd, (const fe256 *)v.fl,
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
    // tiles per wave: 8 (16 entries per lane) where that still leaves 8192 waves -- by measurement at 2^26 entries, where the kernel
    // alone takes a quarter less time with 4 tiles than with 1 (the sweep: profiles/r12_sc_set_parts_timing.txt)
    const u32 tiles = (u32)ceil_div(c->len, 128), sub = std::max<u32>(1u, std::min<u32>(c->sw.set_sub, tiles / 8192u));
    hipLaunchKernelGGL(k_sc_set_parts<ScCtx<C>::F>, dim3(ceil_div(ceil_div(tiles, sub), 4)), dim3(256), 0, c->stream, a, (u32)c->len, lo, sub,
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

// linear_mle_product, first half: out = (xsq, x, con)
template <int C> static reef_status v_sc_coeffs(void *impl, size_t pow, reef_fe *out3_host) {
    ScCtx<C> *c = (ScCtx<C> *)impl;
    if (!c || !out3_host || pow == 0 || 2 * pow > c->len) { set_error("bad argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::STAY);
    REEF_TRY(call.enter());
    REEF_TRY(sc_defer_flush<C>(c));        // rows whose first fold was deferred are written out: this is not their second fold
    if (2 * pow > std::min(c->valid_t, c->valid_e)) { set_error("round with pow = %zu needs %zu live entries per table; T has %zu, EQ has %zu", pow, 2 * pow, c->valid_t, c->valid_e); return REEF_ERR_ARG; }
    if (sc_r1_round<C>(c, pow) && sc_struct_round<C>(c, pow)) {
        u32 blocks = 0;
        REEF_TRY(sc_struct_sums<C>(c, &blocks));
        return sc_r1_finish<C>(c, blocks, pow, out3_host);
    }
    if (sc_r1_round<C>(c, pow)) {
        const R1View<C> v(c);
        const u32 hn = 1u << (c->r1_hi - 1);
        dim3 grid;
        u32 rpc;
        REEF_TRY(sc_r1_grid<C>(c, hn, &grid, &rpc));
        hipLaunchKernelGGL(k_sc_r1_coeffs<ScCtx<C>::F>, grid, dim3(256), 0, c->stream, (const fe256 *)(c->fresh ? c->T0 : c->T).template as<fe256>(), c->r1_lo,
                           hn, rpc, (const fe_limbs *)v.f0, (const fe_limbs *)v.f1, (const fe_limbs *)v.fd, (const fe256 *)v.fl,
                           c->r1acc.template as<unsigned long long>());
        return sc_r1_finish<C>(c, grid.x * grid.y, pow, out3_host);
    }
    c->r1_prev_pow = 0;
    if (c->r1) REEF_TRY(sc_r1_materialize<C>(c));
    const u32 blocks = sc_dense_blocks<C>(c, pow);
    const bool one = sc_one_launch<C>(c, blocks);
    hipLaunchKernelGGL(k_sc_coeffs<ScCtx<C>::F>, dim3(blocks), dim3(256), 0, c->stream, (c->fresh ? c->T0 : c->T).template as<fe256>(),
                       c->E.template as<fe256>(), (u32)pow, c->partial.template as<unsigned long long>(),
                       one ? c->gacc.template as<unsigned long long>() : nullptr, c->pinned3, one ? ++c->seq : 0u, c->sw.order);
    return sc_dense_finish<C>(c, one, blocks, out3_host);
}

// linear_mle_product, second half
template <int C> static reef_status v_sc_fold(void *impl, size_t pow, const reef_fe *r) {
    ScCtx<C> *c = (ScCtx<C> *)impl;
    if (!c || !r || pow == 0 || 2 * pow > c->len) { set_error("bad argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::STAY);
    REEF_TRY(call.enter());
    REEF_TRY(sc_defer_flush<C>(c));        // rows whose first fold was deferred are written out: this is not their second fold
    c->r1_prev_pow = 0;                  // the tables change: no coefficients on the device describe them any more
    if (2 * pow > std::min(c->valid_t, c->valid_e)) { set_error("fold with pow = %zu needs %zu live entries per table; T has %zu, EQ has %zu", pow, 2 * pow, c->valid_t, c->valid_e); return REEF_ERR_ARG; }
    fe256 rr;
    memcpy(&rr, r, sizeof rr);
    if (sc_r1_round<C>(c, pow)) {
        REEF_TRY(sc_r1_prep<C>(c, &rr, pow));
        const u32 fb = (u32)std::min<size_t>(4096, std::max<size_t>(1, ceil_div(pow, 256)));
        hipLaunchKernelGGL(k_sc_r1_fold<ScCtx<C>::F>, dim3(fb), dim3(256), 0, c->stream, (const fe256 *)(c->fresh ? c->T0 : c->T).template as<fe256>(),
                           c->T.template as<fe256>(), (u32)pow, rr);
        c->fresh = false;
        c->valid_t = c->valid_e = pow;
        REEF_HIP_TRY(hipGetLastError());
        if (c->r1_hi == 0) REEF_TRY(sc_r1_materialize<C>(c));      // the FH bits are used up: 2^lo entries, dense from here
        return REEF_OK;
    }
    if (c->r1) REEF_TRY(sc_r1_materialize<C>(c));
    c->valid_t = c->valid_e = pow;
    const u32 blocks = (u32)std::min<size_t>(4096, std::max<size_t>(1, ceil_div(pow, 256)));
    hipLaunchKernelGGL(k_sc_fold<ScCtx<C>::F>, dim3(blocks), dim3(256), 0, c->stream, (const fe256 *)(c->fresh ? c->T0 : c->T).template as<fe256>(),
                       c->T.template as<fe256>(), c->E.template as<fe256>(), (u32)pow, rr);
    c->fresh = false;
    REEF_HIP_TRY(hipGetLastError());
    return REEF_OK;   // ordered before the next call on the ctx's stream
}

// fold with `pow` and return the coefficients of the next round (pow/2) from the same pass
template <int C> static reef_status v_sc_fold_coeffs(void *impl, size_t pow, const reef_fe *r, reef_fe *out3_host) {
    ScCtx<C> *c = (ScCtx<C> *)impl;
    if (!c || !r || !out3_host || pow < 2 || 2 * pow > c->len) { set_error("bad argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::STAY);
    REEF_TRY(call.enter());
    const size_t prev_pow = c->r1_prev_pow;
    c->r1_prev_pow = 0;
    if (2 * pow > std::min(c->valid_t, c->valid_e)) { set_error("fold with pow = %zu needs %zu live entries per table; T has %zu, EQ has %zu", pow, 2 * pow, c->valid_t, c->valid_e); return REEF_ERR_ARG; }
    fe256 rr;
    memcpy(&rr, r, sizeof rr);
    if (c->defer_on && !(pow == c->defer_pow && sc_r1_round<C>(c, pow) && c->r1_hi >= 2 && pow / 2 >= c->sw.r1_min_pow)) REEF_TRY(sc_defer_flush<C>(c));
    if (sc_r1_round<C>(c, pow)) {
        if (c->r1_hi >= 2 && pow / 2 >= c->sw.r1_min_pow) {      // the next round stays rank-one: fold and its sums in one pass over T
            const u32 hn = 1u << (c->r1_hi - 2);
            const bool structured = sc_struct_round<C>(c, pow);
            // the first fold was deferred for the rows of st_f8x: this call is their SECOND fold -- straight from the 4-byte sources
            const bool second = c->defer_on;
            // ... or it is the first fold of a structured table and the next round will be of this kind too: defer what can be
            const bool defer = structured && c->sw.defer && c->r1_hi >= 3 && pow / 4 >= c->sw.r1_min_pow && c->st_f8.n > 0;
            REEF_TRY(sc_r1_prep<C>(c, &rr, pow));
            const R1View<C> v(c);
            dim3 grid;
            u32 rpc;
            REEF_TRY(sc_r1_grid<C>(c, hn, &grid, &rpc));
            // the coefficients of THIS round are still in out3 and r is its challenge: sum t1 e1 of the next round follows from
            // the sum-check identity (REEF_SC_IDENTITY=0: all three sums are accumulated)
            const bool ident = prev_pow == pow && c->sw.identity;
            const fe256 *Tsrc = (const fe256 *)(c->fresh ? c->T0 : c->T).template as<fe256>();
            unsigned long long *part = c->r1acc.template as<unsigned long long>();
            u32 blocks = 0;
            auto general = [&](const u32 *list, u32 nlist, dim3 g, unsigned long long *out) {
                if (ident)
                    hipLaunchKernelGGL((k_sc_r1_fold_coeffs<ScCtx<C>::F, false>), g, dim3(256), 0, c->stream, Tsrc, c->T.template as<fe256>(), c->r1_lo, hn, list, nlist,
                                       rr, (const fe_limbs *)v.f0, (const fe_limbs *)v.f1, (const fe_limbs *)v.fd, (const fe256 *)v.fl, out);
                else
                    hipLaunchKernelGGL((k_sc_r1_fold_coeffs<ScCtx<C>::F, true>), g, dim3(256), 0, c->stream, Tsrc, c->T.template as<fe256>(), c->r1_lo, hn, list, nlist,
                                       rr, (const fe_limbs *)v.f0, (const fe_limbs *)v.f1, (const fe_limbs *)v.fd, (const fe256 *)v.fl, out);
            };
            if (structured) {
                // rows whose four sources are constant or small: 4-byte reads; the few others through the dense kernel
                const u32 *lists = c->st_lists.template as<u32>();
                fe_limbs *ka = c->st_k.template as<fe_limbs>(), *kc = ka + hn;
                u32 *smask = reinterpret_cast<u32 *>(kc + hn);
                const dim3 gf = sc_list_grid<C>(c, c->st_fast.n), gg = sc_list_grid<C>(c, c->st_gen.n);
                hipLaunchKernelGGL(k_sc_r1_kprep<ScCtx<C>::F>, dim3(ceil_div(hn, 256)), dim3(256), 0, c->stream, (const fe256 *)c->T0.template as<fe256>(),
                                   (const u32 *)c->st_flags.template as<u32>(), c->r1_lo, hn, rr, ka, kc, smask);
                if (defer) {
                    // sums of the next round from the structure; rows of st_f8x are not written (their second fold will write a
                    // quarter-size table from the sources), the other fast rows and the general ones as before
                    const dim3 gr = sc_list_grid<C>(c, c->st_frest.n);
                    size_t nblk = (size_t)gr.x * gr.y + (size_t)gg.x * gg.y;
                    for (u32 b = 0; b < 4; ++b) {
                        const dim3 gs = sc_list_grid<C>(c, c->st_d8[b][0].n);
                        nblk += (c->st_d8[b][0].n ? (size_t)gs.x * gs.y : 0) + 4 * (size_t)ceil_div(c->st_d8[b][1].n, 256);   // the merged launch has 4 x the largest set's blocks at most
                    }
                    auto cs = [&](auto kernel, const typename ScCtx<C>::StList &L, dim3 g) {
                        hipLaunchKernelGGL(kernel, g, dim3(256), 0, c->stream, (const u32 *)c->st_s32.template as<u32>(), c->T.template as<fe256>(), c->r1_lo, hn,
                                           lists + L.off, L.n, rr, (const fe_limbs *)ka, (const fe_limbs *)kc, (const u32 *)smask, (const fe_limbs *)v.f0,
                                           (const fe_limbs *)v.f1, (const fe_limbs *)v.fd, (const fe256 *)v.fl, part);
                        blocks += g.x * g.y;
                    };
                    // the deferred rows: their share of the next round's sums straight from the pristine rows, block by block, with
                    // the scaled row factors -- 18 multiply-adds per 4-byte entry, no t' anywhere
                    {
                        fe_limbs *fa4 = reinterpret_cast<fe_limbs *>(smask + hn) + hn, *fd4 = fa4 + 4 * (size_t)hn;   // after K2A, K2C
                        hipLaunchKernelGGL(k_sc_r2s_factors<ScCtx<C>::F>, dim3(ceil_div(hn, 256)), dim3(256), 0, c->stream, (const fe_limbs *)v.f0, (const fe_limbs *)v.f1,
                                           (const fe_limbs *)v.fd, hn, rr, fa4, fd4);
                        const fe256 *T0 = c->T0.template as<fe256>();
                        for (u32 b = 0; b < 4; ++b) {
                            const auto &S = c->st_d8[b][0];
                            const fe_limbs *fab = fa4 + (size_t)b * hn, *fdb = fd4 + (size_t)b * hn;
                            if (S.n) {
                                const dim3 gs = sc_list_grid<C>(c, S.n);
                                hipLaunchKernelGGL((k_sc_r1s_rows<ScCtx<C>::F, false>), gs, dim3(256), 0, c->stream, T0, (const u32 *)c->st_s32.template as<u32>(), c->r1_lo,
                                                   b * hn, b & 1u, lists + S.off, S.n, fab, fdb, (const fe256 *)v.fl, part);
                                blocks += gs.x * gs.y;
                            }
                        }
                        ScConstSets sets = {};
                        u32 kb = 0;
                        for (u32 b = 0; b < 4; ++b) {
                            const auto &K = c->st_d8[b][1];
                            sets.row_off[b] = b * hn; sets.side[b] = b & 1u; sets.nlist[b] = K.n; sets.list[b] = lists + K.off;
                            sets.fa[b] = fa4 + (size_t)b * hn; sets.fd[b] = fd4 + (size_t)b * hn;
                            kb = std::max(kb, ceil_div(K.n, 256));
                        }
                        if (kb) {
                            hipLaunchKernelGGL(k_sc_r1s_const<ScCtx<C>::F>, dim3(kb, 4), dim3(256), 0, c->stream, T0, c->r1_lo, sets,
                                               (const fe256 *)c->st_sumfl.template as<fe256>(), part);
                            blocks += 4 * kb;
                        }
                    }
                    if (c->st_frest.n) {
                        if (ident) cs(k_sc_r1_fold_coeffs_cs<ScCtx<C>::F, false, true>, c->st_frest, gr);
                        else cs(k_sc_r1_fold_coeffs_cs<ScCtx<C>::F, true, true>, c->st_frest, gr);
                    }
                    if (c->st_gen.n) {
                        general(lists + c->st_gen.off, c->st_gen.n, gg, part);
                        blocks += gg.x * gg.y;
                    }
                    if (c->r1_nq)                        // the few entries of t' the masses of the next round read
                        hipLaunchKernelGGL(k_sc_defer_points<ScCtx<C>::F>, dim3(ceil_div(2 * c->r1_nq, 256)), dim3(256), 0, c->stream, (const u32 *)c->st_s32.template as<u32>(),
                                           c->T.template as<fe256>(), c->r1_lo, hn, (u32)(pow / 2), (const u32 *)c->r1mq.template as<u32>(), c->r1_nq, rr,
                                           (const fe_limbs *)ka, (const fe_limbs *)kc, (const u32 *)smask);
                    c->defer_on = true;
                    c->defer_r1 = rr;
                    c->defer_pow = pow / 2;
                    c->defer_hq = hn;
                } else {
                if (c->st_fast.n) {
                    if (ident)
                        hipLaunchKernelGGL((k_sc_r1_fold_coeffs_cs<ScCtx<C>::F, false>), gf, dim3(256), 0, c->stream, (const u32 *)c->st_s32.template as<u32>(),
                                           c->T.template as<fe256>(), c->r1_lo, hn, lists + c->st_fast.off, c->st_fast.n, rr, (const fe_limbs *)ka, (const fe_limbs *)kc,
                                           (const u32 *)smask, (const fe_limbs *)v.f0, (const fe_limbs *)v.f1, (const fe_limbs *)v.fd, (const fe256 *)v.fl, part);
                    else
                        hipLaunchKernelGGL((k_sc_r1_fold_coeffs_cs<ScCtx<C>::F, true>), gf, dim3(256), 0, c->stream, (const u32 *)c->st_s32.template as<u32>(),
                                           c->T.template as<fe256>(), c->r1_lo, hn, lists + c->st_fast.off, c->st_fast.n, rr, (const fe_limbs *)ka, (const fe_limbs *)kc,
                                           (const u32 *)smask, (const fe_limbs *)v.f0, (const fe_limbs *)v.f1, (const fe_limbs *)v.fd, (const fe256 *)v.fl, part);
                    blocks += gf.x * gf.y;
                }
                if (c->st_gen.n) {
                    general(lists + c->st_gen.off, c->st_gen.n, gg, part);
                    blocks += gg.x * gg.y;
                }
                }
            } else if (second) {
                // hn = an eighth of the pristine rows = half of defer_hq: g < hn; st_f8 from the sources, st_g8 from the dense rows
                c->defer_on = false;
                const u32 hq = c->defer_hq;
                const u32 *lists = c->st_lists.template as<u32>();
                fe_limbs *ka = c->st_k.template as<fe_limbs>(), *kc = ka + hq;
                u32 *smask = reinterpret_cast<u32 *>(kc + hq);
                fe_limbs *k2a = reinterpret_cast<fe_limbs *>(smask + hq), *k2c = k2a + hn;
                const dim3 g8 = sc_list_grid<C>(c, c->st_f8.n), gg = sc_list_grid<C>(c, c->st_g8.n);
                hipLaunchKernelGGL(k_sc_r2_kprep<ScCtx<C>::F>, dim3(ceil_div(hn, 256)), dim3(256), 0, c->stream, (const fe_limbs *)ka, (const fe_limbs *)kc, hn, rr, k2a, k2c);
                if (ident)
                    hipLaunchKernelGGL((k_sc_r2_fold_coeffs_cs<ScCtx<C>::F, false>), g8, dim3(256), 0, c->stream, (const u32 *)c->st_s32.template as<u32>(), c->T.template as<fe256>(),
                                       c->r1_lo, hq, lists + c->st_f8.off, c->st_f8.n, c->defer_r1, rr, (const fe_limbs *)k2a, (const fe_limbs *)k2c, (const u32 *)smask,
                                       (const fe_limbs *)v.f0, (const fe_limbs *)v.f1, (const fe_limbs *)v.fd, (const fe256 *)v.fl, part);
                else
                    hipLaunchKernelGGL((k_sc_r2_fold_coeffs_cs<ScCtx<C>::F, true>), g8, dim3(256), 0, c->stream, (const u32 *)c->st_s32.template as<u32>(), c->T.template as<fe256>(),
                                       c->r1_lo, hq, lists + c->st_f8.off, c->st_f8.n, c->defer_r1, rr, (const fe_limbs *)k2a, (const fe_limbs *)k2c, (const u32 *)smask,
                                       (const fe_limbs *)v.f0, (const fe_limbs *)v.f1, (const fe_limbs *)v.fd, (const fe256 *)v.fl, part);
                blocks += g8.x * g8.y;
                if (c->st_g8.n) {
                    general(lists + c->st_g8.off, c->st_g8.n, gg, part);
                    blocks += gg.x * gg.y;
                }
            } else {
                general(nullptr, 0, grid, part);
                blocks = grid.x * grid.y;
            }
            c->fresh = false;
            c->valid_t = c->valid_e = pow;
            return sc_r1_finish<C>(c, blocks, pow / 2, out3_host, ident ? &rr : nullptr);
        }
        // last rank-one round (FH bits used up, or the tables are small now): fold T, write the live entries of EQ out, and
        // take the next sums with the dense kernel
        REEF_TRY(sc_r1_prep<C>(c, &rr, pow));
        const u32 fb = (u32)std::min<size_t>(4096, std::max<size_t>(1, ceil_div(pow, 256)));
        hipLaunchKernelGGL(k_sc_r1_fold<ScCtx<C>::F>, dim3(fb), dim3(256), 0, c->stream, (const fe256 *)(c->fresh ? c->T0 : c->T).template as<fe256>(),
                           c->T.template as<fe256>(), (u32)pow, rr);
        c->fresh = false;
        c->valid_t = c->valid_e = pow;
        REEF_TRY(sc_r1_materialize<C>(c));
        const u32 cb = sc_dense_blocks<C>(c, pow / 2);
        const bool one = sc_one_launch<C>(c, cb);
        hipLaunchKernelGGL(k_sc_coeffs<ScCtx<C>::F>, dim3(cb), dim3(256), 0, c->stream, (const fe256 *)c->T.template as<fe256>(),
                           (const fe256 *)c->E.template as<fe256>(), (u32)(pow / 2), c->partial.template as<unsigned long long>(),
                           one ? c->gacc.template as<unsigned long long>() : nullptr, c->pinned3, one ? ++c->seq : 0u, c->sw.order);
        return sc_dense_finish<C>(c, one, cb, out3_host);
    }
    if (c->r1) REEF_TRY(sc_r1_materialize<C>(c));
    c->valid_t = c->valid_e = pow;
    if (c->sw.one_launch && pow / 2 <= c->sw.split_max) {   // a small round: an item over four waves, always one launch
        const u32 sb = (u32)std::min<size_t>(c->sw.split_blocks, std::max<size_t>(1, ceil_div(pow / 2, 64)));
        hipLaunchKernelGGL(k_sc_fold_coeffs_split<ScCtx<C>::F>, dim3(sb), dim3(256), 0, c->stream, (const fe256 *)(c->fresh ? c->T0 : c->T).template as<fe256>(),
                           c->T.template as<fe256>(), c->E.template as<fe256>(), (u32)pow, rr, c->gacc.template as<unsigned long long>(), c->pinned3, ++c->seq, c->sw.order);
        c->fresh = false;
        return sc_dense_finish<C>(c, true, sb, out3_host);
    }
    const u32 blocks = sc_dense_blocks<C>(c, pow / 2);
    const bool one = sc_one_launch<C>(c, blocks);
    hipLaunchKernelGGL(k_sc_fold_coeffs<ScCtx<C>::F>, dim3(blocks), dim3(256), 0, c->stream, (const fe256 *)(c->fresh ? c->T0 : c->T).template as<fe256>(),
                       c->T.template as<fe256>(), c->E.template as<fe256>(), (u32)pow, rr, c->partial.template as<unsigned long long>(),
                       one ? c->gacc.template as<unsigned long long>() : nullptr, c->pinned3, one ? ++c->seq : 0u, c->sw.order);
    c->fresh = false;
    return sc_dense_finish<C>(c, one, blocks, out3_host);
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
    if (hi_bits >= 1 && c->sw.rank1 && c->len / 2 >= c->sw.r1_min_pow) {
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
        hipLaunchKernelGGL(k_sc_eq_table<ScCtx<C>::F>, dim3((u32)std::min<size_t>(4096, ceil_div(c->len, 256))), dim3(256), 0, c->stream, fac_hi, fac_lo,
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
