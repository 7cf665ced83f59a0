// Host side of the per-curve MSM engine (resident key, workspace, kernel pipeline).
// Included by kernels_pallas.hip / kernels_vesta.hip after msm_kernels.inc with
// REEF_CURVE defined; exports one CurveVTable.
#include <algorithm>
#include <atomic>
#include <mutex>
#include <string.h>
#include <vector>

#include "common.h"
#include "glv_host.h"
#include "host_combine.h"

namespace reef {

static_assert(sizeof(fe256) == sizeof(reef_fe), "fe256 layout");
static_assert(sizeof(affine256) == sizeof(reef_affine), "affine256 layout");
static_assert(sizeof(jacobian256) == sizeof(reef_jacobian), "jacobian256 layout");
static_assert(sizeof(xyzz_mem) == 144, "xyzz_mem layout");

static_assert(sizeof(xyzz_mem) == XYZZ_BYTES && sizeof(u32x2) == ENTRY_BYTES, "msm_plan.h sizes the workspace with these");

static constexpr u32 DEFAULT_L0 = 0;   // chunk length chosen per call (msm_plan.h, with the pipeline's other constants)

static inline u32 windows_for(u32 c) { return (256 + c - 1) / c; }

// Relative cost model (unit: one mixed add) used to pick the window size.
static u32 choose_window(size_t n, u32 groups_mode /*0 = G=W, else G*/) {
    if (groups_mode == 1) {
        // Pre-shifted key, one bucket set: measured on MI355X (tools/sweep_plans.py, profiles/r02_latency_sweep.txt).  Below
        // ~2^16 points the MSM is a latency chain whose length barely depends on the window (c = 13 wins from 2^12 to 2^15);
        // above, the accumulation dominates and the fewest digits win until the bucket reduction catches up at c = 17.
        // Thresholds re-measured in round 5 between the powers of two, one MSM in flight and four (tools/sweep_window_mid.py,
        // profiles/r05_window_mid_sweep.txt): since the tail kernels share their group operations over four waves the
        // smaller windows hold out longer (was 49152 / 98304: c = 17 cost 5 % at 98304..163840 points).
        return n < 61440 ? 13u : n < 180224 ? 15u : 17u;
    }
    u32 best_c = 4;
    double best = 1e300;
    for (u32 c = 3; c <= 20; ++c) {
        const u32 W = windows_for(c);
        const u32 G = groups_mode == 0 ? W : std::min(groups_mode, W);
        const double nb = (double)(1u << (c - 1));
        // expected non-zero digits per 255-bit scalar: full windows, plus the top one (carry only
        // when 255 is a multiple of c)
        const double digits = (double)(255 / c) + ((255 % c) == 0 ? 0.5 : 1.0);
        // fitted to tools/sweep_plans.py on MI355X: with one bucket group the reduction is a
        // latency chain (heavier per bucket); with G groups it runs G-wide in parallel
        const double cost = digits * (double)n + (G == 1 ? 10.0 : 4.0) * G * nb;
        if (cost < best) { best = cost; best_c = c; }
    }
    return best_c;
}

template <int C> struct Key {
    affine256 *tables = nullptr;  // T tables of n points each
    size_t n = 0, cap = 0;     // points per table, allocated points per table
    u32 c = 0, W = 0, G = 0, T = 0;
    affine_limbs *limb_tables = nullptr;   // the same T * n points in the accumulation loop's own form (ec.h: affine_limbs, 128 B each), for k_accum0 alone;
    size_t limb_cap = 0;                   // null: the loop reads `tables` (plain, nibble- and byte-table keys; no room on the device).  limb_cap: allocated records
    affine256 *small_tab = nullptr;   // nibble tables of a small pre-shifted key (k_small_msm), 960 points per key point
    size_t small_n = 0;               // points the nibble tables cover (0: none)
    affine256 *wide_tab = nullptr;    // byte tables of a mid-size pre-shifted key (k_wide_accum), 4096 points per key point
    std::atomic<size_t> wide_n{0};    // points the byte tables cover (0: none yet); published when the build has finished
    std::atomic<int> wide_state{0};   // 0: none, 1: being built on wide_stream, 2: ready
    hipStream_t wide_stream = nullptr;   // the tables are built in the background, on a stream of the key's own
    hipEvent_t wide_event = nullptr;
    void *wide_stage = nullptr;       // window bases while the build runs
    int *wide_abort = nullptr;        // host-mapped flag the build kernels read: set to 1, the levels still queued return at once
    std::mutex wide_mu;
    std::atomic<int> refs{1};
    int device = 0;
};

template <int C> struct Ctx {
    Key<C> *key = nullptr;
    hipStream_t stream = nullptr;              // the pool stream the ctx is on (common.h: StreamLease); valid between ctx_enter and the next idle()
    StreamLease lease;
    std::mutex mu;
    u32 opt_c = 0, opt_G = 0, L0 = DEFAULT_L0, opt_tables = 0;
    // grow-only workspace (steady state allocates nothing)
    DevBuf scalars, blinds, hpoint, result, tmp_xyzz, maxbits;          // staged inputs, results, key-build scratch
    DevBuf dig, counts, tile_sums, bstart, entries;                     // digits, sort histograms, bucket starts, sorted entries
    DevBuf bstart1, seg_first, seg_counts, entries1;                    // two-level sort: coarse bins, segment plan, coarse-sorted entries
    DevBuf bucket_acc, lkeys[2], lvals[2];                              // bucket sums and the partial-sum lists of k_accum0 / k_accumN
    DevBuf rowcol, group_sums;                                          // bucket reduction: row/column sums, one sum per bucket group
    // Ring of HIP-event quads (start, accum0 begin, accum0 end, end), one quad per call, so that
    // per-kernel time can be summed over a whole timed region without a host sync per call.
    static constexpr int EV_RING = 32;
    hipEvent_t evr[EV_RING][4] = {};
    bool ev_pending[EV_RING] = {};
    int ev_next = 0, ev_last = -1;
    hipEvent_t *ev = nullptr;  // quad of the call being recorded
    double sum_total_ms = 0, sum_accum_ms = 0;
    u64 timed_calls = 0;
    jacobian256 *pinned = nullptr;            // host-mapped landing zone for small host-bound results (no copy kernel, one sync)
    static constexpr size_t PINNED_POINTS = 64;
    bool timing = false;
    DevBuf sym_table, sym_tmp, sym_u8;        // block tables of the tiny-scalar row commit (cached per ctx)
    u32 sym_bits = 0, sym_k = 0, sym_row_len = 0;
    u32 symw_bits = 0, symw_planes = 0, symw_row_len = 0;   // the same buffers holding the plane tables of wide symbols instead (0: they do not)
    int two_level = -1;                       // sort: -1 by size, 0 never, 1 whenever the window allows (REEF_MSM_SORT2 overrides)
    u32 wsplit_rank = 0, wsplit_world = 1;   // window split across GPUs (reef_msm_ctx_set_window_split)
    DevBuf h_tab, small_partial;             // nibble table of the blinding generator last used, partial sums of k_small_msm
    DevBuf wide_dig, wide_partial;           // byte-table path: signed byte digits, partial sums (two levels)
    reef_affine h_cached = {};               // the generator h_tab was built for
    const reef_affine *h_host = nullptr;     // the caller's host copy of h during a call with host buffers (spares a read-back)
    bool h_valid = false;
    bool coop = true;                        // tail kernels with four waves per group operation (ec_coop.h); REEF_MSM_COOP=0: one wave
    DevBuf wsum;                             // coop bucket reduction: weighted and plain sums of the rows / columns per group
    DevBuf deep_dig, deep_part;              // deep fold (v_fold_deep): the coefficients' digits, window sums and folded points
    int rowcol_force = -1;                   // row / column sums of a coop ctx: -1 by the rule (rowcol_lanes), 0 always four waves per sum, 16 / 32 / 64 always
                                             // that many lanes per sum (REEF_MSM_ROWCOL)
    u64 rowcol_calls[2] = {};                // MSMs of a coop ctx whose row / column sums took the latency form [0] / the throughput form [1]
    // hipGraphs of the bucket pipeline, one per (scalars pointer, result pointer, launch plan, ...) this ctx keeps seeing (REEF_MSM_GRAPH=1)
    struct GraphEntry {
        const void *scalars; void *out; bool is_mont; u32 wr, ww; CoreLaunch plan; uint64_t gen; int seen;
        hipGraph_t graph; hipGraphExec_t exec;
    };
    std::vector<GraphEntry> graphs;
    Ctx<C> *side = nullptr;                  // a small plain key of this ctx's own for the one-off points of reef_ipa_check (ipa_check_engine.inc)
    Ctx<C> *side_batch = nullptr;            // the same for reef_ipa_check_batch: sized to the largest batch seen, grow-only
    hipEvent_t batch_ev[4] = {};             // a timed batch: S pass begin / end on this ctx's stream, one-off points begin / end on the second
    bool batch_timed = false;                // the last batch ran with timing on
};
// Every entry point that enqueues work holds one of these (under ctx->mu, with the key's device current): the ctx takes the
// pool stream with the fewest callers at work unless work of its own is still in flight.  When the call returns -- with its
// results waited for, with work in flight (device outputs), or with an error half-way -- the stream itself says whether the
// ctx is idle again and free to take another stream next time; if not, the ctx stays where its work is.
template <int C> struct CtxScope {
    Ctx<C> *ctx;
    explicit CtxScope(Ctx<C> *c) : ctx(c) {}
    reef_status enter() { return ctx->lease.enter(ctx->key->device, &ctx->stream); }
    ~CtxScope() {
        if (!ctx->lease.counted) return;
        if (hipStreamQuery(ctx->stream) == hipSuccess) ctx->lease.idle();
        else (void)hipGetLastError();                  // hipErrorNotReady is not an error
    }
};
template <int C> static void graphs_clear(Ctx<C> *ctx) {
    for (auto &e : ctx->graphs) {
        if (e.exec) (void)hipGraphExecDestroy(e.exec);
        if (e.graph) (void)hipGraphDestroy(e.graph);
    }
    ctx->graphs.clear();
}

template <int C> static reef_status ctx_harvest(Ctx<C> *ctx, int slot) {
    if (!ctx->ev_pending[slot]) return REEF_OK;
    REEF_HIP_TRY(hipEventSynchronize(ctx->evr[slot][3]));
    float t = 0, a = 0;
    REEF_HIP_TRY(hipEventElapsedTime(&t, ctx->evr[slot][0], ctx->evr[slot][3]));
    REEF_HIP_TRY(hipEventElapsedTime(&a, ctx->evr[slot][1], ctx->evr[slot][2]));
    ctx->sum_total_ms += t;
    ctx->sum_accum_ms += a;
    ctx->timed_calls += 1;
    ctx->ev_pending[slot] = false;
    return REEF_OK;
}
template <int C> static reef_status ctx_begin_timing(Ctx<C> *ctx) {
    const int slot = ctx->ev_next;
    REEF_TRY(ctx_harvest<C>(ctx, slot));  // long finished by the time the ring wraps
    ctx->ev = ctx->evr[slot];
    ctx->ev_last = slot;
    ctx->ev_next = (slot + 1) % Ctx<C>::EV_RING;
    return REEF_OK;
}

// Stops a build in flight and frees everything the byte tables hold.  The levels of a build are queued all at once; they read
// the key's abort flag (host-mapped) when they start, so the wait below is for the level that is running, not for the build.
template <int C> static void wide_drop(Key<C> *k) {
    if (k->wide_abort) *(volatile int *)k->wide_abort = 1;
    if (k->wide_stream) (void)hipStreamSynchronize(k->wide_stream);
    if (k->wide_event) { (void)hipEventDestroy(k->wide_event); k->wide_event = nullptr; }
    if (k->wide_stream) { (void)hipStreamDestroy(k->wide_stream); k->wide_stream = nullptr; }
    if (k->wide_stage) { (void)hipFree(k->wide_stage); k->wide_stage = nullptr; }
    if (k->wide_tab) { (void)hipFree(k->wide_tab); k->wide_tab = nullptr; }
    if (k->wide_abort) { (void)hipHostFree(k->wide_abort); k->wide_abort = nullptr; }
    k->wide_n.store(0);
    k->wide_state.store(0);
}
template <int C> static void key_release(Key<C> *k) {
    if (k && --k->refs == 0) {
        if (k->tables) (void)hipFree(k->tables);
        if (k->limb_tables) (void)hipFree(k->limb_tables);
        if (k->small_tab) (void)hipFree(k->small_tab);
        wide_drop(k);
        delete k;
    }
}

static reef_status set_lds_limit(const void *fn) {
    REEF_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(MAX_LDS_KEYS * sizeof(u32))));
    return REEF_OK;
}

static reef_status engine_init_once() {
    static std::once_flag once;
    static reef_status st = REEF_OK;
    std::call_once(once, [] {
        auto f = []() -> reef_status {
            REEF_TRY(set_lds_limit((const void *)k_count));
            REEF_TRY(set_lds_limit((const void *)k_recode_count<REEF_CURVE>));
            REEF_TRY(set_lds_limit((const void *)k_scatter<false>));
            REEF_TRY(set_lds_limit((const void *)k_scatter<true>));
            REEF_TRY(set_lds_limit((const void *)k_row_count));
            REEF_TRY(set_lds_limit((const void *)k_row_scatter));
            return REEF_OK;
        };
        st = f();
    });
    return st;
}

static reef_status plan_for(size_t n, uint32_t c_opt, uint32_t g_opt, uint32_t *c, uint32_t *w, uint32_t *g, uint32_t *t);

// ---- small keys: nibble tables (k_shift_chain + k_small_fill / k_small_msm) ----
static inline size_t small_table_points(size_t n) { return (size_t)SMALL_WINDOWS * SMALL_DIGITS * n; }
// pts: n points in key-table form on the device -> out: their nibble tables (enqueued on the ctx's stream)
template <int C> static reef_status small_build(Ctx<C> *ctx, const affine256 *pts, size_t n, affine256 *out) {
    const size_t tp = small_table_points(n), nb = (size_t)SMALL_WINDOWS * n;
    REEF_TRY(ctx->tmp_xyzz.ensure((tp + nb) * sizeof(xyzz_mem)));
    xyzz_mem *mult = ctx->tmp_xyzz.template as<xyzz_mem>(), *base = mult + tp;
    hipLaunchKernelGGL(k_shift_chain<C>, dim3(ceil_div(n, 64)), dim3(64), 0, ctx->stream, pts, (u32)n, 4u, SMALL_WINDOWS, 1, base);
    hipLaunchKernelGGL(k_small_fill<C>, dim3(ceil_div(nb, 64)), dim3(64), 0, ctx->stream, (const xyzz_mem *)base, (u32)n, mult);
    hipLaunchKernelGGL((k_xyzz_normalize<C, false>), dim3(ceil_div(ceil_div(tp, NORM_PER), 256)), dim3(256), 0, ctx->stream, (const xyzz_mem *)mult, (u32)tp,
                       out);
    REEF_HIP_TRY(hipGetLastError());
    return REEF_OK;
}
// Nibble table of the blinding generator h (ABI affine, host or device), rebuilt only when h changes.  h_tab holds the
// table, two staging points of the host path, the copy of h and the flag the device path compares against, and the
// scratch of k_h_refresh.
template <int C> struct HTab {
    affine256 *tab, *raw, *imp, *dev_cached;
    u32 *dev_valid;
    xyzz_mem *scratch;
    static size_t bytes() { return (small_table_points(1) + 4) * sizeof(affine256) + (SMALL_WINDOWS + small_table_points(1)) * sizeof(xyzz_mem); }
    explicit HTab(const DevBuf &b) {
        tab = b.template as<affine256>();
        raw = tab + small_table_points(1);
        imp = raw + 1;
        dev_cached = raw + 2;
        dev_valid = reinterpret_cast<u32 *>(raw + 3);
        scratch = reinterpret_cast<xyzz_mem *>(raw + 4);
    }
};
template <int C> static reef_status ensure_h_table(Ctx<C> *ctx, const reef_affine *h, int loc) {
    if (ctx->h_tab.cap < HTab<C>::bytes()) {
        REEF_TRY(ctx->h_tab.ensure(HTab<C>::bytes()));
        ctx->h_valid = false;
        REEF_HIP_TRY(hipMemsetAsync(HTab<C>(ctx->h_tab).dev_valid, 0, sizeof(affine256), ctx->stream));
    }
    const HTab<C> t(ctx->h_tab);
    if (loc == REEF_DEVICE) {
        // no host round trip: the comparison and, when h changed, the rebuild run on the device in stream order
        // (HyraxPC.commit with device buffers stays asynchronous)
        hipLaunchKernelGGL(k_h_refresh<C>, dim3(1), dim3(64), 0, ctx->stream, reinterpret_cast<const affine256 *>(h), t.dev_cached, t.dev_valid,
                           t.scratch, t.tab);
        REEF_HIP_TRY(hipGetLastError());
        ctx->h_valid = false;                 // the table may no longer be the one built for h_cached
        return REEF_OK;
    }
    reef_affine hv;
    memcpy(&hv, h, sizeof hv);
    if (ctx->h_valid && memcmp(&hv, &ctx->h_cached, sizeof hv) == 0) return REEF_OK;
    REEF_HIP_TRY(hipMemsetAsync(t.dev_valid, 0, sizeof(u32), ctx->stream));     // the device path's copy goes stale with the table
    REEF_HIP_TRY(hipMemcpyAsync(t.raw, &hv, sizeof hv, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_import_key<C>, dim3(1), dim3(256), 0, ctx->stream, t.raw, 1u, t.imp);
    REEF_TRY(small_build<C>(ctx, t.imp, 1, t.tab));
    REEF_HIP_TRY(hipStreamSynchronize(ctx->stream));                  // hv is a stack variable
    ctx->h_cached = hv;
    ctx->h_valid = true;
    return REEF_OK;
}
// out += blinds[r] * h for `rows` results already on the device
template <int C>
static reef_status launch_blind(Ctx<C> *ctx, jacobian256 *d_out, const fe256 *d_blinds, const affine256 *d_h, bool is_mont, size_t rows) {
    if (ctx->h_host) REEF_TRY(ensure_h_table<C>(ctx, ctx->h_host, REEF_HOST));
    else REEF_TRY(ensure_h_table<C>(ctx, (const reef_affine *)d_h, REEF_DEVICE));
    hipLaunchKernelGGL(k_add_blind_tab<C>, dim3(ceil_div(rows * BLIND_LANES, 64)), dim3(64), 0, ctx->stream, d_out, d_blinds, ctx->h_tab.template as<affine256>(),
                       (int)is_mont, (u32)rows);
    return REEF_OK;
}
// sum_i scalars[i] * key[i] (+ blind * h) through the nibble tables: one or two launches, result at d_out (device or host-mapped)
template <int C>
static reef_status run_small(Ctx<C> *ctx, const fe256 *d_scalars, size_t n, bool is_mont, const fe256 *d_blind, bool with_blind, jacobian256 *d_out) {
    Key<C> *key = ctx->key;
    SmallSeg s0{key->small_tab, d_scalars, (u32)key->small_n, (u32)n};
    SmallSeg s1{ctx->h_tab.template as<affine256>(), d_blind, 1u, with_blind ? 1u : 0u};
    const u32 total = SMALL_WINDOWS * (s0.n + s1.n);
    if (total == 0) { REEF_HIP_TRY(hipMemsetAsync(d_out, 0, sizeof(jacobian256), ctx->stream)); return REEF_OK; }
    const u32 blocks = ceil_div(total, SMALL_PER_BLOCK);
    if (ctx->timing) {
        REEF_TRY(ctx_begin_timing<C>(ctx));
        REEF_HIP_TRY(hipEventRecord(ctx->ev[0], ctx->stream));
        REEF_HIP_TRY(hipEventRecord(ctx->ev[1], ctx->stream));
    }
    if (blocks == 1) {
        hipLaunchKernelGGL(k_small_msm<C>, dim3(1), dim3(256), 0, ctx->stream, s0, s1, (int)is_mont, (xyzz_mem *)nullptr, d_out);
    } else {
        REEF_TRY(ctx->small_partial.ensure((size_t)blocks * sizeof(xyzz_mem)));
        hipLaunchKernelGGL(k_small_msm<C>, dim3(blocks), dim3(256), 0, ctx->stream, s0, s1, (int)is_mont, ctx->small_partial.template as<xyzz_mem>(),
                           (jacobian256 *)nullptr);
        hipLaunchKernelGGL(k_small_final<C>, dim3(1), dim3(256), 0, ctx->stream, ctx->small_partial.template as<xyzz_mem>(), blocks, d_out);
    }
    if (ctx->timing) {
        REEF_HIP_TRY(hipEventRecord(ctx->ev[2], ctx->stream));
        REEF_HIP_TRY(hipEventRecord(ctx->ev[3], ctx->stream));
        ctx->ev_pending[ctx->ev_last] = true;
    }
    REEF_HIP_TRY(hipGetLastError());
    return REEF_OK;
}
static inline bool small_path(const void *small_tab, size_t small_n, size_t n, u32 wsplit_world) {
    return small_tab && n <= small_n && wsplit_world <= 1;
}

// ---- mid-size keys: byte tables (k_wide_fill / k_wide_accum) ----
static inline size_t wide_table_points(size_t n) { return (size_t)WIDE_WINDOWS * WIDE_DIGITS * n; }
// Largest key that gets byte tables: 2^16 points (16 GiB) unless REEF_MSM_WIDE_MAX_LOG says otherwise (0: none).  The tables
// are also skipped when the device has not twice their size free.
static inline size_t wide_n_max() {
    static const size_t v = [] {
        const char *e = getenv("REEF_MSM_WIDE_MAX_LOG");
        const int lg = e ? atoi(e) : 16;
        return lg <= 0 ? (size_t)0 : (size_t)1 << std::min(lg, 20);
    }();
    return v;
}
// Which keys get byte tables: pre-shifted keys of 1025 .. 2^REEF_MSM_WIDE_MAX_LOG points that ASK for them -- opts.byte_tables = 1
// (built inside reef_msm_ctx_create) or 3 (built in the background on a low-priority stream of the key's own; the bucket
// pipeline serves the key until they are ready and every call looks whether they are: wide_poll).  opts.byte_tables = 0 follows
// the process-wide policy: none, unless REEF_MSM_WIDE=1 opts every eligible key into the background build; 2 = never.
// REEF_MSM_WIDE=0 refuses the tables to every key.  They are opt-in because they are expensive -- 256 KiB per point (8.6 GB for
// 2^15 points), 14-38 ms of building -- for 0.1 ms per MSM, and because a background build is not free when the GPU is busy:
// measured on the drop-in symbol, calls on a 2^16-point key took 3.4 ms instead of 0.7 ms while its tables were being built
// (profiles/r03_stateless_pcie_inclusive.txt).  A long-lived prover that keeps its keys pays once and should ask.
static inline bool wide_enabled(u32 opt_tables) {
    static const int env = [] { const char *e = getenv("REEF_MSM_WIDE"); return e ? atoi(e) : -1; }();
    if (env == 0 || opt_tables == 2) return false;
    return opt_tables == 1 || opt_tables == 3 || (opt_tables == 0 && env == 1);
}
// Enqueues the table build of `n` points (key table form, ready in memory) on stream st: base = staging of 32 n XYZZ + 32 n
// affine points.
template <int C> static reef_status wide_build(hipStream_t st, const affine256 *pts, size_t n, void *stage_, affine256 *out, const int *abort_flag) {
    // window bases 256^w * P_i: one chain of doublings per point, one normalisation, then into the d = 1 rows of the table
    const size_t nb = (size_t)WIDE_WINDOWS * n;
    xyzz_mem *stage = (xyzz_mem *)stage_;
    affine256 *base = (affine256 *)(stage + nb);
    hipLaunchKernelGGL(k_shift_chain<C>, dim3(ceil_div(n, 64)), dim3(64), 0, st, pts, (u32)n, 8u, WIDE_WINDOWS, 1, stage);
    hipLaunchKernelGGL((k_xyzz_normalize<C, false>), dim3(ceil_div(ceil_div(nb, NORM_PER), 256)), dim3(256), 0, st, (const xyzz_mem *)stage, (u32)nb, base);
    for (u32 w = 0; w < WIDE_WINDOWS; ++w)
        REEF_HIP_TRY(hipMemcpyAsync(out + (size_t)w * WIDE_DIGITS * n, base + (size_t)w * n, n * sizeof(affine256), hipMemcpyDeviceToDevice, st));
    // seven doubling levels, in place and in affine form: W[m + j] = W[m] + W[j], inversions shared by Montgomery's trick
    for (u32 m = 1; m < WIDE_DIGITS; m <<= 1) {
        const u64 adds = (u64)WIDE_WINDOWS * m * n;
        hipLaunchKernelGGL(k_wide_level<C>, dim3((u32)ceil_div(ceil_div(adds, (u64)WIDE_LEVEL_K), 256)), dim3(256), 0, st, out, (u32)n, m, abort_flag);
    }
    REEF_HIP_TRY(hipGetLastError());
    return REEF_OK;
}
static inline bool wide_path(const void *wide_tab, size_t wide_n, size_t n, u32 wsplit_world) {
    return wide_tab && n <= wide_n && wsplit_world <= 1;
}
// Starts the background build for a freshly built key (key->tables complete and synchronised).  No room on the device, or an
// ineligible key: nothing happens and the bucket pipeline keeps the key.
template <int C> static reef_status wide_start(Key<C> *key, u32 opt_tables) {
    const size_t n = key->n;
    if (!wide_enabled(opt_tables) || key->G != 1 || n <= SMALL_N_MAX || n > wide_n_max()) return REEF_OK;
    std::lock_guard<std::mutex> lk(key->wide_mu);
    const size_t bytes = wide_table_points(n) * sizeof(affine256);
    const size_t stage_bytes = (size_t)WIDE_WINDOWS * n * (sizeof(xyzz_mem) + sizeof(affine256));
    size_t free_b = 0, total_b = 0;
    REEF_HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (free_b < 2 * bytes + (size_t(8) << 30)) return REEF_OK;
    if (hipMalloc((void **)&key->wide_tab, bytes) != hipSuccess || hipMalloc(&key->wide_stage, stage_bytes) != hipSuccess) {
        (void)hipGetLastError();
        wide_drop(key);
        return REEF_OK;
    }
    int lo = 0, hi = 0;
    REEF_HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));                 // lo = the numerically largest = the lowest priority
    REEF_HIP_TRY(hipStreamCreateWithPriority(&key->wide_stream, hipStreamNonBlocking, lo));
    REEF_HIP_TRY(hipEventCreateWithFlags(&key->wide_event, hipEventDisableTiming));
    REEF_HIP_TRY(hipHostMalloc((void **)&key->wide_abort, sizeof(int), hipHostMallocDefault));
    *key->wide_abort = 0;
    REEF_TRY(wide_build<C>(key->wide_stream, key->tables, n, key->wide_stage, key->wide_tab, key->wide_abort));
    REEF_HIP_TRY(hipEventRecord(key->wide_event, key->wide_stream));
    key->wide_state.store(1, std::memory_order_release);
    return REEF_OK;
}
// Publishes the tables once the build has finished (wait: block until it has).  Cheap when there is nothing to do.
template <int C> static void wide_poll(Key<C> *key, bool wait = false) {
    if (key->wide_state.load(std::memory_order_acquire) != 1) return;
    std::lock_guard<std::mutex> lk(key->wide_mu);
    if (key->wide_state.load(std::memory_order_acquire) != 1) return;
    if (wait) (void)hipEventSynchronize(key->wide_event);
    else if (hipEventQuery(key->wide_event) != hipSuccess) { (void)hipGetLastError(); return; }
    if (key->wide_stage) { (void)hipFree(key->wide_stage); key->wide_stage = nullptr; }
    key->wide_n.store(key->n, std::memory_order_release);
    key->wide_state.store(2, std::memory_order_release);
}
// table entries per thread of k_wide_accum: one wave per SIMD while 16 entries per thread cover the input, two beyond (the chain
// is what costs here); REEF_MSM_WIDE_PER overrides (experiments)
static inline u32 wide_per(u64 total) {
    static const u32 per_env = [] { const char *e = exp_env("REEF_MSM_WIDE_PER"); return e ? (u32)atoi(e) : 0u; }();
    u32 per = (u32)std::max<u64>(4, ceil_div(total, 65536));
    if (per > 16) per = (u32)std::max<u64>(16, ceil_div(total, 131072));
    return per_env ? per_env : per;
}
// d_out = sum_i scalars[i] * key[i] from the byte tables
template <int C>
static reef_status run_wide(Ctx<C> *ctx, const fe256 *d_scalars, size_t n, bool is_mont, jacobian256 *d_out) {
    Key<C> *key = ctx->key;
    hipStream_t st = ctx->stream;
    const u64 total = (u64)WIDE_WINDOWS * n;
    const u32 per = wide_per(total);
    const u32 wgs = (u32)ceil_div(total, (u64)256 * per);
    REEF_TRY(ctx->wide_dig.ensure(total * sizeof(short)));
    const u32 lvl2 = ceil_div(wgs, 64);
    REEF_TRY(ctx->wide_partial.ensure(((size_t)wgs + lvl2) * sizeof(xyzz_mem)));
    xyzz_mem *p1 = ctx->wide_partial.template as<xyzz_mem>(), *p2 = p1 + wgs;
    if (ctx->timing) {
        REEF_TRY(ctx_begin_timing<C>(ctx));
        REEF_HIP_TRY(hipEventRecord(ctx->ev[0], st));
    }
    hipLaunchKernelGGL(k_wide_recode<C>, dim3(ceil_div(n, 256)), dim3(256), 0, st, d_scalars, (u32)n, (int)is_mont, ctx->wide_dig.template as<short>());
    if (ctx->timing) REEF_HIP_TRY(hipEventRecord(ctx->ev[1], st));
    hipLaunchKernelGGL((k_wide_accum<C, false>), dim3(wgs), dim3(256), 0, st, (const affine256 *)key->wide_tab, (u32)key->wide_n.load(),
                       (const short *)ctx->wide_dig.template as<short>(), (u32)n, per, 0u, p1);
    if (ctx->timing) REEF_HIP_TRY(hipEventRecord(ctx->ev[2], st));
    const xyzz_mem *last = p1;
    u32 cnt = wgs;
    if (cnt > 512) {                                   // k_small_final takes up to 512 partial sums in one workgroup
        hipLaunchKernelGGL(k_wide_reduce<C>, dim3(lvl2), dim3(256), 0, st, (const xyzz_mem *)p1, cnt, p2);
        last = p2;
        cnt = lvl2;
    }
    hipLaunchKernelGGL(k_small_final<C>, dim3(1), dim3(256), 0, st, last, cnt, d_out);
    if (ctx->timing) {
        REEF_HIP_TRY(hipEventRecord(ctx->ev[3], st));
        ctx->ev_pending[ctx->ev_last] = true;
    }
    REEF_HIP_TRY(hipGetLastError());
    return REEF_OK;
}

// -------------------------------------------------------------- key setup ----
// Which keys get a second copy of their tables in the accumulation loop's form (Key::limb_tables: 128 B per table point beside the
// packed 64 B, so a key's device memory triples): pre-shifted keys that the bucket pipeline serves.  Not plain keys (T = 1: their
// tables are as often as not rebuilt per call), not keys served from nibble or byte tables, not the keys of the drop-in symbols'
// process-wide table (tl_packed_tables_only).  REEF_MSM_LIMB_TABLES=0 (experiment build) keeps every key packed, for A/B runs.
static inline bool limb_tables_wanted(size_t n, u32 G, u32 T, u32 opt_tables) {
    if (n == 0 || T <= 1 || (u64)T * n >= (1ull << 31) || tl_packed_tables_only) return false;
    if (G == 1 && (n <= SMALL_N_MAX || (wide_enabled(opt_tables) && n <= wide_n_max()))) return false;
    const char *e = exp_env("REEF_MSM_LIMB_TABLES");
    return !(e && atoi(e) == 0);
}
template <int C>
static reef_status key_build(Ctx<C> *ctx, const reef_affine *bases, size_t n, int loc) {
    Key<C> *key = ctx->key;
    u32 c, W, G, T;
    REEF_TRY(plan_for(n, ctx->opt_c, ctx->opt_G, &c, &W, &G, &T));
    wide_drop(key);                                    // byte tables of the previous bases; a build in flight reads key->tables
    const size_t need = (size_t)T * std::max<size_t>(n, 1);
    if (need > key->cap) {
        if (key->tables) { (void)hipFree(key->tables); key->tables = nullptr; key->cap = 0; }
        REEF_HIP_TRY(hipMalloc((void **)&key->tables, need * sizeof(affine256)));
        key->cap = need;
    }
    key->n = n; key->c = c; key->W = W; key->G = G; key->T = T;
    ctx->sym_bits = ctx->symw_bits = 0;   // block tables belong to the previous bases
    graphs_clear(ctx);   // captured launches read the previous tables and plan
    const bool limbs = limb_tables_wanted(n, G, T, ctx->opt_tables);
    if (key->limb_tables && (!limbs || need > key->limb_cap)) { (void)hipFree(key->limb_tables); key->limb_tables = nullptr; key->limb_cap = 0; }
    if (limbs && !key->limb_tables) {                  // no room for them is never fatal: the loop reads the packed tables then
        if (hipMalloc((void **)&key->limb_tables, need * sizeof(affine_limbs)) == hipSuccess) key->limb_cap = need;
        else { (void)hipGetLastError(); key->limb_tables = nullptr; }
    }
    if (n == 0) return REEF_OK;
    // ABI points -> key-table form (internal Montgomery radix, canonical): one pass, once per key
    const affine256 *src = (const affine256 *)bases;
    // all shifted tables are built in one chain per point and one normalisation; in batches when the XYZZ staging would pass 1 GiB
    const u32 per_batch = T > 1 ? (u32)std::max<size_t>(1, std::min<size_t>(T - 1, (size_t(1) << 30) / (n * sizeof(xyzz_mem)))) : 1;
    // staging: the XYZZ points of the shift chain (pre-shifted keys only), the nibble tables' scratch, and the raw upload of host bases.  A PLAIN key (T = 1)
    // needs the last alone: 64 B per point, not 144 -- rounds 1-5 sized it for a chain that never runs, which put a 2^20-point plain key's staging above the
    // release threshold below: 144 MiB allocated and freed again on EVERY call of the drop-in symbols' plain path (hipFree alone: 1.2 ms).
    size_t staging_bytes = T > 1 ? (size_t)per_batch * n * sizeof(xyzz_mem) : 0;
    if (G == 1 && n <= SMALL_N_MAX) staging_bytes = std::max(staging_bytes, (small_table_points(n) + (size_t)SMALL_WINDOWS * n) * sizeof(xyzz_mem));
    if (loc != REEF_DEVICE) staging_bytes = std::max(staging_bytes, n * sizeof(affine256));
    REEF_TRY(ctx->tmp_xyzz.ensure(std::max<size_t>(staging_bytes, 16)));     // sized once, before anything reads it
    if (loc != REEF_DEVICE) {
        REEF_HIP_TRY(hipMemcpyAsync(ctx->tmp_xyzz.p, bases, n * sizeof(affine256), hipMemcpyHostToDevice, ctx->stream));
        src = ctx->tmp_xyzz.template as<affine256>();
    }
    hipLaunchKernelGGL(k_import_key<C>, dim3(ceil_div(n, 256)), dim3(256), 0, ctx->stream, src, (u32)n, key->tables);
    if (T > 1) {
        for (u32 j = 1; j < T; j += per_batch) {
            const u32 cnt = std::min(per_batch, T - j);
            hipLaunchKernelGGL(k_shift_chain<C>, dim3(ceil_div(n, 64)), dim3(64), 0, ctx->stream, key->tables + (size_t)(j - 1) * n, (u32)n, c * G, cnt, 0,
                               ctx->tmp_xyzz.template as<xyzz_mem>());
            hipLaunchKernelGGL((k_xyzz_normalize<C, false>), dim3(ceil_div(ceil_div((size_t)cnt * n, NORM_PER), 256)), dim3(256), 0, ctx->stream,
                               ctx->tmp_xyzz.template as<xyzz_mem>(), (u32)((size_t)cnt * n), key->tables + (size_t)j * n);
        }
    }
    if (key->limb_tables)                              // every table in the loop's form, from the packed ones, once
        hipLaunchKernelGGL(k_limb_tables<C>, dim3(ceil_div((size_t)T * n, 256)), dim3(256), 0, ctx->stream, (const affine256 *)key->tables, (u32)((size_t)T * n),
                           key->limb_tables);
    key->small_n = 0;
    if (G == 1 && n <= SMALL_N_MAX) {   // a small resident commitment key: nibble tables for the sort-free path (k_small_msm)
        if (key->small_tab) { (void)hipFree(key->small_tab); key->small_tab = nullptr; }
        REEF_HIP_TRY(hipMalloc((void **)&key->small_tab, small_table_points(n) * sizeof(affine256)));
        REEF_TRY(small_build<C>(ctx, key->tables, n, key->small_tab));
        key->small_n = n;
    }
    REEF_HIP_TRY(hipGetLastError());
    REEF_HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->tmp_xyzz.cap > (size_t(96) << 20)) ctx->tmp_xyzz.release();   // the shift chain's staging goes; a plain key's upload buffer (72 MiB at 2^20 points) stays for the next call
    if (wide_start<C>(key, ctx->opt_tables) != REEF_OK) {                  // byte tables: built in the background from here on
        (void)hipGetLastError();                                           // never fatal: the bucket pipeline serves the key
        wide_drop(key);
    }
    if (ctx->opt_tables == 1) wide_poll<C>(key, true);
    return REEF_OK;
}

template <int C> static void ctx_free(Ctx<C> *ctx) {
    if (!ctx) return;
    ctx_free(ctx->side);
    ctx_free(ctx->side_batch);
    for (auto &e : ctx->batch_ev)
        if (e) (void)hipEventDestroy(e);
    graphs_clear(ctx);
    for (DevBuf *b : {&ctx->scalars, &ctx->blinds, &ctx->hpoint, &ctx->dig, &ctx->counts, &ctx->bstart, &ctx->bstart1, &ctx->seg_first,
                      &ctx->seg_counts, &ctx->entries1, &ctx->sym_table, &ctx->sym_tmp, &ctx->sym_u8, &ctx->tile_sums,
                      &ctx->entries, &ctx->bucket_acc, &ctx->rowcol, &ctx->group_sums, &ctx->result,
                      &ctx->tmp_xyzz, &ctx->maxbits, &ctx->wsum, &ctx->deep_dig, &ctx->deep_part, &ctx->h_tab, &ctx->small_partial, &ctx->wide_dig, &ctx->wide_partial, &ctx->lkeys[0], &ctx->lkeys[1], &ctx->lvals[0], &ctx->lvals[1]})
        b->release();
    for (auto &q : ctx->evr)
        for (auto &e : q)
            if (e) (void)hipEventDestroy(e);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    ctx->lease.idle();                                  // the streams belong to the pool
    ctx->lease.unpin();
    stream_pool().context_destroyed();
    key_release(ctx->key);
    delete ctx;
}

// A ctx for `*device` (opts->device, or the caller's current device when that is -1), without changing the caller's
// current device.
template <int C> static reef_status ctx_new(Ctx<C> **out, const reef_msm_opts *opts, int *device) {
    REEF_TRY(engine_init_once());
    int dev = -1;
    if (opts && opts->device >= 0) dev = opts->device;
    else REEF_HIP_TRY(hipGetDevice(&dev));
    int ndev = 0;
    REEF_HIP_TRY(hipGetDeviceCount(&ndev));
    if (dev < 0 || dev >= ndev) { set_error("device %d out of range (%d visible)", dev, ndev); return REEF_ERR_ARG; }
    REEF_ON_DEVICE(dev);
    Ctx<C> *ctx = new Ctx<C>();
    if (const char *e = exp_env("REEF_MSM_SORT2")) ctx->two_level = atoi(e);   // tuning knob: -1 by size (default), 0 off, 1 on
    if (const char *e = exp_env("REEF_MSM_COOP")) ctx->coop = atoi(e) != 0;
    if (const char *e = exp_env("REEF_MSM_ROWCOL")) {  // A/B: 0 = the four-wave row / column sums always, 16 / 32 / 64 = that many lanes per sum always
        const int v = atoi(e);
        if (v == 0 || v == 16 || v == 32 || v == 64) ctx->rowcol_force = v;
    }
    if (opts) {
        ctx->opt_c = opts->window_bits;
        ctx->opt_G = opts->bucket_groups;
        if (opts->chunk) ctx->L0 = opts->chunk;
        ctx->opt_tables = opts->byte_tables;
    }
    {
        const reef_status st = stream_pool().context_created(dev);   // the pool grows here, at creation time, not in a hot call
        if (st != REEF_OK) { stream_pool().context_destroyed(); delete ctx; return st; }
    }
    *out = ctx;   // no stream yet: the ctx takes one from the pool when it first has work (CtxScope)   // the timing events are created by the first reef_msm_ctx_enable_timing (128 hipEventCreate cost ~7 ms)
    *device = dev;
    return REEF_OK;
}

template <int C>
static reef_status v_ctx_create(void **impl, const reef_affine *bases, size_t n, int loc, const reef_msm_opts *opts) {
    if (!impl || (n && !bases)) { set_error("null argument"); return REEF_ERR_ARG; }
    REEF_TRY(plan_for(n, opts ? opts->window_bits : 0, opts ? opts->bucket_groups : 0, nullptr, nullptr, nullptr, nullptr));
    Ctx<C> *ctx = nullptr;
    int dev = -1;
    REEF_TRY(ctx_new<C>(&ctx, opts, &dev));
    ctx->key = new Key<C>();
    ctx->key->device = dev;
    REEF_ON_DEVICE(dev);
    reef_status st;
    {
        CtxScope<C> scope(ctx);
        st = scope.enter();
        if (st == REEF_OK) st = key_build<C>(ctx, bases, n, loc);
    }
    if (st != REEF_OK) { ctx_free(ctx); return st; }
    *impl = ctx;
    return REEF_OK;
}

template <int C> static reef_status v_ctx_rekey(void *impl, const reef_affine *bases, size_t n, int loc) {
    Ctx<C> *ctx = (Ctx<C> *)impl;
    if (!ctx || (n && !bases)) { set_error("null argument"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->key->refs.load() != 1) { set_error("rekey on a shared key"); return REEF_ERR_ARG; }
    REEF_ON_DEVICE(ctx->key->device);
    CtxScope<C> scope(ctx);
    REEF_TRY(scope.enter());
    return key_build<C>(ctx, bases, n, loc);
}

template <int C> static reef_status v_ctx_clone(void **impl, void *src_) {
    Ctx<C> *src = (Ctx<C> *)src_;
    reef_msm_opts o = {};
    o.window_bits = src->opt_c; o.bucket_groups = src->opt_G; o.chunk = src->L0; o.byte_tables = src->opt_tables; o.device = src->key->device;
    Ctx<C> *ctx = nullptr;
    int dev = -1;
    REEF_TRY(ctx_new<C>(&ctx, &o, &dev));
    ctx->key = src->key;
    ++ctx->key->refs;
    ctx->wsplit_rank = src->wsplit_rank;
    ctx->wsplit_world = src->wsplit_world;
    ctx->coop = src->coop;
    ctx->rowcol_force = src->rowcol_force;
    *impl = ctx;
    return REEF_OK;
}

// ctx becomes a handle on src's key -- what a clone of src would be -- keeping its own stream and workspace: for callers with
// many keys and few threads (the drop-in symbols' per-thread context, api.cpp).  Waits for the work already enqueued on ctx.
template <int C> static reef_status v_ctx_attach(void *impl, void *src_) {
    Ctx<C> *ctx = (Ctx<C> *)impl, *src = (Ctx<C> *)src_;
    if (ctx == src || ctx->key == src->key) return REEF_OK;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->key->device != src->key->device) { set_error("attach: the two keys live on different devices"); return REEF_ERR_ARG; }
    REEF_ON_DEVICE(ctx->key->device);
    if (ctx->lease.counted) {                           // work of the previous key still in flight
        REEF_HIP_TRY(hipStreamSynchronize(ctx->stream));
        ctx->lease.idle();
    }
    Key<C> *old = ctx->key;
    ctx->key = src->key;
    ++ctx->key->refs;
    key_release(old);
    ctx->opt_c = src->opt_c; ctx->opt_G = src->opt_G; ctx->opt_tables = src->opt_tables;
    ctx->wsplit_rank = src->wsplit_rank;
    ctx->wsplit_world = src->wsplit_world;
    ctx->sym_bits = ctx->symw_bits = 0;   // block tables and captured launches belong to the previous key
    graphs_clear(ctx);
    return REEF_OK;
}

template <int C> static int v_ctx_byte_tables(void *impl) {
    Ctx<C> *ctx = (Ctx<C> *)impl;
    if (!ctx || !ctx->key) return 0;
    DeviceGuard dg(ctx->key->device);
    if (!dg.ok) return 0;
    wide_poll<C>(ctx->key);
    return ctx->key->wide_n.load(std::memory_order_acquire) ? 1 : 0;
}
template <int C> static void v_ctx_destroy(void *impl) {
    Ctx<C> *ctx = (Ctx<C> *)impl;
    if (ctx && ctx->lease.counted) (void)hipStreamSynchronize(ctx->stream);
    ctx_free(ctx);
}
template <int C> static reef_status v_ctx_sync(void *impl) {
    Ctx<C> *ctx = (Ctx<C> *)impl;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->lease.counted && !ctx->lease.pinned) return REEF_OK;   // nothing in flight: every earlier call has been waited for
    REEF_HIP_TRY(hipStreamSynchronize(ctx->stream));                 // (a stream that was handed out may carry the caller's own work)
    ctx->lease.idle();
    return REEF_OK;
}
// The stream is handed out (RCCL / torch work is ordered after it): from here on the ctx stays on it.
template <int C> static void *v_ctx_stream(void *impl) {
    Ctx<C> *ctx = (Ctx<C> *)impl;
    std::lock_guard<std::mutex> lk(ctx->mu);
    DeviceGuard dg(ctx->key->device);
    if (!dg.ok) { set_error("cannot make device %d current: %s", ctx->key->device, hipGetErrorString(dg.err)); return nullptr; }
    if (ctx->lease.pin(ctx->key->device, &ctx->stream) != REEF_OK) return nullptr;
    return (void *)ctx->stream;
}
template <int C> static reef_status v_ctx_timing(void *impl, float *total_ms, float *acc_ms) {
    Ctx<C> *ctx = (Ctx<C> *)impl;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (ctx->ev_last < 0) { set_error("no timed call yet (reef_msm_ctx_enable_timing first)"); return REEF_ERR_ARG; }
    hipEvent_t *q = ctx->evr[ctx->ev_last];
    REEF_HIP_TRY(hipEventSynchronize(q[3]));
    if (total_ms) REEF_HIP_TRY(hipEventElapsedTime(total_ms, q[0], q[3]));
    if (acc_ms) REEF_HIP_TRY(hipEventElapsedTime(acc_ms, q[1], q[2]));
    return REEF_OK;
}
template <int C> static reef_status v_ctx_enable_timing(void *impl, int on) {
    Ctx<C> *ctx = (Ctx<C> *)impl;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (on && !ctx->evr[0][0]) {
        REEF_ON_DEVICE(ctx->key->device);
        for (auto &q : ctx->evr)
            for (auto &ev : q) REEF_HIP_TRY(hipEventCreate(&ev));
    }
    ctx->timing = on != 0;
    return REEF_OK;
}
template <int C> static reef_status v_ctx_window_split(void *impl, uint32_t rank, uint32_t world) {
    Ctx<C> *ctx = (Ctx<C> *)impl;
    if (world == 0 || rank >= world) { set_error("window split: rank %u of %u", rank, world); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    ctx->wsplit_rank = rank;
    ctx->wsplit_world = world;
    return REEF_OK;
}
// Sums over every call since the last reset (syncs with the calls still in flight).
template <int C> static reef_status v_ctx_timing_stats(void *impl, int reset, uint64_t *calls, double *total_ms, double *acc_ms) {
    Ctx<C> *ctx = (Ctx<C> *)impl;
    std::lock_guard<std::mutex> lk(ctx->mu);
    for (int i = 0; i < Ctx<C>::EV_RING; ++i) REEF_TRY(ctx_harvest<C>(ctx, i));
    if (calls) *calls = ctx->timed_calls;
    if (total_ms) *total_ms = ctx->sum_total_ms;
    if (acc_ms) *acc_ms = ctx->sum_accum_ms;
    if (reset) { ctx->timed_calls = 0; ctx->sum_total_ms = ctx->sum_accum_ms = 0; }
    return REEF_OK;
}
template <int C> static reef_status v_ctx_rowcol_forms(void *impl, int reset, uint64_t *latency_calls, uint64_t *throughput_calls) {
    Ctx<C> *ctx = (Ctx<C> *)impl;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (latency_calls) *latency_calls = ctx->rowcol_calls[0];
    if (throughput_calls) *throughput_calls = ctx->rowcol_calls[1];
    if (reset) ctx->rowcol_calls[0] = ctx->rowcol_calls[1] = 0;
    return REEF_OK;
}
// Sum of n Jacobian points on the ctx's own stream (device buffers), e.g. right after an
// RCCL all-gather of per-rank partial MSMs that was ordered on the same stream.
template <int C> static reef_status v_ctx_sum_points(void *impl, const reef_jacobian *in, size_t n, reef_jacobian *out) {
    Ctx<C> *ctx = (Ctx<C> *)impl;
    if (!in || !out || n > 65536) { set_error("bad argument"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    REEF_ON_DEVICE(ctx->key->device);
    CtxScope<C> scope(ctx);
    REEF_TRY(scope.enter());
    hipLaunchKernelGGL(k_sum_points<C>, dim3(1), dim3(64), 0, ctx->stream, (const jacobian256 *)in, (u32)n, (jacobian256 *)out);
    REEF_HIP_TRY(hipGetLastError());
    return REEF_OK;
}
template <int C> static reef_status v_ctx_plan(void *impl, uint32_t *c, uint32_t *w, uint32_t *g, uint32_t *t) {
    Key<C> *k = ((Ctx<C> *)impl)->key;
    if (c) *c = k->c;
    if (w) *w = k->W;
    if (g) *g = k->G;
    if (t) *t = k->T;
    return REEF_OK;
}

// ------------------------------------------------------------ the pipeline ----
// One MSM through the buckets is a plan and four stages.  core_launch_plan (msm_plan.h: pure integer arithmetic, tested on the host)
// decides everything -- chunk length, sort levels and entry forms, scan route, fusions, merge levels, row / column split -- and sizes
// every workspace buffer; ensure_core_workspace grows what is too small BEFORE the first launch; launch_sort, launch_accumulate,
// launch_partial_merge and launch_reduce enqueue what the plan says and decide nothing.

// The experiment switches of the bucket pipeline (common.h: exp_env), read once per process.
static const CoreSwitches &core_switches() {
    static const CoreSwitches sw = [] {
        CoreSwitches s;
        auto off = [](const char *name) { const char *e = exp_env(name); return e && atoi(e) == 0; };
        s.fuse_merge = !off("REEF_MSM_FUSE_MERGE");        // 0: k_accum0 and the first merge level stay two kernels
        s.merge1 = !off("REEF_MSM_MERGE1");                // 0: slot-per-lane first merge level
        if (const char *e = exp_env("REEF_MSM_FUSE_MAX_CHUNKS")) s.fuse_max_chunks = (u32)atoi(e);
        s.fuse_recode = !off("REEF_MSM_FUSE_RECODE");      // 0: k_recode and k_count stay two kernels
        s.sort_compact = !off("REEF_MSM_SORT_COMPACT");    // 0: 8-byte entries between the two sort levels
        s.sort_word = !off("REEF_MSM_SORT_WORD");          // 0: 8-byte sorted entries
        // TIMING ONLY -- the result is garbage: 1 leaves the whole bucket reduction out, 2 its row / column sums only.  What a window would be
        // worth if its bucket reduction were free: the upper bound on anything a faster reduction can buy
        // (profiles/r06_free_reduction_bound.txt: VERDICT r5 item 3's kill criterion, measured before any kernel was written).
        if (const char *e = exp_env("REEF_MSM_SKIP_REDUCE")) s.skip_reduce = atoi(e);
        return s;
    }();
    return sw;
}

// Partial merge after k_accum0 (msm_plan.h: merge_plan): the two slots per chunk -> bucket sums.
template <int C>
static void launch_partial_merge(Ctx<C> *ctx, const MergePlan &m, u32 nchunks0, xyzz_mem *acc) {
    hipStream_t st = ctx->stream;
    u32 *keys[2] = {ctx->lkeys[0].template as<u32>(), ctx->lkeys[1].template as<u32>()};
    xyzz_mem *vals[2] = {ctx->lvals[0].template as<xyzz_mem>(), ctx->lvals[1].template as<xyzz_mem>()};
    if (m.first == MERGE_FIRST_COOP)
        hipLaunchKernelGGL((k_merge_chunks<C, true>), dim3(m.first_grid), dim3(256), 0, st, keys[0], vals[0], nchunks0, acc, keys[1], vals[1]);
    else if (m.first == MERGE_FIRST_PLAIN)
        hipLaunchKernelGGL((k_merge_chunks<C, false>), dim3(m.first_grid), dim3(256), 0, st, keys[0], vals[0], nchunks0, acc, keys[1], vals[1]);
    u32 cur = m.cur;
    for (u32 i = 0; i < m.nlevels; ++i, cur ^= 1) {
        const u32 len = m.len[i];
        if (ctx->coop) hipLaunchKernelGGL(k_accumN_coop<C>, dim3(ceil_div(len, 64)), dim3(256), 0, st, keys[cur], vals[cur], len, acc, keys[cur ^ 1], vals[cur ^ 1]);
        else hipLaunchKernelGGL(k_accumN<C>, dim3(ceil_div(len, 256)), dim3(256), 0, st, keys[cur], vals[cur], len, acc, keys[cur ^ 1], vals[cur ^ 1]);
    }
}

// The form the row / column sums of the bucket reduction take in this call: 0 = one four-wave workgroup per sum (k_reduce_rowcol_coop), else
// the lanes per sum of k_reduce_rowcol.  The four-wave form has the shortest chain (10 shared additions of 3.7 us) and issues 38.7 M VALU
// wave-instructions per MSM at c = 17; with 64 / 32 / 16 lanes per sum it is 27.1 / 17.2 / 13.0 M on a chain of 9 / 12 / 19 additions of
// 7.2 us.  A caller who waits for ONE MSM sees the chain; a device that other work fills sees only the issue slots: with three MSMs in
// flight every lane count beat the four-wave form in every run, 32 by the most (+1.4 %).  So that form runs where both hold: the bucket
// matrix is large (NB >= 2^16, plans with c >= 17: below, an MSM is a latency chain the IPA rounds wait for), and the device is shared at the
// moment of the launch: another caller is at work on it (profiles/r17_rowcol_forms.txt).  Work this ctx itself still has queued does NOT
// count: it is on the same stream, the new MSM runs after it and not beside it, so a lone caller that queues MSMs back to back would pay the
// longer chain in full.  (A caller counts from its first enqueue to the wait that finds it idle: a ctx whose device-side result was never
// waited for through the library still counts, and the rule then errs towards the throughput form.)  Both forms return the same group
// element.  A ctx without coop tails (REEF_MSM_COOP=0) keeps every tail on one wave: 64 lanes per sum.
template <int C> static int rowcol_lanes(const Ctx<C> *ctx, u32 NB) {
    if (!ctx->coop) return 64;
    if (ctx->rowcol_force >= 0) return ctx->rowcol_force;
    if (NB < ROWCOL_SHARED_MIN_BUCKETS) return 0;
    const bool shared = callers_at_work(ctx->key->device).load(std::memory_order_relaxed) > 1;   // this ctx counts as one
    return shared ? ROWCOL_SHARED_LANES : 0;
}

// The plan of one call: the shape, what the ctx adds (the form of the row / column sums as of now), the switches.
template <int C>
static reef_status core_plan(const Ctx<C> *ctx, const CorePlan &pl, bool group_sums_out, CoreLaunch *p) {
    const CoreCtxOpts o{ctx->L0, ctx->coop, ctx->two_level, rowcol_lanes<C>(ctx, 1u << (pl.c - 1)), group_sums_out};
    const char *why = nullptr;
    const reef_status rs = core_launch_plan(pl, o, core_switches(), p, &why);
    if (rs != REEF_OK) set_error("%s (%llu buckets, %llu digits)", why, (unsigned long long)p->groups_total * p->NB, (unsigned long long)p->Mmax);
    return rs;
}

// Every buffer the chain touches, sized before its first launch: a buffer that has to grow is freed and allocated here, not between
// two kernels of the chain (and not under an open graph capture).  Steady state allocates nothing.
template <int C> static reef_status ensure_core_workspace(Ctx<C> *ctx, const CoreBytes &b) {
    REEF_TRY(ctx->dig.ensure(b.dig));
    REEF_TRY(ctx->counts.ensure(b.counts));
    REEF_TRY(ctx->tile_sums.ensure(b.tile_sums));
    REEF_TRY(ctx->bstart.ensure(b.bstart));
    REEF_TRY(ctx->entries.ensure(b.entries));
    REEF_TRY(ctx->bstart1.ensure(b.bstart1));
    REEF_TRY(ctx->seg_first.ensure(b.seg_first));
    REEF_TRY(ctx->seg_counts.ensure(b.seg_counts));
    REEF_TRY(ctx->entries1.ensure(b.entries1));
    REEF_TRY(ctx->bucket_acc.ensure(b.bucket_acc));
    for (int i = 0; i < 2; ++i) {
        REEF_TRY(ctx->lkeys[i].ensure(b.lkeys[i]));
        REEF_TRY(ctx->lvals[i].ensure(b.lvals[i]));
    }
    REEF_TRY(ctx->rowcol.ensure(b.rowcol));
    REEF_TRY(ctx->group_sums.ensure(b.group_sums));
    REEF_TRY(ctx->wsum.ensure(b.wsum));
    return REEF_OK;
}

// ---- digits, then the counting sort by bucket: ctx->entries in bucket order, ctx->bstart the buckets' first entries
template <int C>
static void launch_sort(Ctx<C> *ctx, const CorePlan &pl, const CoreLaunch &p, const fe256 *d_scalars, bool is_mont) {
    hipStream_t st = ctx->stream;
    u32 *dig = ctx->dig.template as<u32>(), *bstart = ctx->bstart.template as<u32>(), *counts = ctx->counts.template as<u32>();
    u32 *tile_sums = ctx->tile_sums.template as<u32>();
    u32 *bstart_c = p.two_level ? ctx->bstart1.template as<u32>() : bstart;     // scan output of the (coarse) histogram pass
    void *entries = (void *)ctx->entries.template as<u32x2>();
    const u32 NBTc = p.NBTc, S = p.S;
    auto launch_recode = [&] {
        hipLaunchKernelGGL(k_recode<C>, dim3(ceil_div(p.N, 256)), dim3(256), 0, st, d_scalars, (u32)p.N, (int)is_mont, pl.c, pl.W, ctx->wsplit_rank,
                           ctx->wsplit_world, dig);
    };
    SortShape sh{};
    RowSortShape rsh{};
    u32 *totals_src = counts;
    if (!p.row_mode) {
        sh.n = pl.row_len; sh.B = pl.rows; sh.W = pl.W; sh.G = pl.G; sh.NB = p.NBc; sh.shift = p.shift; sh.KB = p.KB; sh.per = p.per;
        sh.NBT = NBTc; sh.row_len = 0; sh.n_ctx = pl.n_ctx; sh.L0 = p.L0;
        if (p.recode_fused) {
            hipLaunchKernelGGL(k_recode_count<C>, dim3(S), dim3(1024), p.KB * sizeof(u32), st, d_scalars, (int)is_mont, pl.c, ctx->wsplit_rank, ctx->wsplit_world, sh,
                               dig, counts);
        } else {
            launch_recode();
            hipLaunchKernelGGL(k_count, dim3(S, p.groups_total, p.P), dim3(1024), p.KB * sizeof(u32), st, dig, sh, counts);
        }
        totals_src = counts + (size_t)S * NBTc;
    } else {
        rsh.rows = pl.rows; rsh.row_len = pl.row_len; rsh.W = pl.W; rsh.G = pl.G; rsh.NB = p.NB;
        rsh.rows_per_block = p.rows_per_block; rsh.n_ctx = pl.n_ctx; rsh.L0 = p.L0;
        launch_recode();
        hipLaunchKernelGGL(k_row_count, dim3(ceil_div(pl.rows, p.rows_per_block)), dim3(1024), p.rows_per_block * p.keys_per_row * sizeof(u32), st, dig, rsh,
                           totals_src);
    }
    if (p.scan == SCAN_SMALL) {
        hipLaunchKernelGGL(k_scan_small, dim3(1), dim3(1024), 0, st, counts, S, NBTc, bstart_c);
    } else {
        const bool wave = p.scan == SCAN_WAVE;              // a wave per key, or a thread
        if (wave) hipLaunchKernelGGL(k_slice_totals_w, dim3(ceil_div(NBTc, 4)), dim3(256), 0, st, counts, S, NBTc, totals_src);
        else if (!p.row_mode) hipLaunchKernelGGL(k_slice_totals, dim3(ceil_div(NBTc, 256)), dim3(256), 0, st, counts, S, NBTc, totals_src);
        hipLaunchKernelGGL(k_scan_tiles, dim3(p.ntiles), dim3(SCAN_BLOCK), 0, st, totals_src, NBTc, bstart_c, tile_sums);
        hipLaunchKernelGGL(k_scan_tile_sums, dim3(1), dim3(1024), 0, st, tile_sums, p.ntiles, bstart_c + NBTc);
        if (wave) hipLaunchKernelGGL(k_scan_finish_w, dim3(ceil_div(NBTc, 4)), dim3(256), 0, st, bstart_c, tile_sums, counts, S, NBTc);
        else hipLaunchKernelGGL(k_scan_finish, dim3(ceil_div(NBTc, 256)), dim3(256), 0, st, bstart_c, tile_sums, counts, p.row_mode ? 0u : S, NBTc);
    }
    if (p.two_level) {
        // coarse bins into entries1, then each bin by its low key bits into entries; the entry forms (msm_plan.h) are template arguments
        auto two_level_sort = [&](auto compact, auto word) {
            constexpr bool COMPACT = decltype(compact)::value, WORD = decltype(word)::value;
            const void *e1 = (const void *)ctx->entries1.template as<u32x2>();
            u32 *seg_first = ctx->seg_first.template as<u32>(), *seg_counts = ctx->seg_counts.template as<u32>();
            const size_t fine_lds = p.fine * sizeof(u32);
            hipLaunchKernelGGL(k_scatter<COMPACT>, dim3(S, p.groups_total, p.P), dim3(1024), p.KB * sizeof(u32), st, dig, sh, counts, (void *)e1);
            hipLaunchKernelGGL(k_seg_plan, dim3(1), dim3(1024), 0, st, bstart_c, NBTc, seg_first);
            hipLaunchKernelGGL(k_fine_count<COMPACT>, dim3(p.nseg_max), dim3(1024), fine_lds, st, e1, bstart_c, seg_first, NBTc, p.shift, seg_counts);
            hipLaunchKernelGGL(k_fine_offsets, dim3(NBTc), dim3(p.fine), 0, st, bstart_c, seg_first, NBTc, p.shift, seg_counts, bstart);
            hipLaunchKernelGGL((k_fine_scatter<COMPACT, WORD>), dim3(p.nseg_max), dim3(1024), fine_lds, st, e1, bstart_c, seg_first, NBTc, p.shift, seg_counts, entries);
        };
        if (p.word_entries) two_level_sort(std::true_type{}, std::true_type{});
        else if (p.compact) two_level_sort(std::true_type{}, std::false_type{});
        else two_level_sort(std::false_type{}, std::false_type{});
    } else if (!p.row_mode) {
        hipLaunchKernelGGL(k_scatter<false>, dim3(S, p.groups_total, p.P), dim3(1024), p.KB * sizeof(u32), st, dig, sh, counts, entries);
    } else {
        hipLaunchKernelGGL(k_row_scatter, dim3(ceil_div(pl.rows, p.rows_per_block)), dim3(1024), p.rows_per_block * p.keys_per_row * sizeof(u32), st, dig, rsh,
                           bstart, ctx->entries.template as<u32x2>());
    }
}

// ---- bucket accumulation: a chunk of L0 sorted entries per thread; k_accum0's (first merge level fused, one-word entries, table form)
template <int C> static void launch_accumulate(Ctx<C> *ctx, const CoreLaunch &p) {
    hipStream_t st = ctx->stream;
    const bool fused = p.merge.fused, word = p.word_entries;
    const u32 NBT = p.NBT, L0 = p.L0, nchunks0 = p.nchunks0;
    const dim3 ag(ceil_div(nchunks0, 256)), ab(256);
    const void *ent = (const void *)ctx->entries.template as<u32x2>();
    const u32 *bend = ctx->bstart.template as<u32>() + NBT;
    xyzz_mem *bacc = ctx->bucket_acc.template as<xyzz_mem>();
    u32 *ok = ctx->lkeys[fused ? 1 : 0].template as<u32>();
    xyzz_mem *ov = ctx->lvals[fused ? 1 : 0].template as<xyzz_mem>();
    auto launch_accum0 = [&](const auto *tables) {   // the key's packed tables, or its loop-form copy: the same indices
        using TABLE = std::remove_cv_t<std::remove_pointer_t<decltype(tables)>>;
        if (fused && word) hipLaunchKernelGGL((k_accum0<C, true, true, TABLE>), ag, ab, 0, st, tables, ent, bend, L0, nchunks0, bacc, ok, ov, NBT);
        else if (fused) hipLaunchKernelGGL((k_accum0<C, true, false, TABLE>), ag, ab, 0, st, tables, ent, bend, L0, nchunks0, bacc, ok, ov, 0u);
        else if (word) hipLaunchKernelGGL((k_accum0<C, false, true, TABLE>), ag, ab, 0, st, tables, ent, bend, L0, nchunks0, bacc, ok, ov, NBT);
        else hipLaunchKernelGGL((k_accum0<C, false, false, TABLE>), ag, ab, 0, st, tables, ent, bend, L0, nchunks0, bacc, ok, ov, 0u);
    };
    if (ctx->key->limb_tables) launch_accum0((const affine_limbs *)ctx->key->limb_tables);
    else launch_accum0((const affine256 *)ctx->key->tables);
}

// ---- bucket reduction (row/column sums, two short weighted sums), final Horner over groups
template <int C>
static void launch_reduce(Ctx<C> *ctx, const CorePlan &pl, const CoreLaunch &p, jacobian256 *d_out, const xyzz_mem **group_sums_out) {
    hipStream_t st = ctx->stream;
    const u32 c1 = p.c1, c2 = p.c2, groups_total = p.groups_total;
    const xyzz_mem *bacc = ctx->bucket_acc.template as<xyzz_mem>();
    const u32 *bstart = ctx->bstart.template as<u32>();
    xyzz_mem *rowcol = ctx->rowcol.template as<xyzz_mem>(), *wsum = ctx->wsum.template as<xyzz_mem>();
    xyzz_mem *gsum = ctx->group_sums.template as<xyzz_mem>();
    if (group_sums_out && ctx->pinned && (size_t)groups_total * sizeof(xyzz_mem) <= Ctx<C>::PINNED_POINTS * sizeof(jacobian256))
        gsum = (xyzz_mem *)ctx->pinned;                // host finishes the combine: let the kernel store where the host reads
    jacobian256 *direct_out = p.direct ? d_out : (jacobian256 *)nullptr;
    if (group_sums_out) *group_sums_out = gsum;        // the caller finishes the window combine on the host
    if (p.skip_reduce == 1) return;
    auto launch_rowcol = [&](auto lps) {
        constexpr int LPS = decltype(lps)::value;
        hipLaunchKernelGGL((k_reduce_rowcol<C, LPS>), dim3(ceil_div(ceil_div(p.rc_waves, 64u / LPS), 4)), dim3(256), 0, st, bacc, bstart, c1, c2, groups_total, rowcol);
    };
    if (ctx->coop) {
        const int lanes = p.rowcol_lanes;
        ++ctx->rowcol_calls[lanes != 0];
        if (p.skip_reduce == 2) {}
        else if (lanes == 16) launch_rowcol(std::integral_constant<int, 16>{});
        else if (lanes == 32) launch_rowcol(std::integral_constant<int, 32>{});
        else if (lanes == 64) launch_rowcol(std::integral_constant<int, 64>{});
        else hipLaunchKernelGGL(k_reduce_rowcol_coop<C>, dim3(p.rc_waves), dim3(256), 0, st, bacc, bstart, c1, c2, groups_total, rowcol);
        hipLaunchKernelGGL(k_reduce_weighted_coop<C>, dim3(groups_total, 2), dim3(256), 0, st, rowcol, c1, c2, wsum);
        hipLaunchKernelGGL(k_reduce_combine_coop<C>, dim3(groups_total), dim3(256), 0, st, wsum, c2, gsum, direct_out);
    } else {
        if (p.skip_reduce != 2) launch_rowcol(std::integral_constant<int, 64>{});
        hipLaunchKernelGGL(k_reduce_weighted<C>, dim3(groups_total), dim3(128), 0, st, rowcol, c1, c2, gsum, direct_out);
    }
    if (!group_sums_out && !p.direct) hipLaunchKernelGGL(k_final<C>, dim3(ceil_div(pl.rows, 64)), dim3(64), 0, st, gsum, pl.G, pl.c, pl.rows, d_out);
}

template <int C>
static reef_status run_core(Ctx<C> *ctx, const fe256 *d_scalars, const CorePlan &pl, const CoreLaunch &p, bool is_mont, const fe256 *d_blinds,
                            const affine256 *d_h, jacobian256 *d_out, const xyzz_mem **group_sums_out = nullptr) {
    hipStream_t st = ctx->stream;
    REEF_TRY(ensure_core_workspace<C>(ctx, p.bytes));
    if (ctx->timing) {
        REEF_TRY(ctx_begin_timing<C>(ctx));
        REEF_HIP_TRY(hipEventRecord(ctx->ev[0], st));
    }
    launch_sort<C>(ctx, pl, p, d_scalars, is_mont);
    if (ctx->timing) REEF_HIP_TRY(hipEventRecord(ctx->ev[1], st));
    launch_accumulate<C>(ctx, p);
    if (ctx->timing) REEF_HIP_TRY(hipEventRecord(ctx->ev[2], st));
    launch_partial_merge<C>(ctx, p.merge, p.nchunks0, ctx->bucket_acc.template as<xyzz_mem>());
    launch_reduce<C>(ctx, pl, p, d_out, group_sums_out);
    if (d_blinds && (ctx->wsplit_world <= 1 || ctx->wsplit_rank == 0))   // window split: the blind term belongs to one partial sum only
        REEF_TRY(launch_blind<C>(ctx, d_out, d_blinds, d_h, is_mont, pl.rows));
    if (ctx->timing) {
        REEF_HIP_TRY(hipEventRecord(ctx->ev[3], st));
        ctx->ev_pending[ctx->ev_last] = true;
    }
    REEF_HIP_TRY(hipGetLastError());
    return REEF_OK;
}
template <int C>
static reef_status run_core(Ctx<C> *ctx, const fe256 *d_scalars, const CorePlan &pl, bool is_mont, const fe256 *d_blinds,
                            const affine256 *d_h, jacobian256 *d_out, const xyzz_mem **group_sums_out = nullptr) {
    CoreLaunch p;
    REEF_TRY(core_plan<C>(ctx, pl, group_sums_out != nullptr, &p));
    return run_core<C>(ctx, d_scalars, pl, p, is_mont, d_blinds, d_h, d_out, group_sums_out);
}

// Where the kernels write `count` results: the caller's device buffer, the host-mapped landing zone
// (host-bound, few points: the final kernel stores straight into pinned host memory, so the host
// needs one stream sync and no copy), or device scratch followed by a copy.
template <int C>
static reef_status result_target(Ctx<C> *ctx, size_t count, reef_jacobian *out, int out_loc, jacobian256 **d_res) {
    if (out_loc == REEF_DEVICE) { *d_res = (jacobian256 *)out; return REEF_OK; }
    if (count <= Ctx<C>::PINNED_POINTS) {
        if (!ctx->pinned) REEF_HIP_TRY(hipHostMalloc((void **)&ctx->pinned, Ctx<C>::PINNED_POINTS * sizeof(jacobian256), hipHostMallocDefault));
        *d_res = ctx->pinned;
        return REEF_OK;
    }
    REEF_TRY(ctx->result.ensure(count * sizeof(jacobian256)));
    *d_res = ctx->result.template as<jacobian256>();
    return REEF_OK;
}
template <int C>
static reef_status finish_output(Ctx<C> *ctx, jacobian256 *d_res, size_t count, reef_jacobian *out, int out_loc) {
    if (out_loc == REEF_DEVICE) {
        if ((void *)d_res != (void *)out)
            REEF_HIP_TRY(hipMemcpyAsync(out, d_res, count * sizeof(jacobian256), hipMemcpyDeviceToDevice, ctx->stream));
        return REEF_OK;
    }
    if (d_res == ctx->pinned) {
        REEF_HIP_TRY(hipStreamSynchronize(ctx->stream));
        memcpy(out, ctx->pinned, count * sizeof(jacobian256));
        return REEF_OK;
    }
    REEF_HIP_TRY(hipMemcpyAsync(out, d_res, count * sizeof(jacobian256), hipMemcpyDeviceToHost, ctx->stream));
    REEF_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return REEF_OK;
}

// Group sums for a host-side window combine: already in host-mapped memory, or copied.
template <int C>
static reef_status fetch_group_sums(Ctx<C> *ctx, const xyzz_mem *gs, u32 G, std::vector<xyzz_mem> &hs) {
    hs.resize(G);
    if ((const void *)gs == (const void *)ctx->pinned) {
        REEF_HIP_TRY(hipStreamSynchronize(ctx->stream));
        memcpy(hs.data(), gs, G * sizeof(xyzz_mem));
        return REEF_OK;
    }
    REEF_HIP_TRY(hipMemcpyAsync(hs.data(), gs, G * sizeof(xyzz_mem), hipMemcpyDeviceToHost, ctx->stream));
    REEF_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return REEF_OK;
}

// The bucket pipeline of one MSM as a hipGraph (REEF_MSM_GRAPH=1; experiment, see DESIGN "tried").  A prover issues the same
// call again and again -- same staging buffer, same landing zone, same length -- so the chain of launches is captured the second
// time a call shape is seen and replayed from the third on: one hipGraphLaunch instead of 10-15 kernel launches.  Entries are
// dropped when any workspace buffer moves (g_devbuf_gen), on re-keying and with the ctx; timing events keep the plain path.
template <int C>
static reef_status run_core_graphed(Ctx<C> *ctx, const fe256 *d_scalars, const CorePlan &pl, bool is_mont, jacobian256 *d_out) {
    hipStream_t st = ctx->stream;
    const uint64_t gen = g_devbuf_gen.load();
    CoreLaunch plan;                                          // a captured chain IS one plan: the whole of it is part of the key, and the
    REEF_TRY(core_plan<C>(ctx, pl, false, &plan));            // plan compared here is the one run_core launches, at capture and at replay
    typename Ctx<C>::GraphEntry *hit = nullptr;
    for (size_t i = 0; i < ctx->graphs.size();) {
        auto &e = ctx->graphs[i];
        if (e.gen != gen) {                                   // its pointers may be stale
            if (e.exec) (void)hipGraphExecDestroy(e.exec);
            if (e.graph) (void)hipGraphDestroy(e.graph);
            ctx->graphs.erase(ctx->graphs.begin() + i);
            continue;
        }
        if (e.scalars == d_scalars && e.out == d_out && e.is_mont == is_mont && e.wr == ctx->wsplit_rank && e.ww == ctx->wsplit_world && same_plan(e.plan, plan)) hit = &e;
        ++i;
    }
    if (hit && hit->exec) {
        if (ctx->coop) ++ctx->rowcol_calls[plan.rowcol_lanes != 0];
        REEF_HIP_TRY(hipGraphLaunch(hit->exec, st));
        return REEF_OK;
    }
    if (hit && hit->seen == 1) {                              // second appearance: capture (the first run sized every buffer)
        // Contexts share the pool's streams: while a capture is open on `st`, kernels another thread's context (or a stateless call's
        // scratch) enqueues there would be RECORDED into this graph instead of run (ADVICE r4).  Capture only while this context is
        // the stream's sole user, and RESERVE the stream in the same atomic step (ADVICE r5: a check followed by a reservation let a
        // second caller in between): StreamPool::try_reserve is one compare-and-swap on the stream's user count, the pool hands a
        // reserved stream to nobody, and a context pinned to it waits the microseconds the capture lasts (common.h).  Otherwise this
        // call runs the plain path and the capture is tried again at the next one.
        PoolStream *ps = ctx->lease.ps;
        if (!ps || ctx->lease.bg || !stream_pool().try_reserve(ps, ctx->lease.pinned ? 1 : 0)) return run_core<C>(ctx, d_scalars, pl, plan, is_mont, nullptr, nullptr, d_out);
        hit->seen = 2;
        struct Reserve {                                      // until the capture has ended
            PoolStream *p;
            explicit Reserve(PoolStream *q) : p(q) {}
            ~Reserve() { StreamPool::unreserve(p); }
        } reserve(ps);
        if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            const reef_status rs = run_core<C>(ctx, d_scalars, pl, plan, is_mont, nullptr, nullptr, d_out);
            hipGraph_t g = nullptr;
            const hipError_t ee = hipStreamEndCapture(st, &g);
            if (rs == REEF_OK && ee == hipSuccess && g && g_devbuf_gen.load() == gen && hipGraphInstantiate(&hit->exec, g, nullptr, nullptr, 0) == hipSuccess) {
                hit->graph = g;
                REEF_HIP_TRY(hipGraphLaunch(hit->exec, st));
                return REEF_OK;
            }
            if (g) (void)hipGraphDestroy(g);
            hit->exec = nullptr;
            (void)hipGetLastError();
        } else {
            (void)hipGetLastError();
        }
        return run_core<C>(ctx, d_scalars, pl, plan, is_mont, nullptr, nullptr, d_out);   // capture refused: the plain path, from now on
    }
    REEF_TRY(run_core<C>(ctx, d_scalars, pl, plan, is_mont, nullptr, nullptr, d_out));
    if (!hit) {
        if (ctx->graphs.size() >= 4) {
            auto &v = ctx->graphs.front();
            if (v.exec) (void)hipGraphExecDestroy(v.exec);
            if (v.graph) (void)hipGraphDestroy(v.graph);
            ctx->graphs.erase(ctx->graphs.begin());
        }
        ctx->graphs.push_back({d_scalars, d_out, is_mont, ctx->wsplit_rank, ctx->wsplit_world, plan, g_devbuf_gen.load(), 1, nullptr, nullptr});
    }
    return REEF_OK;
}

// The window combine of a plain key (G > 1 bucket groups: sum_g 2^(c*g) S_g) for a result that STAYS ON THE DEVICE, without a host sync: the chain of ~255
// dependent doublings takes ~1 ms on one GPU wave whatever the size of the MSM (2^12 points: 1.32 ms against 0.24 on a pre-shifted key,
// profiles/r05_latency_sweep.txt) and 0.05-0.1 ms on a host core in arithmetic shaped for one (host_combine.h).  So the group sums land in host-mapped memory, a host function enqueued ON THE STREAM
// (hipLaunchHostFunc: it runs on a thread of the runtime when the stream reaches it; plain arithmetic, no HIP call inside) finishes the combine, and a 96-byte
// copy, again in stream order, puts the point where the caller asked for it.  The call only enqueues work, as before (include/reef_msm.h: reef_msm).
template <int C> struct HostCombineJob {
    const xyzz_mem *gs;      // G group sums, host-mapped
    u32 G, c;
    jacobian256 *res;        // host-mapped: where the copy that follows reads the point
};
template <int C> static void host_combine_fn(void *p) {
    HostCombineJob<C> *j = (HostCombineJob<C> *)p;
    *j->res = host_window_combine<C>(j->gs, j->G, j->c);     // host_combine.h: the group law on four 64-bit limbs
    delete j;
}
static inline bool host_combine_fits(u32 G) { return (size_t)G * sizeof(xyzz_mem) <= 62 * sizeof(jacobian256); }   // the landing zone's last slot is the result's

// sum_i scalars[i] * key[i] for scalars already on the device (ctx->mu held, n >= 1, d_res from result_target)
template <int C>
static reef_status msm_device_scalars(Ctx<C> *ctx, const fe256 *d_scalars, size_t n, bool is_mont, reef_jacobian *out, int out_loc, jacobian256 *d_res) {
    Key<C> *key = ctx->key;
    if (small_path(key->small_tab, key->small_n, n, ctx->wsplit_world)) {   // a small resident key: nibble tables, one or two launches
        REEF_TRY(run_small<C>(ctx, d_scalars, n, is_mont, nullptr, false, d_res));
        return finish_output<C>(ctx, d_res, 1, out, out_loc);
    }
    wide_poll<C>(key);                                 // have the byte tables become ready?
    if (wide_path(key->wide_tab, key->wide_n.load(std::memory_order_acquire), n, ctx->wsplit_world)) {   // a key of Reef's size: byte tables, no sort, no buckets
        REEF_TRY(run_wide<C>(ctx, d_scalars, n, is_mont, d_res));
        return finish_output<C>(ctx, d_res, 1, out, out_loc);
    }
    CorePlan pl{key->c, key->W, key->G, 1u, (u32)n, (u32)key->n};
    // REEF_MSM_HOST_COMBINE=0 keeps the combine on the device (k_final): measured in profiles/r02_host_combine.txt
    static const bool host_combine = !(getenv("REEF_MSM_HOST_COMBINE") && atoi(getenv("REEF_MSM_HOST_COMBINE")) == 0);
    if (out_loc != REEF_DEVICE && pl.G > 1 && host_combine) {
        // Result goes to the host anyway: the window combine sum_g 2^(c*g) S_g is a chain of ~255
        // dependent doublings -- ~1 ms on one GPU lane, 0.05-0.1 ms on a host core (host_combine.h).
        const xyzz_mem *gs = nullptr;
        REEF_TRY(run_core<C>(ctx, d_scalars, pl, is_mont, nullptr, nullptr, d_res, &gs));
        std::vector<xyzz_mem> hs;
        REEF_TRY(fetch_group_sums<C>(ctx, gs, pl.G, hs));
        const jacobian256 j = host_window_combine<C>(hs.data(), pl.G, pl.c);
        memcpy(out, &j, sizeof j);
        return REEF_OK;
    }
    if (out_loc == REEF_DEVICE && pl.G > 1 && host_combine && host_combine_fits(pl.G)) {
        if (!ctx->pinned) REEF_HIP_TRY(hipHostMalloc((void **)&ctx->pinned, Ctx<C>::PINNED_POINTS * sizeof(jacobian256), hipHostMallocDefault));
        const xyzz_mem *gs = nullptr;
        REEF_TRY(run_core<C>(ctx, d_scalars, pl, is_mont, nullptr, nullptr, d_res, &gs));
        if ((const void *)gs == (const void *)ctx->pinned) {
            jacobian256 *res = ctx->pinned + (Ctx<C>::PINNED_POINTS - 1);
            HostCombineJob<C> *job = new HostCombineJob<C>{gs, pl.G, pl.c, res};
            const hipError_t e = hipLaunchHostFunc(ctx->stream, host_combine_fn<C>, job);     // the job is the function's from here on
            if (e != hipSuccess) { delete job; REEF_HIP_TRY(e); }
            REEF_HIP_TRY(hipMemcpyAsync(out, res, sizeof(jacobian256), hipMemcpyHostToDevice, ctx->stream));
            if (ctx->timing) REEF_HIP_TRY(hipEventRecord(ctx->ev[3], ctx->stream));       // the call's end is the copy's, not the last kernel's (run_core recorded it there)
            return REEF_OK;
        }
        hipLaunchKernelGGL(k_final<C>, dim3(1), dim3(64), 0, ctx->stream, gs, pl.G, pl.c, 1u, d_res);      // (the group sums did not fit the landing zone)
        REEF_HIP_TRY(hipGetLastError());
        return finish_output<C>(ctx, d_res, 1, out, out_loc);
    }
    static const bool use_graphs = getenv("REEF_MSM_GRAPH") && atoi(getenv("REEF_MSM_GRAPH")) != 0;
    if (use_graphs && !ctx->timing && pl.G == 1) REEF_TRY(run_core_graphed<C>(ctx, d_scalars, pl, is_mont, d_res));
    else REEF_TRY(run_core<C>(ctx, d_scalars, pl, is_mont, nullptr, nullptr, d_res));
    return finish_output<C>(ctx, d_res, 1, out, out_loc);
}

template <int C>
static reef_status v_msm(void *impl, const reef_fe *scalars, size_t n, int loc, bool is_mont, reef_jacobian *out, int out_loc) {
    Ctx<C> *ctx = (Ctx<C> *)impl;
    if (!ctx || !out || (n && !scalars)) { set_error("null argument"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    Key<C> *key = ctx->key;
    REEF_ON_DEVICE(key->device);
    CtxScope<C> scope(ctx);
    REEF_TRY(scope.enter());
    if (n > key->n) { set_error("n = %zu exceeds the key length %zu", n, key->n); return REEF_ERR_ARG; }
    jacobian256 *d_res = nullptr;
    REEF_TRY(result_target<C>(ctx, 1, out, out_loc, &d_res));
    if (n == 0) {
        REEF_HIP_TRY(hipMemsetAsync(d_res, 0, sizeof(jacobian256), ctx->stream));
        return finish_output<C>(ctx, d_res, 1, out, out_loc);
    }
    const fe256 *d_scalars = (const fe256 *)scalars;
    if (loc != REEF_DEVICE) {
        REEF_TRY(ctx->scalars.ensure(n * sizeof(fe256)));
        REEF_HIP_TRY(hipMemcpyAsync(ctx->scalars.p, scalars, n * sizeof(fe256), hipMemcpyHostToDevice, ctx->stream));
        d_scalars = ctx->scalars.template as<fe256>();
    }
    return msm_device_scalars<C>(ctx, d_scalars, n, is_mont, out, out_loc, d_res);
}

// The tail the symbol routes share: M table entries in row order, `blocks` a row, written by launch_entries(entries, bucket_start)
// as (row, table index) with bucket_start[row] = row*blocks, are summed per row by k_accum0 with the rows as "buckets".
template <int C, class LaunchEntries>
static reef_status sym_rows_sum(Ctx<C> *ctx, u64 M, u32 blocks, size_t rows, bool is_mont, const fe256 *d_blinds, const affine256 *d_h,
                                jacobian256 *d_out, LaunchEntries launch_entries) {
    hipStream_t st = ctx->stream;
    // chunk length as in run_core: about one wave per two SIMDs at least, long chunks when the chip stays full
    u32 L0 = ctx->L0;
    if (L0 == 0) {
        L0 = 32;
        while (L0 < 128 && L0 < blocks && M / (2 * L0) >= 131072) L0 *= 2;
        while (L0 > 8 && M / L0 < 24576) L0 /= 2;
    }
    const u32 nchunks0 = (u32)round_up(ceil_div(M, L0), 64);
    REEF_TRY(ctx->entries.ensure((u64)nchunks0 * L0 * sizeof(u32x2)));
    REEF_TRY(ctx->bstart.ensure((rows + 1) * sizeof(u32)));
    REEF_TRY(ctx->bucket_acc.ensure(rows * sizeof(xyzz_mem)));
    const u32 len1 = 2 * nchunks0, len2 = 2 * ceil_div(len1, 64);
    REEF_TRY(ctx->lkeys[0].ensure((u64)len1 * sizeof(u32)));
    REEF_TRY(ctx->lvals[0].ensure((u64)len1 * sizeof(xyzz_mem)));
    REEF_TRY(ctx->lkeys[1].ensure((u64)len2 * sizeof(u32)));
    REEF_TRY(ctx->lvals[1].ensure((u64)len2 * sizeof(xyzz_mem)));
    u32x2 *entries = ctx->entries.template as<u32x2>();
    u32 *bstart = ctx->bstart.template as<u32>();
    xyzz_mem *row_acc = ctx->bucket_acc.template as<xyzz_mem>();
    if (ctx->timing) {
        REEF_TRY(ctx_begin_timing<C>(ctx));
        REEF_HIP_TRY(hipEventRecord(ctx->ev[0], st));
    }
    launch_entries(entries, bstart);
    if (ctx->timing) REEF_HIP_TRY(hipEventRecord(ctx->ev[1], st));
    hipLaunchKernelGGL((k_accum0<C, false, false>), dim3(ceil_div(nchunks0, 256)), dim3(256), 0, st, ctx->sym_table.template as<affine256>(), (const void *)entries, bstart + rows, L0,
                       nchunks0, row_acc, ctx->lkeys[0].template as<u32>(), ctx->lvals[0].template as<xyzz_mem>(), 0u);
    if (ctx->timing) REEF_HIP_TRY(hipEventRecord(ctx->ev[2], st));
    launch_partial_merge<C>(ctx, merge_plan(nchunks0, ctx->coop, core_switches(), false), nchunks0, row_acc);
    hipLaunchKernelGGL(k_final<C>, dim3(ceil_div(rows, 64)), dim3(64), 0, st, row_acc, 1u, 0u, (u32)rows, d_out);   // XYZZ row sums -> Jacobian
    if (d_blinds) REEF_TRY(launch_blind<C>(ctx, d_out, d_blinds, d_h, is_mont, rows));
    if (ctx->timing) {
        REEF_HIP_TRY(hipEventRecord(ctx->ev[3], st));
        ctx->ev_pending[ctx->ev_last] = true;
    }
    REEF_HIP_TRY(hipGetLastError());
    return REEF_OK;
}

// Row commits of `bits`-bit symbols through block tables (see k_sym_multiples).  d_sym: rows*row_len bytes on the device.
static inline u32 sym_block_size(u32 bits) { return std::max<u32>(1, 9 / bits); }
static inline bool sym_path_pays(size_t rows, size_t row_len, u32 bits, bool cached) {
    if (bits == 0 || bits > 8 || row_len == 0) return false;
    const u64 table_points = (u64)ceil_div(row_len, sym_block_size(bits)) << (bits * sym_block_size(bits));
    if (table_points > (1ull << 26)) return false;                 // 4 GiB of table at most
    return cached || (u64)rows * row_len >= 2 * table_points;      // building the tables costs about two additions per table entry
}
template <int C>
static reef_status run_rows_symbols(Ctx<C> *ctx, const unsigned char *d_sym, size_t rows, size_t row_len, u32 bits, bool is_mont,
                                    const fe256 *d_blinds, const affine256 *d_h, jacobian256 *d_out) {
    hipStream_t st = ctx->stream;
    if (ctx->wsplit_world > 1 && ctx->wsplit_rank != 0) {   // no windows to split here: rank 0 owns the whole sum, the others contribute the identity
        REEF_HIP_TRY(hipMemsetAsync(d_out, 0, rows * sizeof(jacobian256), st));
        return REEF_OK;
    }
    const u32 k = sym_block_size(bits), combos = 1u << (bits * k);
    const u32 blocks = (u32)ceil_div(row_len, k);
    const u64 table_points = (u64)blocks * combos;
    const u64 M = (u64)rows * blocks;
    if (M >= (1ull << 31)) { set_error("too many row entries"); return REEF_ERR_ARG; }
    if (ctx->sym_bits != bits || ctx->sym_k != k || ctx->sym_row_len != row_len) {
        const u32 lb = bits <= 4 ? bits : (bits + 1) / 2, hb = bits - lb;
        const u64 lo_cnt = (u64)row_len << lb, hi_cnt = hb ? (u64)row_len << hb : 0;
        REEF_TRY(ctx->sym_table.ensure(table_points * sizeof(affine256)));
        REEF_TRY(ctx->sym_tmp.ensure((lo_cnt + hi_cnt + (k > 1 || hb ? table_points : 0)) * sizeof(xyzz_mem)));
        xyzz_mem *lo = ctx->sym_tmp.template as<xyzz_mem>(), *hi = lo + lo_cnt, *full = hi + hi_cnt;
        hipLaunchKernelGGL(k_sym_multiples<C>, dim3(ceil_div(2 * row_len, 256)), dim3(256), 0, st, ctx->key->tables, (u32)row_len, lb, hb, lo, hi);
        const xyzz_mem *src = lo;                       // k = 1 and one level: the multiples are the table
        if (k > 1 || hb) {
            hipLaunchKernelGGL(k_sym_blocks<C>, dim3((u32)ceil_div(table_points, 256)), dim3(256), 0, st, lo, hi, (u32)row_len, bits, lb, k, blocks, full);
            src = full;
        }
        hipLaunchKernelGGL((k_xyzz_normalize<C, false>), dim3((u32)ceil_div(ceil_div(table_points, NORM_PER), 256)), dim3(256), 0, st, src,
                           (u32)table_points, ctx->sym_table.template as<affine256>());
        ctx->sym_bits = bits; ctx->sym_k = k; ctx->sym_row_len = (u32)row_len;
        ctx->symw_bits = 0;                             // the wide route's tables lived in the same buffers
    }
    return sym_rows_sum<C>(ctx, M, blocks, rows, is_mont, d_blinds, d_h, d_out, [&](u32x2 *entries, u32 *bstart) {
        hipLaunchKernelGGL(k_sym_entries, dim3((u32)ceil_div(std::max<u64>(M, rows + 1), 256)), dim3(256), 0, st, d_sym, (u32)rows, (u32)row_len, bits, k, blocks,
                           entries, bstart);
    });
}

// Row commits of symbols wider than a byte (see k_sym_entries_wide): P = ceil(bits / 8) byte planes over the generators 256^p * G_j.
// The tables are the byte route's at k = 1, built by its kernels over the plane generators: 256 multiples for each generator of the
// P - 1 full planes, 2^top_bits for the top plane.  d_sym: rows*row_len symbols of T on the device.
static inline u64 sym_wide_table_points(size_t row_len, u32 bits) {
    const u32 P = ceil_div(bits, 8u);
    return (u64)(P - 1) * row_len * 256 + ((u64)row_len << (bits - 8 * (P - 1)));
}
template <int C>
static void sym_wide_multiples(Ctx<C> *ctx, const affine256 *gens, u64 n, u32 bits, xyzz_mem *scratch, xyzz_mem *table) {
    const u32 lb = bits <= 4 ? bits : (bits + 1) / 2, hb = bits - lb;   // n*2^bits table entries: v*gens[j] at table[(j << bits) + v]
    xyzz_mem *lo = hb ? scratch : table, *hi = scratch + (n << lb);      // one level: the multiples are the table
    hipLaunchKernelGGL(k_sym_multiples<C>, dim3((u32)ceil_div(2 * n, 256)), dim3(256), 0, ctx->stream, gens, (u32)n, lb, hb, lo, hi);
    if (hb) hipLaunchKernelGGL(k_sym_blocks<C>, dim3((u32)ceil_div(n << bits, 256)), dim3(256), 0, ctx->stream, lo, hi, (u32)n, bits, lb, 1u, (u32)n, table);
}
template <int C, typename T>
static reef_status run_rows_symbols_wide(Ctx<C> *ctx, const T *d_sym, size_t rows, size_t row_len, u32 bits, bool is_mont,
                                         const fe256 *d_blinds, const affine256 *d_h, jacobian256 *d_out) {
    hipStream_t st = ctx->stream;
    if (ctx->wsplit_world > 1 && ctx->wsplit_rank != 0) {   // as run_rows_symbols: rank 0 owns the whole sum
        REEF_HIP_TRY(hipMemsetAsync(d_out, 0, rows * sizeof(jacobian256), st));
        return REEF_OK;
    }
    const u32 P = ceil_div(bits, 8u), top_bits = bits - 8 * (P - 1);
    const u64 full_gens = (u64)(P - 1) * row_len, table_points = sym_wide_table_points(row_len, bits);
    const u64 M = (u64)rows * row_len * P;
    if (ctx->symw_bits != bits || ctx->symw_planes != P || ctx->symw_row_len != row_len) {
        ctx->sym_bits = 0; ctx->symw_bits = 0;          // the byte route's tables lived in the same buffers
        // scratch: plane generators (XYZZ, then affine), the two half-byte multiples of the widest build, the table in XYZZ
        const u64 mult_cnt = std::max<u64>(full_gens << 5, top_bits > 4 ? (u64)row_len << (1 + (top_bits + 1) / 2) : 0);
        REEF_TRY(ctx->sym_table.ensure(table_points * sizeof(affine256)));
        REEF_TRY(ctx->sym_tmp.ensure((u64)P * row_len * (sizeof(xyzz_mem) + sizeof(affine256)) + (mult_cnt + table_points) * sizeof(xyzz_mem)));
        xyzz_mem *planes = ctx->sym_tmp.template as<xyzz_mem>(), *mult = planes + (u64)P * row_len, *full = mult + mult_cnt;
        affine256 *gens = (affine256 *)(full + table_points);
        const affine256 *top_gens = ctx->key->tables;   // table 0 of the key: G_j itself, whatever the key's kind
        if (P > 1) {
            // planes[p*row_len + j] = 256^p * G_j, 8 doublings from the plane below, then one batch normalisation
            hipLaunchKernelGGL(k_shift_chain<C>, dim3((u32)ceil_div(row_len, 64)), dim3(64), 0, st, ctx->key->tables, (u32)row_len, 8u, P, 1, planes);
            hipLaunchKernelGGL((k_xyzz_normalize<C, false>), dim3((u32)ceil_div(ceil_div((u64)P * row_len, NORM_PER), 256)), dim3(256), 0, st, planes,
                               (u32)(P * row_len), gens);
            sym_wide_multiples<C>(ctx, gens, full_gens, 8, mult, full);
            top_gens = gens + full_gens;
        }
        sym_wide_multiples<C>(ctx, top_gens, row_len, top_bits, mult, full + (full_gens << 8));
        hipLaunchKernelGGL((k_xyzz_normalize<C, false>), dim3((u32)ceil_div(ceil_div(table_points, NORM_PER), 256)), dim3(256), 0, st, full,
                           (u32)table_points, ctx->sym_table.template as<affine256>());
        ctx->symw_bits = bits; ctx->symw_planes = P; ctx->symw_row_len = (u32)row_len;
    }
    return sym_rows_sum<C>(ctx, M, (u32)(P * row_len), rows, is_mont, d_blinds, d_h, d_out, [&](u32x2 *entries, u32 *bstart) {
        hipLaunchKernelGGL(k_sym_entries_wide<T>, dim3((u32)ceil_div(std::max<u64>((u64)rows * row_len, rows + 1), 256)), dim3(256), 0, st, d_sym, (u32)rows,
                           (u32)row_len, bits, P, entries, bstart);
    });
}

template <int C>
static reef_status v_msm_rows(void *impl, const reef_fe *scalars, size_t rows, size_t row_len, int loc, bool is_mont,
                              uint32_t max_bits, const reef_fe *blinds, const reef_affine *h, reef_jacobian *out, int out_loc) {
    Ctx<C> *ctx = (Ctx<C> *)impl;
    if (!ctx || !out || ((rows * row_len) && !scalars) || (blinds && !h)) { set_error("null argument"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    Key<C> *key = ctx->key;
    REEF_ON_DEVICE(key->device);
    CtxScope<C> scope(ctx);
    REEF_TRY(scope.enter());
    if (row_len > key->n) { set_error("row_len = %zu exceeds the key length %zu", row_len, key->n); return REEF_ERR_ARG; }
    if (rows == 0) return REEF_OK;
    const size_t N = rows * row_len;
    jacobian256 *d_res = nullptr;
    REEF_TRY(result_target<C>(ctx, rows, out, out_loc, &d_res));
    const fe256 *d_scalars = (const fe256 *)scalars;
    const fe256 *d_blinds = (const fe256 *)blinds;
    const affine256 *d_h = (const affine256 *)h;
    ctx->h_host = (loc != REEF_DEVICE && blinds) ? h : nullptr;
    if (loc != REEF_DEVICE) {
        if (N) {
            REEF_TRY(ctx->scalars.ensure(N * sizeof(fe256)));
            REEF_HIP_TRY(hipMemcpyAsync(ctx->scalars.p, scalars, N * sizeof(fe256), hipMemcpyHostToDevice, ctx->stream));
            d_scalars = ctx->scalars.template as<fe256>();
        }
        if (blinds) {
            REEF_TRY(ctx->blinds.ensure(rows * sizeof(fe256)));
            REEF_TRY(ctx->hpoint.ensure(sizeof(affine256)));
            REEF_HIP_TRY(hipMemcpyAsync(ctx->blinds.p, blinds, rows * sizeof(fe256), hipMemcpyHostToDevice, ctx->stream));
            REEF_HIP_TRY(hipMemcpyAsync(ctx->hpoint.p, h, sizeof(affine256), hipMemcpyHostToDevice, ctx->stream));
            d_blinds = ctx->blinds.template as<fe256>();
            d_h = ctx->hpoint.template as<affine256>();
        }
    }
    if (row_len == 0) {
        REEF_HIP_TRY(hipMemsetAsync(d_res, 0, rows * sizeof(jacobian256), ctx->stream));
        if (d_blinds && (ctx->wsplit_world <= 1 || ctx->wsplit_rank == 0)) REEF_TRY(launch_blind<C>(ctx, d_res, d_blinds, d_h, is_mont, rows));
        return finish_output<C>(ctx, d_res, rows, out, out_loc);
    }
    if (rows == 1 && small_path(key->small_tab, key->small_n, row_len, ctx->wsplit_world)) {
        // CE::commit on a small resident key: v*G (+ blind*H) straight from the nibble tables
        if (d_blinds) {
            if (ctx->h_host) REEF_TRY(ensure_h_table<C>(ctx, ctx->h_host, REEF_HOST));
            else REEF_TRY(ensure_h_table<C>(ctx, (const reef_affine *)d_h, REEF_DEVICE));
        }
        REEF_TRY(run_small<C>(ctx, d_scalars, row_len, is_mont, d_blinds, d_blinds != nullptr, d_res));
        return finish_output<C>(ctx, d_res, 1, out, out_loc);
    }
    if (rows == 1 && (max_bits == 0 || max_bits > 13)) {
        // CE::commit on a key of Reef's size: v*G from the byte tables, + blind*H from H's nibble table
        wide_poll<C>(key);
        if (wide_path(key->wide_tab, key->wide_n.load(std::memory_order_acquire), row_len, ctx->wsplit_world)) {
            REEF_TRY(run_wide<C>(ctx, d_scalars, row_len, is_mont, d_res));
            if (d_blinds) REEF_TRY(launch_blind<C>(ctx, d_res, d_blinds, d_h, is_mont, 1));
            return finish_output<C>(ctx, d_res, 1, out, out_loc);
        }
    }
    // scalar width: given, or measured on the device (one small sync)
    u32 bits = max_bits;
    if (bits == 0) {
        REEF_TRY(ctx->maxbits.ensure(sizeof(u32)));
        REEF_HIP_TRY(hipMemsetAsync(ctx->maxbits.p, 0, sizeof(u32), ctx->stream));
        hipLaunchKernelGGL(k_max_bits<C>, dim3(std::min<u32>(2048, ceil_div(N, 256))), dim3(256), 0, ctx->stream, d_scalars, (u32)N,
                           (int)is_mont, ctx->maxbits.template as<u32>());
        REEF_HIP_TRY(hipMemcpyAsync(&bits, ctx->maxbits.p, sizeof(u32), hipMemcpyDeviceToHost, ctx->stream));
        REEF_HIP_TRY(hipStreamSynchronize(ctx->stream));
        if (bits == 0) bits = 1;
    }
    if (bits > 255) bits = 255;
    if (row_len <= key->n && sym_path_pays(rows, row_len, bits, ctx->sym_bits == bits && ctx->sym_row_len == row_len)) {
        // tiny scalars (document symbols): block tables, no sort and no bucket reduction
        REEF_TRY(ctx->sym_u8.ensure(N));
        hipLaunchKernelGGL(k_row_symbols<C>, dim3((u32)ceil_div(N, 256)), dim3(256), 0, ctx->stream, d_scalars, (u64)N, (int)is_mont,
                           ctx->sym_u8.template as<unsigned char>());
        REEF_TRY(run_rows_symbols<C>(ctx, ctx->sym_u8.template as<unsigned char>(), rows, row_len, bits, is_mont, d_blinds, d_h, d_res));
        return finish_output<C>(ctx, d_res, rows, out, out_loc);
    }
    CorePlan pl{};
    pl.rows = (u32)rows; pl.row_len = (u32)row_len; pl.n_ctx = (u32)key->n;
    if (bits + 1 <= 13) {  // one signed window holds every scalar: only table 0 is needed
        pl.c = std::max<u32>(2, bits + 1); pl.W = 1; pl.G = 1;
    } else if (key->T == 1) {  // no precompute: free choice of window for the row length
        pl.c = std::min<u32>(choose_window(row_len, 0), 11);
        pl.W = ceil_div(bits + 1, pl.c); pl.G = pl.W;
    } else {
        pl.c = key->c; pl.W = std::min<u32>(key->W, ceil_div(bits + 1, key->c)); pl.G = key->G;  // table shifts fix G
    }
    const u64 keys_per_row = (u64)pl.G << (pl.c - 1);
    const u64 key_keys_per_row = (u64)key->G << (key->c - 1);
    if (rows > 1 && row_len >= 8192 && bits + 1 > 13 && key_keys_per_row * 2 <= MAX_SCAN_KEYS) {
        // long rows: each is a K1-sized MSM; sort them in batches with the sliced sort, share the rest
        const size_t per_batch = std::min<size_t>({rows, (size_t)(MAX_SCAN_KEYS / key_keys_per_row),
                                                   (size_t)(((1ull << 31) - 1) / ((u64)row_len * key->W)), (size_t)64});
        for (size_t r = 0; r < rows; r += per_batch) {
            const size_t cnt = std::min(per_batch, rows - r);
            CorePlan bp{key->c, std::min<u32>(key->W, ceil_div(bits + 1, key->c)), key->G, (u32)cnt, (u32)row_len, (u32)key->n};
            bp.slice_sort = cnt > 1;
            REEF_TRY(run_core<C>(ctx, d_scalars + r * row_len, bp, is_mont, d_blinds ? d_blinds + r : nullptr, d_h, d_res + r));
        }
    } else if (rows == 1 || keys_per_row > MAX_LDS_KEYS || keys_per_row * rows > MAX_SCAN_KEYS) {
        // rows too wide for the LDS row sort: run them one by one through the K1 path
        CorePlan one{key->c, key->W, key->G, 1u, (u32)row_len, (u32)key->n};
        for (size_t r = 0; r < rows; ++r)
            REEF_TRY(run_core<C>(ctx, d_scalars + r * row_len, one, is_mont, d_blinds ? d_blinds + r : nullptr, d_h, d_res + r));
    } else {
        REEF_TRY(run_core<C>(ctx, d_scalars, pl, is_mont, d_blinds, d_h, d_res));
    }
    return finish_output<C>(ctx, d_res, rows, out, out_loc);
}

// HyraxPC::commit on the document's own symbols (elem_bytes = 1, 2 or 4 each, < 2^bits): no field elements cross the ABI.
template <int C>
static reef_status msm_rows_symbols_any(void *impl, const void *symbols, u32 elem_bytes, size_t rows, size_t row_len, int loc, uint32_t bits,
                                        const reef_fe *blinds, const reef_affine *h, bool blinds_are_mont, reef_jacobian *out, int out_loc) {
    Ctx<C> *ctx = (Ctx<C> *)impl;
    const bool wide = elem_bytes > 1;
    if (!ctx || !out || ((rows * row_len) && !symbols) || (blinds && !h)) { set_error("null argument"); return REEF_ERR_ARG; }
    if (!wide && (bits == 0 || bits > 8)) { set_error("symbol width must be 1..8 bits"); return REEF_ERR_ARG; }
    if (wide && (bits == 0 || bits > 8 * elem_bytes)) { set_error("symbol_bits = %u: a %u-byte symbol holds 1..%u bits", bits, elem_bytes, 8 * elem_bytes); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    Key<C> *key = ctx->key;
    REEF_ON_DEVICE(key->device);
    CtxScope<C> scope(ctx);
    REEF_TRY(scope.enter());
    if (row_len > key->n) { set_error("row_len = %zu exceeds the key length %zu", row_len, key->n); return REEF_ERR_ARG; }
    if (rows == 0) return REEF_OK;
    const u64 table_points = wide ? sym_wide_table_points(std::max<size_t>(row_len, 1), bits)
                                  : (u64)ceil_div(std::max<size_t>(row_len, 1), sym_block_size(bits)) << (bits * sym_block_size(bits));
    if (table_points > (1ull << 26)) { set_error("symbol tables too large for this row length"); return REEF_ERR_ARG; }
    if (wide && (u64)rows * row_len * ceil_div(bits, 8u) >= (1ull << 31)) { set_error("too many row entries"); return REEF_ERR_ARG; }
    jacobian256 *d_res = nullptr;
    REEF_TRY(result_target<C>(ctx, rows, out, out_loc, &d_res));
    const fe256 *d_blinds = (const fe256 *)blinds;
    const affine256 *d_h = (const affine256 *)h;
    ctx->h_host = (loc != REEF_DEVICE && blinds) ? h : nullptr;
    const void *d_sym = symbols;
    if (loc != REEF_DEVICE) {
        if (rows * row_len) {
            REEF_TRY(ctx->sym_u8.ensure(rows * row_len * elem_bytes));
            REEF_HIP_TRY(hipMemcpyAsync(ctx->sym_u8.p, symbols, rows * row_len * elem_bytes, hipMemcpyHostToDevice, ctx->stream));
            d_sym = ctx->sym_u8.p;
        }
        if (blinds) {
            REEF_TRY(ctx->blinds.ensure(rows * sizeof(fe256)));
            REEF_TRY(ctx->hpoint.ensure(sizeof(affine256)));
            REEF_HIP_TRY(hipMemcpyAsync(ctx->blinds.p, blinds, rows * sizeof(fe256), hipMemcpyHostToDevice, ctx->stream));
            REEF_HIP_TRY(hipMemcpyAsync(ctx->hpoint.p, h, sizeof(affine256), hipMemcpyHostToDevice, ctx->stream));
            d_blinds = ctx->blinds.template as<fe256>();
            d_h = ctx->hpoint.template as<affine256>();
        }
    }
    if (row_len == 0) {
        REEF_HIP_TRY(hipMemsetAsync(d_res, 0, rows * sizeof(jacobian256), ctx->stream));
        if (d_blinds && (ctx->wsplit_world <= 1 || ctx->wsplit_rank == 0)) REEF_TRY(launch_blind<C>(ctx, d_res, d_blinds, d_h, blinds_are_mont, rows));
        return finish_output<C>(ctx, d_res, rows, out, out_loc);
    }
    if (elem_bytes == 4) REEF_TRY((run_rows_symbols_wide<C, uint32_t>(ctx, (const uint32_t *)d_sym, rows, row_len, bits, blinds_are_mont, d_blinds, d_h, d_res)));
    else if (elem_bytes == 2) REEF_TRY((run_rows_symbols_wide<C, uint16_t>(ctx, (const uint16_t *)d_sym, rows, row_len, bits, blinds_are_mont, d_blinds, d_h, d_res)));
    else REEF_TRY(run_rows_symbols<C>(ctx, (const unsigned char *)d_sym, rows, row_len, bits, blinds_are_mont, d_blinds, d_h, d_res));
    return finish_output<C>(ctx, d_res, rows, out, out_loc);
}
template <int C>
static reef_status v_msm_rows_symbols(void *impl, const uint8_t *symbols, size_t rows, size_t row_len, int loc, uint32_t bits,
                                      const reef_fe *blinds, const reef_affine *h, bool blinds_are_mont, reef_jacobian *out, int out_loc) {
    return msm_rows_symbols_any<C>(impl, symbols, 1, rows, row_len, loc, bits, blinds, h, blinds_are_mont, out, out_loc);
}
// The same from 16- and 32-bit symbols (reef_msm_rows_symbols_wide).
template <int C>
static reef_status v_msm_rows_symbols_wide(void *impl, const void *symbols, uint32_t elem_bytes, size_t rows, size_t row_len, int loc, uint32_t bits,
                                           const reef_fe *blinds, const reef_affine *h, bool blinds_are_mont, reef_jacobian *out, int out_loc) {
    if (elem_bytes != 2 && elem_bytes != 4) { set_error("elem_bytes = %u: wide symbols are 2 or 4 bytes each", elem_bytes); return REEF_ERR_ARG; }
    return msm_rows_symbols_any<C>(impl, symbols, elem_bytes, rows, row_len, loc, bits, blinds, h, blinds_are_mont, out, out_loc);
}

// The nibble table of one point h (ABI affine, host) into buf: small_table_points(1) points, then two staging points.  Built on
// ctx's stream (its scratch), waited for.  For a second blind term beside the one ctx->h_tab caches (ipa_cross_run's tab2).
template <int C> static reef_status point_table_build(Ctx<C> *ctx, const reef_affine *h, DevBuf &buf) {
    REEF_TRY(buf.ensure((small_table_points(1) + 2) * sizeof(affine256)));
    affine256 *tab = buf.template as<affine256>(), *raw = tab + small_table_points(1), *imp = raw + 1;
    REEF_HIP_TRY(hipMemcpyAsync(raw, h, sizeof(reef_affine), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_import_key<C>, dim3(1), dim3(256), 0, ctx->stream, (const affine256 *)raw, 1u, imp);
    REEF_TRY(small_build<C>(ctx, imp, 1, tab));
    REEF_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return REEF_OK;
}
// out += blinds[r] * P for `rows` results on the device, P's nibble table given (blinds: canonical integers)
template <int C> static reef_status launch_blind_tab(Ctx<C> *ctx, jacobian256 *d_out, const fe256 *d_blinds, const affine256 *tab, size_t rows) {
    hipLaunchKernelGGL(k_add_blind_tab<C>, dim3(ceil_div(rows * BLIND_LANES, 64)), dim3(64), 0, ctx->stream, d_out, d_blinds, tab, 0, (u32)rows);
    return REEF_OK;
}

// The four routes of the cross terms (byte tables, nibble tables, pre-shifted key, plain key) on a ctx already entered, a on the device.  With
// d_blinds (two canonical integers on the device) L += d_blinds[0] h and R += d_blinds[1] h through h's nibble table (h: affine,
// host); with d_blinds2 also L += d_blinds2[0] P, R += d_blinds2[1] P through P's nibble table tab2 (point_table_build; only with
// d_blinds); without them nothing is added and the launches are those of reef_ipa_cross_terms.
template <int C>
static reef_status ipa_cross_run(Ctx<C> *ctx, const fe256 *d_a, size_t n_k, bool is_mont, const reef_fe *w1s, const reef_fe *w2s, size_t k,
                                 const fe256 *d_blinds, const reef_affine *h, const fe256 *d_blinds2, const affine256 *tab2,
                                 reef_jacobian *out_l, reef_jacobian *out_r) {
    if (!d_blinds) d_blinds2 = nullptr;
    Key<C> *key = ctx->key;
    const size_t n = key->n;
    hipStream_t st = ctx->stream;
    REEF_TRY(ctx->scalars.ensure((2 * n + n_k) * sizeof(fe256)));
    fe256 *s_l = ctx->scalars.template as<fe256>(), *s_r = s_l + n;
    struct HostH {                                     // launch_blind takes h's nibble table from ctx->h_host (rebuilt only when h changes)
        Ctx<C> *c;
        const reef_affine *saved;
        ~HostH() { c->h_host = saved; }
    } host_h{ctx, ctx->h_host};
    if (d_blinds) ctx->h_host = h;
    const size_t ncoef = (size_t)1 << k;
    REEF_TRY(ctx->blinds.ensure(ncoef * sizeof(fe256)));
    fe256 *coef = ctx->blinds.template as<fe256>();
    IpaChallenges ch;
    memset(&ch, 0, sizeof ch);
    if (k) {
        memcpy(ch.w1, w1s, k * sizeof(fe256));
        memcpy(ch.w2, w2s, k * sizeof(fe256));
    }
    hipLaunchKernelGGL(k_ipa_coef<C>, dim3(ceil_div(ncoef, 256)), dim3(256), 0, st, ch, (u32)k, coef);
    REEF_TRY(ctx->result.ensure(2 * sizeof(jacobian256)));
    jacobian256 *d_res = ctx->result.template as<jacobian256>();
    jacobian256 *land = nullptr;                       // host-mapped landing zone (allocated on first use)
    reef_jacobian dummy;
    REEF_TRY(result_target<C>(ctx, 2, &dummy, REEF_HOST, &land));
    wide_poll<C>(key);
    if (wide_path(key->wide_tab, key->wide_n.load(std::memory_order_acquire), n, ctx->wsplit_world)) {
        // byte tables: L and R in ONE pass over the 32 n table entries -- every point feeds exactly one of them
        if (ctx->timing) {
            REEF_TRY(ctx_begin_timing<C>(ctx));
            REEF_HIP_TRY(hipEventRecord(ctx->ev[0], st));
        }
        hipLaunchKernelGGL(k_ipa_expand_merged<C>, dim3(ceil_div(n, 256)), dim3(256), 0, st, d_a, (u32)n_k, (const fe256 *)coef, (u32)n, (int)is_mont, s_l);
        const u64 total = (u64)WIDE_WINDOWS * n;
        const u32 per = wide_per(total);
        const u32 wgs = (u32)ceil_div(total, (u64)256 * per);          // <= 512 for n <= 65536 with the default chunking
        if (wgs > 512) { set_error("REEF_MSM_WIDE_PER = %u leaves %u partial sums per cross term (the final kernel takes 512)", per, wgs); return REEF_ERR_ARG; }
        REEF_TRY(ctx->wide_dig.ensure(total * sizeof(short)));
        REEF_TRY(ctx->wide_partial.ensure((size_t)2 * wgs * sizeof(xyzz_mem)));
        xyzz_mem *p1 = ctx->wide_partial.template as<xyzz_mem>();
        hipLaunchKernelGGL(k_wide_recode<C>, dim3(ceil_div(n, 256)), dim3(256), 0, st, (const fe256 *)s_l, (u32)n, 0, ctx->wide_dig.template as<short>());
        if (ctx->timing) REEF_HIP_TRY(hipEventRecord(ctx->ev[1], st));
        hipLaunchKernelGGL((k_wide_accum<C, true>), dim3(wgs), dim3(256), 0, st, (const affine256 *)key->wide_tab, (u32)key->wide_n.load(),
                           (const short *)ctx->wide_dig.template as<short>(), (u32)n, per, (u32)n_k, p1);
        if (ctx->timing) REEF_HIP_TRY(hipEventRecord(ctx->ev[2], st));
        hipLaunchKernelGGL(k_small_final<C>, dim3(2), dim3(256), 0, st, (const xyzz_mem *)p1, wgs, land);
        if (d_blinds) REEF_TRY(launch_blind<C>(ctx, land, d_blinds, nullptr, false, 2));
        if (d_blinds2) REEF_TRY(launch_blind_tab<C>(ctx, land, d_blinds2, tab2, 2));
        if (ctx->timing) {
            REEF_HIP_TRY(hipEventRecord(ctx->ev[3], st));
            ctx->ev_pending[ctx->ev_last] = true;
        }
        REEF_HIP_TRY(hipGetLastError());
        REEF_HIP_TRY(hipStreamSynchronize(st));
        memcpy(out_l, &land[0], sizeof(jacobian256));
        memcpy(out_r, &land[1], sizeof(jacobian256));
        return REEF_OK;
    }
    hipLaunchKernelGGL(k_ipa_expand<C>, dim3(ceil_div(n, 256)), dim3(256), 0, st, d_a, (u32)n_k, coef, (u32)n, (int)is_mont, s_l, s_r);
    if (small_path(key->small_tab, key->small_n, n, ctx->wsplit_world)) {
        // a small key (a folded one above all: reef_msm_ctx_create_folded): L and R are two sums over its nibble tables, no sort, no buckets
        REEF_TRY(run_small<C>(ctx, s_l, n, false, nullptr, false, land));
        REEF_TRY(run_small<C>(ctx, s_r, n, false, nullptr, false, land + 1));
        if (d_blinds) REEF_TRY(launch_blind<C>(ctx, land, d_blinds, nullptr, false, 2));
        if (d_blinds2) REEF_TRY(launch_blind_tab<C>(ctx, land, d_blinds2, tab2, 2));
        REEF_HIP_TRY(hipGetLastError());
        REEF_HIP_TRY(hipStreamSynchronize(st));
        memcpy(out_l, &land[0], sizeof(jacobian256));
        memcpy(out_r, &land[1], sizeof(jacobian256));
        return REEF_OK;
    }
    CorePlan pl{key->c, key->W, key->G, 1u, (u32)n, (u32)key->n};
    if (pl.G == 1) {   // L and R as a batch of two MSMs: one pass of the pipeline, one result copy
        CorePlan two = pl;
        two.rows = 2;
        two.slice_sort = true;
        REEF_TRY(run_core<C>(ctx, s_l, two, false, d_blinds, nullptr, land));   // the final kernel stores L and R where the host reads them
        if (d_blinds2) REEF_TRY(launch_blind_tab<C>(ctx, land, d_blinds2, tab2, 2));
        REEF_HIP_TRY(hipStreamSynchronize(st));
        memcpy(out_l, &land[0], sizeof(jacobian256));
        memcpy(out_r, &land[1], sizeof(jacobian256));
        return REEF_OK;
    }
    reef_jacobian *outs[2] = {out_l, out_r};
    const fe256 *vecs[2] = {s_l, s_r};
    // blind terms: d_blinds[v] h into the landing zone's last two slots (past the group sums), ahead of the MSMs whose group-sum
    // waits cover it; each is added to its window combine on the host
    jacobian256 *bt = (d_blinds && (size_t)pl.G * sizeof(xyzz_mem) <= 62 * sizeof(jacobian256)) ? land + 62 : nullptr;
    if (bt) {
        memset(bt, 0, 2 * sizeof(jacobian256));
        REEF_TRY(launch_blind<C>(ctx, bt, d_blinds, nullptr, false, 2));
        if (d_blinds2) REEF_TRY(launch_blind_tab<C>(ctx, bt, d_blinds2, tab2, 2));
    }
    for (int v = 0; v < 2; ++v) {   // plain key: finish each window combine on the host (as in v_msm)
        const xyzz_mem *gs = nullptr;
        REEF_TRY(run_core<C>(ctx, vecs[v], pl, false, nullptr, nullptr, d_res + v, &gs));
        std::vector<xyzz_mem> hs;
        REEF_TRY(fetch_group_sums<C>(ctx, gs, pl.G, hs));
        jacobian256 j = host_window_combine<C>(hs.data(), pl.G, pl.c);
        if (bt) j = host_jacobian_add<C>(j, bt[v]);
        memcpy(outs[v], &j, sizeof j);
    }
    if (d_blinds && !bt) {   // many groups: the blind term on the device, the combined sums there and back
        jacobian256 both[2];
        memcpy(&both[0], out_l, sizeof(jacobian256));
        memcpy(&both[1], out_r, sizeof(jacobian256));
        REEF_HIP_TRY(hipMemcpyAsync(d_res, both, sizeof both, hipMemcpyHostToDevice, st));
        REEF_TRY(launch_blind<C>(ctx, d_res, d_blinds, nullptr, false, 2));
        if (d_blinds2) REEF_TRY(launch_blind_tab<C>(ctx, d_res, d_blinds2, tab2, 2));
        REEF_HIP_TRY(hipGetLastError());
        REEF_HIP_TRY(hipMemcpyAsync(both, d_res, sizeof both, hipMemcpyDeviceToHost, st));
        REEF_HIP_TRY(hipStreamSynchronize(st));
        memcpy(out_l, &both[0], sizeof(jacobian256));
        memcpy(out_r, &both[1], sizeof(jacobian256));
    }
    return REEF_OK;
}

// Cross terms of IPA round k over the ORIGINAL generators (see k_ipa_expand).  a = a_lo || a_hi
// (n_k scalars), w1s/w2s = the k fold challenges so far (canonical, host).  L and R go to the host.
template <int C>
static reef_status v_ipa_cross(void *impl, const reef_fe *a, size_t n_k, int loc, bool is_mont, const reef_fe *w1s,
                               const reef_fe *w2s, size_t k, reef_jacobian *out_l, reef_jacobian *out_r) {
    Ctx<C> *ctx = (Ctx<C> *)impl;
    if (!ctx || !a || !out_l || !out_r || (k && (!w1s || !w2s))) { set_error("null argument"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    Key<C> *key = ctx->key;
    REEF_ON_DEVICE(key->device);
    CtxScope<C> scope(ctx);
    REEF_TRY(scope.enter());
    const size_t n = key->n;
    if (k > 31) { set_error("too many IPA rounds"); return REEF_ERR_ARG; }
    if (n_k < 2 || (n_k & (n_k - 1)) || (n_k << k) != n) { set_error("n_k * 2^k must equal the key length (powers of two)"); return REEF_ERR_ARG; }
    const fe256 *d_a = (const fe256 *)a;
    if (loc != REEF_DEVICE) {
        REEF_TRY(ctx->scalars.ensure((2 * n + n_k) * sizeof(fe256)));
        fe256 *stage_a = ctx->scalars.template as<fe256>() + 2 * n;
        REEF_HIP_TRY(hipMemcpyAsync(stage_a, a, n_k * sizeof(fe256), hipMemcpyHostToDevice, ctx->stream));
        d_a = stage_a;
    }
    return ipa_cross_run<C>(ctx, d_a, n_k, is_mont, w1s, w2s, k, nullptr, nullptr, nullptr, nullptr, out_l, out_r);
}

// Commitment over the generators k folds away from the resident key, without the folds: the generators after k rounds of
// G'_i = w1*G_i + w2*G_{i + half} are G^(k)_j = sum_t coef(t) * G_{j + t*n_k} (k_ipa_coef), so
//   sum_{j < len} v[j] * G^(k)_{off + j}  =  MSM over the ORIGINAL key with scalars v[j] * coef(t) at j + off + t*n_k.
template <int C>
static reef_status v_msm_folded(void *impl, const reef_fe *v, size_t len, size_t off, int loc, bool is_mont, const reef_fe *w1s, const reef_fe *w2s,
                                size_t k, reef_jacobian *out, int out_loc) {
    Ctx<C> *ctx = (Ctx<C> *)impl;
    if (!ctx || !out || (len && !v) || (k && (!w1s || !w2s))) { set_error("null argument"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    Key<C> *key = ctx->key;
    REEF_ON_DEVICE(key->device);
    CtxScope<C> scope(ctx);
    REEF_TRY(scope.enter());
    const size_t n = key->n;
    if (k > 31 || n == 0 || ((n >> k) << k) != n) { set_error("the key length must be a multiple of 2^k (k <= 31)"); return REEF_ERR_ARG; }
    const size_t n_k = n >> k;
    if (off > n_k || len > n_k - off) { set_error("slice [%zu, %zu) exceeds the %zu folded generators", off, off + len, n_k); return REEF_ERR_ARG; }
    jacobian256 *d_res = nullptr;
    REEF_TRY(result_target<C>(ctx, 1, out, out_loc, &d_res));
    hipStream_t st = ctx->stream;
    if (len == 0) {
        REEF_HIP_TRY(hipMemsetAsync(d_res, 0, sizeof(jacobian256), st));
        return finish_output<C>(ctx, d_res, 1, out, out_loc);
    }
    REEF_TRY(ctx->scalars.ensure((n + len) * sizeof(fe256)));
    fe256 *expanded = ctx->scalars.template as<fe256>(), *stage = expanded + n;
    const fe256 *d_v = (const fe256 *)v;
    if (loc != REEF_DEVICE) {
        REEF_HIP_TRY(hipMemcpyAsync(stage, v, len * sizeof(fe256), hipMemcpyHostToDevice, st));
        d_v = stage;
    }
    const size_t ncoef = (size_t)1 << k;
    REEF_TRY(ctx->blinds.ensure(ncoef * sizeof(fe256)));
    fe256 *coef = ctx->blinds.template as<fe256>();
    IpaChallenges ch;
    memset(&ch, 0, sizeof ch);
    if (k) {
        memcpy(ch.w1, w1s, k * sizeof(fe256));
        memcpy(ch.w2, w2s, k * sizeof(fe256));
    }
    hipLaunchKernelGGL(k_ipa_coef<C>, dim3(ceil_div(ncoef, 256)), dim3(256), 0, st, ch, (u32)k, coef);
    hipLaunchKernelGGL(k_fold_expand<C>, dim3(ceil_div(n, 256)), dim3(256), 0, st, d_v, (u32)len, (u32)off, (u32)n_k, (const fe256 *)coef, (u32)n, (int)is_mont,
                       expanded);
    return msm_device_scalars<C>(ctx, expanded, n, false, out, out_loc, d_res);
}

// ------------------------------------------------------- stateless helpers ----
// Per-thread grow-only staging buffers for the stateless helpers (fold, normalize, generators ...): no hipMalloc in steady
// state.  The stream of a call comes from the library's pool (common.h) -- the one with the fewest callers at work -- and goes
// back when the call ends; every call waits for what it enqueued before it returns.
struct ScratchPool {
    hipEvent_t ev[2] = {nullptr, nullptr};     // for calls that run two independent kernels side by side (key derivation)
    DevBuf bufs[6];
    int device = -1;
    void drop_events() {
        for (auto &e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    }
    ~ScratchPool() {
        for (auto &b : bufs) b.release();
        drop_events();
    }
};
static ScratchPool &scratch_pool() {
    static thread_local ScratchPool pool;
    return pool;
}
struct ScratchStream {
    hipStream_t s = nullptr;
    PoolStream *ps = nullptr, *ps2 = nullptr;
    bool bg = false, bg2 = false;
    int used = 0;
    reef_status init() {
        ScratchPool &p = scratch_pool();
        int dev = 0;
        REEF_HIP_TRY(hipGetDevice(&dev));
        if (p.device != dev) {  // the caller switched devices: start over on the new one
            for (auto &b : p.bufs) b.release();
            p.drop_events();
            p.device = dev;
        }
        REEF_TRY(stream_pool().pick(dev, &ps, &bg));
        s = ps->s;
        return REEF_OK;
    }
    // the thread's two events (created on first use), for a call that orders its stream against another
    reef_status events(hipEvent_t **ev) {
        ScratchPool &p = scratch_pool();
        if (!p.ev[0])
            for (auto &e : p.ev) REEF_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        *ev = p.ev;
        return REEF_OK;
    }
    // a second stream for the call and the two events
    reef_status side(hipStream_t *s2, hipEvent_t **ev) {
        REEF_TRY(events(ev));
        if (!ps2) REEF_TRY(stream_pool().pick(scratch_pool().device, &ps2, &bg2));
        *s2 = ps2->s;
        return REEF_OK;
    }
    reef_status alloc(void **out, size_t bytes) {
        ScratchPool &p = scratch_pool();
        if (used >= 6) { set_error("scratch pool exhausted"); return REEF_ERR_ARG; }
        DevBuf &b = p.bufs[used++];
        REEF_TRY(b.ensure(bytes ? bytes : 16));
        *out = b.p;
        return REEF_OK;
    }
    ~ScratchStream() {
        if (ps) { (void)hipStreamSynchronize(ps->s); StreamPool::leave(ps, bg); }       // nothing of a call outlives it, on either stream
        if (ps2) { (void)hipStreamSynchronize(ps2->s); StreamPool::leave(ps2, bg2); }
    }
};

template <class T>
static reef_status stage_in(ScratchStream &ss, const T **dev, const void *src, size_t count, int loc) {
    if (loc == REEF_DEVICE) { *dev = (const T *)src; return REEF_OK; }
    void *p = nullptr;
    REEF_TRY(ss.alloc(&p, count * sizeof(T)));
    REEF_HIP_TRY(hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, ss.s));
    *dev = (const T *)p;
    return REEF_OK;
}
template <class T> static reef_status stage_out(ScratchStream &ss, T **dev, void *dst, size_t count, int loc) {
    if (loc == REEF_DEVICE) { *dev = (T *)dst; return REEF_OK; }
    void *p = nullptr;
    REEF_TRY(ss.alloc(&p, count * sizeof(T)));
    *dev = (T *)p;
    return REEF_OK;
}
template <class T> static reef_status finish_out(ScratchStream &ss, T *dev, void *dst, size_t count, int loc) {
    REEF_HIP_TRY(hipGetLastError());
    if (loc != REEF_DEVICE) REEF_HIP_TRY(hipMemcpyAsync(dst, dev, count * sizeof(T), hipMemcpyDeviceToHost, ss.s));
    REEF_HIP_TRY(hipStreamSynchronize(ss.s));
    return REEF_OK;
}

template <int C>
static reef_status v_fold(const reef_affine *gens, size_t half, int loc, const reef_fe *w1, const reef_fe *w2, reef_affine *out) {
    if (!gens || !w1 || !w2 || !out) { set_error("null argument"); return REEF_ERR_ARG; }
    if (half == 0) return REEF_OK;
    ScratchStream ss;
    REEF_TRY(ss.init());
    const affine256 *d_gens;
    affine256 *d_out;
    REEF_TRY(stage_in<affine256>(ss, &d_gens, gens, 2 * half, loc));
    REEF_TRY(stage_out<affine256>(ss, &d_out, out, half, loc));
    void *tmp;
    REEF_TRY(ss.alloc(&tmp, half * sizeof(xyzz_mem)));
    fe256 a, b;
    memcpy(&a, w1, sizeof(fe256));
    memcpy(&b, w2, sizeof(fe256));
    // both scalars split with the curve endomorphism: 128-bit joint double-and-add (k_fold_glv); a scalar that is not
    // canonical (>= r) cannot be split and takes the plain 255-bit chain
    GlvSplit s1, s2;
    if (glv_split<C>(a.w, &s1) && glv_split<C>(b.w, &s2)) {
        GlvScalars sc;
        memcpy(sc.k[0], s1.k1, 20); memcpy(sc.k[1], s1.k2, 20); memcpy(sc.k[2], s2.k1, 20); memcpy(sc.k[3], s2.k2, 20);
        sc.neg[0] = s1.neg1; sc.neg[1] = s1.neg2; sc.neg[2] = s2.neg1; sc.neg[3] = s2.neg2;
        int top = -1;
        for (int j = 0; j < 4; ++j)
            for (int w = 4; w >= 0; --w)
                if (sc.k[j][w]) { top = std::max(top, 32 * w + 31 - __builtin_clz(sc.k[j][w])); break; }
        sc.top = (u32)top;
        void *table;
        REEF_TRY(ss.alloc(&table, 16 * half * sizeof(xyzz_mem)));
        // up to 2^14 outputs the chain's latency is the cost, not the work: four waves per group operation (REEF_MSM_FOLD_COOP=0: one)
        static const bool fold_coop = [] { const char *e = exp_env("REEF_MSM_FOLD_COOP"); return !(e && e[0] == '0'); }();
        if (fold_coop && half <= ((size_t)1 << 14) && top >= 0)
            hipLaunchKernelGGL(k_fold_glv_coop<C>, dim3(ceil_div(half, 64)), dim3(256), 0, ss.s, d_gens, (u32)half, sc, (xyzz_mem *)table, (xyzz_mem *)tmp);
        else
            hipLaunchKernelGGL(k_fold_glv<C>, dim3(ceil_div(half, 256)), dim3(256), 0, ss.s, d_gens, (u32)half, sc, (xyzz_mem *)table, (xyzz_mem *)tmp);
    } else {
        hipLaunchKernelGGL(k_fold<C>, dim3(ceil_div(half, 256)), dim3(256), 0, ss.s, d_gens, (u32)half, a, b, (xyzz_mem *)tmp);
    }
    hipLaunchKernelGGL((k_xyzz_normalize<C, true>), dim3(ceil_div(ceil_div(half, NORM_PER), 256)), dim3(256), 0, ss.s, (const xyzz_mem *)tmp,
                       (u32)half, d_out);
    return finish_out<affine256>(ss, d_out, out, half, loc);
}

// ---- deep fold (K3, deep): G^(k)_j = sum_t s_t * G_{t*n_k + j} in one bucket pass (k_deep_accum) ----
// The 2^k coefficients s_t on the host, canonical integers: s_t = prod_m (bit_{k-1-m}(t) ? w2_m : w1_m), what k_ipa_coef forms.
template <int C> static void deep_coefs(const fe256 *w1s, const fe256 *w2s, size_t k, std::vector<hostcombine::f4> &coef) {
    using namespace hostcombine;
    constexpr int F = 1 - C;
    const Field<F> &fd = field<F>();
    static const f4 r2 = [&] {                        // 2^512 mod r: fmul(w, r2) = w * 2^256, and fmul(s, w * 2^256) = s * w
        f4 v = {{1, 0, 0, 0}};
        for (int i = 0; i < 512; ++i) v = fdbl(fd, v);
        return v;
    }();
    auto load = [](const fe256 &w) {
        f4 v;
        for (int i = 0; i < 4; ++i) v.l[i] = (u64)w.w[2 * i] | ((u64)w.w[2 * i + 1] << 32);
        return v;
    };
    coef.assign(1, f4{{1, 0, 0, 0}});
    for (size_t m = 0; m < k; ++m) {
        const f4 m1 = fmul(fd, load(w1s[m]), r2), m2 = fmul(fd, load(w2s[m]), r2);
        std::vector<f4> next(coef.size() * 2);
        for (size_t t = 0; t < coef.size(); ++t) {
            next[2 * t] = fmul(fd, coef[t], m1);
            next[2 * t + 1] = fmul(fd, coef[t], m2);
        }
        coef.swap(next);
    }
}
// magnitude (nw 32-bit words) -> signed 3-bit digits in [-4, 4] at dig[w * stride], negated when neg; returns the windows used
static inline u32 deep_recode(const u32 *mag, int nw, bool neg, signed char *dig, size_t stride) {
    u32 carry = 0, used = 0;
    for (u32 w = 0; w < DEEP_WMAX; ++w) {
        const u32 bit = DEEP_C * w;
        u32 raw = carry;
        for (u32 b = 0; b < DEEP_C; ++b) {
            const u32 pos = bit + b;
            if ((int)(pos >> 5) < nw) raw += ((mag[pos >> 5] >> (pos & 31u)) & 1u) << b;
        }
        int d = (int)raw;
        carry = 0;
        if (raw > 4) { d = (int)raw - 8; carry = 1; }
        if (d) used = w + 1;
        dig[(size_t)w * stride] = (signed char)(neg ? -d : d);
    }
    return used;
}
// The deep fold of ctx's key on ctx's stream (ctx entered, its key's device current): d_out[j] = G^(k)_j for j < n >> k, ABI affine on the
// device.  Arguments checked by the caller (k <= 31, n a multiple of 2^k, canonical scalars).  Waited for.
template <int C>
static reef_status deep_fold_run(Ctx<C> *ctx, const fe256 *w1s, const fe256 *w2s, size_t k, affine256 *d_out) {
    Key<C> *key = ctx->key;
    const size_t n = key->n, T = (size_t)1 << k, n_k = n >> k;
    if (n_k == 0) return REEF_OK;
    hipStream_t st = ctx->stream;
    std::vector<hostcombine::f4> coef;
    deep_coefs<C>(w1s, w2s, k, coef);
    // the GLV halves of every coefficient; one that does not split (or REEF_FOLD_DEEP_GLV=0 in the +experiment build) sends all of them
    // down the 255-bit form, one half
    const char *glv_env = exp_env("REEF_FOLD_DEEP_GLV");     // read per call: a test sets it for one fold
    const bool glv_on = !(glv_env && glv_env[0] == '0');
    std::vector<GlvSplit> halves(glv_on ? T : 0);
    bool glv = glv_on;
    for (size_t t = 0; t < T && glv; ++t) {
        u32 w8[8];
        for (int i = 0; i < 4; ++i) { w8[2 * i] = (u32)coef[t].l[i]; w8[2 * i + 1] = (u32)(coef[t].l[i] >> 32); }
        glv = glv_split<C>(w8, &halves[t]);
    }
    const u32 H = glv ? 2u : 1u;
    std::vector<signed char> dig((size_t)H * DEEP_WMAX * T);
    u32 W = 1;
    for (size_t t = 0; t < T; ++t) {
        if (glv) {
            W = std::max(W, deep_recode(halves[t].k1, 5, halves[t].neg1, dig.data() + t, T));
            W = std::max(W, deep_recode(halves[t].k2, 5, halves[t].neg2, dig.data() + (size_t)DEEP_WMAX * T + t, T));
        } else {
            u32 w8[8];
            for (int i = 0; i < 4; ++i) { w8[2 * i] = (u32)coef[t].l[i]; w8[2 * i + 1] = (u32)(coef[t].l[i] >> 32); }
            W = std::max(W, deep_recode(w8, 8, false, dig.data() + t, T));
        }
    }
    REEF_TRY(ctx->deep_dig.ensure(dig.size()));
    REEF_HIP_TRY(hipMemcpyAsync(ctx->deep_dig.p, dig.data(), dig.size(), hipMemcpyHostToDevice, st));
    // outputs in slabs of at most 2^14 (the window sums of a slab: 144 B * W * slab); few outputs of many terms split their terms over
    // S chunks (of at least 8) so that the device still sees 2^17 lanes: two waves on every SIMD
    const size_t slab = std::min<size_t>(n_k, (size_t)1 << 14);
    size_t S = std::max<size_t>(1, std::min<size_t>(T / 8, ((size_t)131072 + slab * W - 1) / (slab * W)));
    const u32 t_per = (u32)((T + S - 1) / S);
    S = (T + t_per - 1) / t_per;
    REEF_TRY(ctx->deep_part.ensure((S * W + 1) * slab * sizeof(xyzz_mem)));
    xyzz_mem *part = ctx->deep_part.template as<xyzz_mem>(), *folded = part + S * W * slab;
    const signed char *d_dig = ctx->deep_dig.template as<signed char>();
    for (size_t j0 = 0; j0 < n_k; j0 += slab) {
        const u32 cnt = (u32)std::min(slab, n_k - j0);
        hipLaunchKernelGGL(k_deep_accum<C>, dim3(ceil_div(cnt, 64), W, (u32)S), dim3(64), 0, st, (const affine256 *)key->tables, (u32)n_k, (u32)j0, cnt, (u32)T,
                           t_per, H, d_dig, part);
        if (S > 1) hipLaunchKernelGGL(k_deep_reduce<C>, dim3(ceil_div((u64)W * cnt, 64)), dim3(64), 0, st, part, W * cnt, (u32)S);
        hipLaunchKernelGGL(k_deep_horner_coop<C>, dim3(ceil_div(cnt, 64)), dim3(256), 0, st, (const xyzz_mem *)part, cnt, W, folded);
        hipLaunchKernelGGL((k_xyzz_normalize<C, true>), dim3(ceil_div(ceil_div(cnt, NORM_PER), 256)), dim3(256), 0, st, (const xyzz_mem *)folded, cnt, d_out + j0);
    }
    REEF_HIP_TRY(hipGetLastError());
    REEF_HIP_TRY(hipStreamSynchronize(st));               // the digits' host copy and the workspace are free again
    return REEF_OK;
}
// the argument errors of the deep fold: nothing is written when one is found
template <int C> static reef_status deep_fold_check(Ctx<C> *ctx, const reef_fe *w1s, const reef_fe *w2s, size_t k) {
    using namespace hostcombine;
    const size_t n = ctx->key->n;
    if (k > 31 || ((n >> k) << k) != n) { set_error("the key length (%zu) must be a multiple of 2^k (k = %zu, at most 31)", n, k); return REEF_ERR_ARG; }
    if (ctx->wsplit_world > 1) { set_error("a ctx with a window split cannot fold its key"); return REEF_ERR_ARG; }
    const Field<1 - C> &fd = field<1 - C>();
    for (size_t m = 0; m < k; ++m)
        for (const reef_fe *w : {w1s + m, w2s + m}) {
            fe256 v;
            memcpy(&v, w, sizeof v);
            f4 x;
            for (int i = 0; i < 4; ++i) x.l[i] = (u64)v.w[2 * i] | ((u64)v.w[2 * i + 1] << 32);
            if (geq(x, fd.p)) { set_error("challenge %zu is not below the modulus (canonical integers are expected)", m); return REEF_ERR_ARG; }
        }
    return REEF_OK;
}
template <int C>
static reef_status v_fold_deep(void *impl, const reef_fe *w1s, const reef_fe *w2s, size_t k, reef_affine *out, int out_loc) {
    Ctx<C> *ctx = (Ctx<C> *)impl;
    if (!ctx || !out || (k && (!w1s || !w2s))) { set_error("null argument"); return REEF_ERR_ARG; }
    std::lock_guard<std::mutex> lk(ctx->mu);
    REEF_TRY(deep_fold_check<C>(ctx, w1s, w2s, k));
    Key<C> *key = ctx->key;
    const size_t n_k = key->n >> k;
    if (n_k == 0) return REEF_OK;
    REEF_ON_DEVICE(key->device);
    CtxScope<C> scope(ctx);
    REEF_TRY(scope.enter());
    if (out_loc == REEF_DEVICE) return deep_fold_run<C>(ctx, (const fe256 *)w1s, (const fe256 *)w2s, k, (affine256 *)out);
    REEF_TRY(ctx->hpoint.ensure(n_k * sizeof(affine256)));
    REEF_TRY(deep_fold_run<C>(ctx, (const fe256 *)w1s, (const fe256 *)w2s, k, ctx->hpoint.template as<affine256>()));
    REEF_HIP_TRY(hipMemcpyAsync(out, ctx->hpoint.p, n_k * sizeof(affine256), hipMemcpyDeviceToHost, ctx->stream));
    REEF_HIP_TRY(hipStreamSynchronize(ctx->stream));
    return REEF_OK;
}
// A resident key of the folded points: the deep fold into a device buffer, then the key built from it.  Nothing visits the host.
template <int C>
static reef_status v_ctx_create_folded(void **impl, void *src_, const reef_fe *w1s, const reef_fe *w2s, size_t k, const reef_msm_opts *opts) {
    Ctx<C> *src = (Ctx<C> *)src_;
    if (!impl || !src || (k && (!w1s || !w2s))) { set_error("null argument"); return REEF_ERR_ARG; }
    reef_msm_opts o = {};
    if (opts) o = *opts;
    o.device = src->key->device;
    REEF_ON_DEVICE(src->key->device);
    DevBuf pts;
    struct Release {
        DevBuf &b;
        ~Release() { b.release(); }
    } release{pts};
    size_t n_k = 0;
    {
        std::lock_guard<std::mutex> lk(src->mu);
        REEF_TRY(deep_fold_check<C>(src, w1s, w2s, k));
        n_k = src->key->n >> k;
        REEF_TRY(plan_for(n_k, o.window_bits, o.bucket_groups, nullptr, nullptr, nullptr, nullptr));
        CtxScope<C> scope(src);
        REEF_TRY(scope.enter());
        REEF_TRY(pts.ensure(std::max<size_t>(n_k, 1) * sizeof(affine256)));
        REEF_TRY(deep_fold_run<C>(src, (const fe256 *)w1s, (const fe256 *)w2s, k, (affine256 *)pts.p));
    }
    return v_ctx_create<C>(impl, (const reef_affine *)pts.p, n_k, REEF_DEVICE, &o);
}

template <int C>
static reef_status v_normalize(const reef_jacobian *in, size_t n, int loc, reef_affine *out_aff, uint8_t *out_comp) {
    if (!in || (!out_aff && !out_comp)) { set_error("null argument"); return REEF_ERR_ARG; }
    if (n == 0) return REEF_OK;
    ScratchStream ss;
    REEF_TRY(ss.init());
    const jacobian256 *d_in;
    REEF_TRY(stage_in<jacobian256>(ss, &d_in, in, n, loc));
    affine256 *d_aff = nullptr;
    fe256 *d_comp = nullptr;
    if (out_aff) REEF_TRY(stage_out<affine256>(ss, &d_aff, out_aff, n, loc));
    if (out_comp) REEF_TRY(stage_out<fe256>(ss, &d_comp, out_comp, n, loc));
    hipLaunchKernelGGL(k_normalize<C>, dim3(ceil_div(ceil_div(n, NORM_PER), 256)), dim3(256), 0, ss.s, d_in, (u32)n, d_aff, d_comp);
    REEF_HIP_TRY(hipGetLastError());
    if (loc != REEF_DEVICE) {
        if (out_aff) REEF_HIP_TRY(hipMemcpyAsync(out_aff, d_aff, n * sizeof(affine256), hipMemcpyDeviceToHost, ss.s));
        if (out_comp) REEF_HIP_TRY(hipMemcpyAsync(out_comp, d_comp, n * sizeof(fe256), hipMemcpyDeviceToHost, ss.s));
    }
    REEF_HIP_TRY(hipStreamSynchronize(ss.s));
    return REEF_OK;
}

// K4's inverse (decompress_kernels.inc).  The decode of n encodings on stream s, device pointers; stats: two 64-bit words on the device
// (how many were invalid, the lowest such index: all ones when none).  The root is the windowed one; the +experiment build takes
// REEF_DECOMPRESS_ROOT=0 for Tonelli-Shanks (tools/time_decompress.py compares the two).
template <int C>
static void decompress_launch(hipStream_t s, const fe256 *d_in, size_t n, affine256 *d_out, unsigned long long *d_stats, hipEvent_t before_kernel = nullptr) {
    const char *e = exp_env("REEF_DECOMPRESS_ROOT");
    (void)hipMemsetAsync(d_stats, 0, sizeof(u64), s);
    (void)hipMemsetAsync(d_stats + 1, 0xff, sizeof(u64), s);
    if (before_kernel) (void)hipEventRecord(before_kernel, s);
    if (e && e[0] == '0') hipLaunchKernelGGL((k_decompress<C, false>), dim3(ceil_div(n, 64)), dim3(64), 0, s, d_in, (u32)n, d_out, d_stats);
    else hipLaunchKernelGGL((k_decompress<C, true>), dim3(ceil_div(n, 64)), dim3(64), 0, s, d_in, (u32)n, d_out, d_stats);
}
template <int C>
static reef_status v_decompress(const uint8_t *in, size_t n, int loc, reef_affine *out_aff, uint64_t *invalid, uint64_t *first_invalid) {
    if (n && (!in || !out_aff)) { set_error("null argument"); return REEF_ERR_ARG; }
    if (n >= (1ull << 32)) { set_error("reef_decompress: %zu encodings, the limit is 2^32 - 1", n); return REEF_ERR_ARG; }
    if (loc == REEF_DEVICE && (((uintptr_t)in | (uintptr_t)out_aff) & 15)) { set_error("reef_decompress: device buffers must be 16-byte aligned"); return REEF_ERR_ARG; }
    if (invalid) *invalid = 0;
    if (first_invalid) *first_invalid = n;
    if (n == 0) return REEF_OK;
    ScratchStream ss;
    REEF_TRY(ss.init());
    const fe256 *d_in;
    affine256 *d_out;
    void *d_stats;
    REEF_TRY(stage_in<fe256>(ss, &d_in, in, n, loc));
    REEF_TRY(stage_out<affine256>(ss, &d_out, out_aff, n, loc));
    REEF_TRY(ss.alloc(&d_stats, 2 * sizeof(u64)));
    // the +experiment build times the kernel alone on request and leaves the figure where reef_last_error() finds it (the call still returns REEF_OK)
    const bool timed = exp_env("REEF_DECOMPRESS_EVENTS") != nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (timed) {
        REEF_HIP_TRY(hipEventCreate(&e0));
        REEF_HIP_TRY(hipEventCreate(&e1));
    }
    decompress_launch<C>(ss.s, d_in, n, d_out, (unsigned long long *)d_stats, e0);
    if (timed) REEF_HIP_TRY(hipEventRecord(e1, ss.s));
    REEF_HIP_TRY(hipGetLastError());
    u64 stats[2] = {0, 0};
    REEF_HIP_TRY(hipMemcpyAsync(stats, d_stats, sizeof stats, hipMemcpyDeviceToHost, ss.s));
    REEF_TRY(finish_out<affine256>(ss, d_out, out_aff, n, loc));
    if (invalid) *invalid = stats[0];
    if (first_invalid) *first_invalid = stats[0] ? stats[1] : n;
    if (timed) {
        float ms = 0;
        REEF_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        set_error("reef_decompress: kernel %.3f us", ms * 1e3);
    }
    return REEF_OK;
}

template <int C> static reef_status v_sum_points(const reef_jacobian *in, size_t n, int loc, reef_jacobian *out) {
    if (!in || !out || n > 65536) { set_error("bad argument"); return REEF_ERR_ARG; }
    ScratchStream ss;
    REEF_TRY(ss.init());
    const jacobian256 *d_in;
    jacobian256 *d_out;
    REEF_TRY(stage_in<jacobian256>(ss, &d_in, in, n, loc));
    REEF_TRY(stage_out<jacobian256>(ss, &d_out, out, 1, loc));
    hipLaunchKernelGGL(k_sum_points<C>, dim3(1), dim3(64), 0, ss.s, d_in, (u32)n, d_out);
    return finish_out<jacobian256>(ss, d_out, out, 1, loc);
}

template <int C> static reef_status v_gen_bases(uint64_t k0, uint64_t d, size_t n, reef_affine *out, int loc) {
    if (!out && n) { set_error("null argument"); return REEF_ERR_ARG; }
    if (n == 0) return REEF_OK;
    ScratchStream ss;
    REEF_TRY(ss.init());
    affine256 *d_out;
    REEF_TRY(stage_out<affine256>(ss, &d_out, out, n, loc));
    void *tmp;
    REEF_TRY(ss.alloc(&tmp, n * sizeof(xyzz_mem)));
    const u32 per = 16;
    hipLaunchKernelGGL(k_gen_bases_ap<C>, dim3(ceil_div(ceil_div(n, per), 256)), dim3(256), 0, ss.s, k0, d, (u32)n, per, (xyzz_mem *)tmp);
    hipLaunchKernelGGL((k_xyzz_normalize<C, true>), dim3(ceil_div(ceil_div(n, NORM_PER), 256)), dim3(256), 0, ss.s, (const xyzz_mem *)tmp, (u32)n,
                       d_out);
    return finish_out<affine256>(ss, d_out, out, n, loc);
}

template <int C>
static reef_status v_gen_scalars(uint64_t seed, int kind, uint64_t small_bound, size_t n, bool to_mont, reef_fe *out, int loc) {
    if (!out && n) { set_error("null argument"); return REEF_ERR_ARG; }
    if (n == 0) return REEF_OK;
    ScratchStream ss;
    REEF_TRY(ss.init());
    fe256 *d_out;
    REEF_TRY(stage_out<fe256>(ss, &d_out, out, n, loc));
    hipLaunchKernelGGL(k_gen_scalars<C>, dim3(ceil_div(n, 256)), dim3(256), 0, ss.s, seed, kind, small_bound, (u32)n, (int)to_mont, d_out);
    return finish_out<fe256>(ss, d_out, out, n, loc);
}

template <int C> static reef_status v_test_field_op(int op, const reef_fe *a, const reef_fe *b, reef_fe *out, size_t n) {
    if (!a || !b || !out) { set_error("null argument"); return REEF_ERR_ARG; }
    if (n == 0) return REEF_OK;
    ScratchStream ss;
    REEF_TRY(ss.init());
    const fe256 *da, *db;
    fe256 *dout;
    REEF_TRY(stage_in<fe256>(ss, &da, a, n, REEF_HOST));
    REEF_TRY(stage_in<fe256>(ss, &db, b, n, REEF_HOST));
    REEF_TRY(stage_out<fe256>(ss, &dout, out, n, REEF_HOST));
    if (op == 8) hipLaunchKernelGGL((k_test_sqrt<C, true>), dim3(ceil_div(n, 64)), dim3(64), 0, ss.s, da, dout, (u32)n);          // the root that ships
    else if (op == 9) hipLaunchKernelGGL((k_test_sqrt<C, false>), dim3(ceil_div(n, 64)), dim3(64), 0, ss.s, da, dout, (u32)n);   // Tonelli-Shanks
    else hipLaunchKernelGGL(k_test_field<C>, dim3(ceil_div(n, 64)), dim3(64), 0, ss.s, op, da, db, dout, (u32)n);
    return finish_out<fe256>(ss, dout, out, n, REEF_HOST);
}

template <int C>
static reef_status v_test_ec_op(int op, const reef_affine *p, const reef_affine *q, const reef_fe *k, reef_jacobian *out, size_t n) {
    if (!p || !q || !k || !out) { set_error("null argument"); return REEF_ERR_ARG; }
    if (n == 0) return REEF_OK;
    ScratchStream ss;
    REEF_TRY(ss.init());
    const affine256 *dp, *dq;
    const fe256 *dk;
    jacobian256 *dout;
    REEF_TRY(stage_in<affine256>(ss, &dp, p, n, REEF_HOST));
    REEF_TRY(stage_in<affine256>(ss, &dq, q, n, REEF_HOST));
    REEF_TRY(stage_in<fe256>(ss, &dk, k, n, REEF_HOST));
    REEF_TRY(stage_out<jacobian256>(ss, &dout, out, n, REEF_HOST));
    if (op == 19) hipLaunchKernelGGL(k_test_dd<C>, dim3(ceil_div(n, 64)), dim3(256), 0, ss.s, op, dp, dout, (u32)n);
    else if ((op >= 4 && op <= 8) || (op >= 11 && op <= 18) || (op >= 20 && op <= 22)) hipLaunchKernelGGL(k_test_ec_coop<C>, dim3(ceil_div(n, 64)), dim3(256), 0, ss.s, op, dp, dq, dout, (u32)n);
    else hipLaunchKernelGGL(k_test_ec<C>, dim3(ceil_div(n, 64)), dim3(64), 0, ss.s, op, dp, dq, dk, dout, (u32)n);
    return finish_out<jacobian256>(ss, dout, out, n, REEF_HOST);
}

template <int C> static reef_status v_bench_fmul(uint32_t iters, double *per_s) {
    ScratchStream ss;
    REEF_TRY(ss.init());
    const u32 threads = 256 * 256 * 8;  // 8 blocks of 256 per CU
    void *buf;
    REEF_TRY(ss.alloc(&buf, (size_t)threads * 2 * sizeof(fe256)));
    hipLaunchKernelGGL(k_gen_scalars<1 - C>, dim3(2 * threads / 256), dim3(256), 0, ss.s, 99ull, 0, 0ull, 2 * threads, 0, (fe256 *)buf);
    hipEvent_t e0, e1;
    REEF_HIP_TRY(hipEventCreate(&e0));
    REEF_HIP_TRY(hipEventCreate(&e1));
    hipLaunchKernelGGL(k_bench_fmul<C>, dim3(threads / 256), dim3(256), 0, ss.s, (fe256 *)buf, 8u);  // warm-up
    REEF_HIP_TRY(hipEventRecord(e0, ss.s));
    hipLaunchKernelGGL(k_bench_fmul<C>, dim3(threads / 256), dim3(256), 0, ss.s, (fe256 *)buf, iters);
    REEF_HIP_TRY(hipEventRecord(e1, ss.s));
    REEF_HIP_TRY(hipEventSynchronize(e1));
    float ms = 0;
    REEF_HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *per_s = (double)threads * iters * 2.0 / (ms * 1e-3);
    return REEF_OK;
}

}  // namespace reef
#include "sumcheck_engine.inc"
#include "mle_engine.inc"
#include "merkle_engine.inc"
#include "keygen_engine.inc"
namespace reef {

// Plan the engine would use for an n-point key (pure host logic, no device needed).  Everything a later
// reef_msm on the key depends on is validated here, so an unsupported combination is rejected when the
// key is created (or re-keyed), never at MSM time: the bucket keys of one MSM must fit the scan
// (G * 2^(c-1) <= MAX_SCAN_KEYS) and its digits a 32-bit index (n * W < 2^32, n < 2^27).
static reef_status plan_for(size_t n, uint32_t c_opt, uint32_t g_opt, uint32_t *c, uint32_t *w, uint32_t *g, uint32_t *t) {
    if (n >= (1ull << 27)) { set_error("key too large (%zu points; the limit is 2^27 - 1)", n); return REEF_ERR_ARG; }
    u32 cc = c_opt ? c_opt : choose_window(n, g_opt);
    if (cc < 2 || cc > 20) { set_error("window_bits %u out of range [2,20]", cc); return REEF_ERR_ARG; }
    auto groups_of = [&](u32 cw) { const u32 W = windows_for(cw); return g_opt == 0 ? W : std::min(g_opt, W); };
    auto fits = [&](u32 cw) {
        return ((u64)groups_of(cw) << (cw - 1)) <= MAX_SCAN_KEYS && (u64)n * windows_for(cw) < (1ull << 32);
    };
    if (!c_opt) {
        // the cost model may ask for more bucket keys than one scan holds (G = W at n >= 2^24 wants c = 20,
        // 13 * 2^19 keys): take the nearest window that fits -- smaller first (fewer keys), then larger (fewer digits)
        u32 pick = 0;
        for (u32 d = 0; d <= 18 && !pick; ++d) {
            if (cc >= 2 + d && fits(cc - d)) pick = cc - d;
            else if (cc + d <= 20 && fits(cc + d)) pick = cc + d;
        }
        if (!pick) { set_error("no window size fits a key of %zu points with bucket_groups = %u", n, g_opt); return REEF_ERR_ARG; }
        cc = pick;
    } else if (!fits(cc)) {
        set_error("window_bits = %u with bucket_groups = %u needs %llu bucket keys / %llu digits for %zu points (limits: %u keys, 2^32 digits)",
                  cc, g_opt, (unsigned long long)((u64)groups_of(cc) << (cc - 1)), (unsigned long long)((u64)n * windows_for(cc)), n, MAX_SCAN_KEYS);
        return REEF_ERR_ARG;
    }
    const u32 W = windows_for(cc);
    const u32 G = groups_of(cc);
    if (c) *c = cc;
    if (w) *w = W;
    if (g) *g = G;
    if (t) *t = ceil_div(W, G);
    return REEF_OK;
}

template <int C> static CurveVTable make_vtable() {
    return CurveVTable{v_ctx_create<C>, v_ctx_rekey<C>, v_ctx_clone<C>, v_ctx_attach<C>, v_ctx_destroy<C>, v_ctx_sync<C>, v_ctx_stream<C>,
                       v_ctx_timing<C>, v_ctx_enable_timing<C>, v_ctx_window_split<C>, v_ctx_timing_stats<C>, v_ctx_rowcol_forms<C>, v_ctx_sum_points<C>, v_ctx_plan<C>, v_ctx_byte_tables<C>, v_msm<C>, v_msm_rows<C>, v_msm_rows_symbols<C>, v_msm_rows_symbols_wide<C>, v_ipa_cross<C>, v_msm_folded<C>, v_fold<C>, v_normalize<C>, v_sum_points<C>,
                       v_gen_bases<C>, v_gen_scalars<C>, v_test_field_op<C>, v_test_ec_op<C>, v_bench_fmul<C>,
                       v_sc_create<C>, v_sc_destroy<C>, v_sc_set<C>, v_sc_set_parts<C>, v_sc_read<C>, v_sc_lookup<C>, v_sc_coeffs<C>, v_sc_fold<C>, v_sc_fold_coeffs<C>, v_sc_gen_eq<C>, v_sc_reset<C>, v_sc_sync<C>, v_mle_bound<C>, v_merkle_commit<C>, v_derive_generators<C>, plan_for, v_decompress<C>, doc_check, doc_transform,
                       v_fold_deep<C>, v_ctx_create_folded<C>};
}

}  // namespace reef
