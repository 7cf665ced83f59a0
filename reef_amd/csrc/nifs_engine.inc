// Host side of row N6 (the NIFS fold of one step: nifs_kernels.inc); included after engine.inc.
namespace reef {

template <int C> struct SpartanState;                     // row N5 on the same ctx (spartan_engine.inc)
template <int C> static void spartan_release(SpartanState<C> *s);

// The lines of a matrix triple (rows of the CSR, or columns of the CSC copy) that k_nifs_rows_short leaves to k_nifs_rows_long:
// their indices, their segments (nifs_kernels.inc) and the segments' partial sums.
struct NifsSegs {
    DevBuf long_rows, seg_row, seg_first, part;
    u32 nlong = 0, nseg = 0;
    bool prepared = false;               // up to date with the three matrices
    void release() {
        for (DevBuf *b : {&long_rows, &seg_row, &seg_first, &part}) b->release();
        prepared = false;
    }
};

template <int C> struct NifsCtx : DeviceCtx {   // ev: orders the key ctx's stream after the upload of z2 (commit_T) and after the IPA rounds
    static constexpr int F = 1 - C;      // scalar field of curve C
    size_t num_cons = 0, num_vars = 0, num_io = 0, nz = 0;   // nz = num_vars + 1 + num_io
    DevBuf rowptr[3], ent[3], side[3];   // CSR of A, B, C: row pointers, {col, class} per entry, general coefficients by entry
    std::vector<u32> h_rowptr[3];        // host copies: the long-row list is made from them
    bool has[3] = {false, false, false};
    NifsSegs rows;                       // long rows of the CSR
    DevBuf colptr[3], cent[3], cside[3]; // row N5: the column-major copy of A, B, C ({row, class} per entry), built by set_matrix
    std::vector<u32> h_colptr[3];
    NifsSegs cols;                       // long columns of the CSC
    SpartanState<C> *sp = nullptr;       // row N5 workspace, made by the first reef_spartan_begin
    size_t open_n_small = 0;             // reef_spartan_open_set_small_key: the openings begun from now on move to a folded key at this length (0: never)
    struct EvalWs { DevBuf pts, ex, zy, partial, out; } evw;   // the verifier's matrix evaluations (3k): eq factors, eq(r_x) by row, the column
                                         // weights, block sums, results; empty until the first reef_spartan_eval_matrices
    struct EvalBatchWs {                 // the same at many points (3o), its own buffers: the single call's workspace and launches stay as they are
        DevBuf pts, tab, partial, part, out;   // every point's eq factors; the eq tables of one group (ex of its points, then zy); block sums by
                                         // point; the long rows' segment sums by pair; 3 m results
        size_t budget = 0;               // reef_nifs_set_eval_workspace: bytes of tab a call may use (0: the default)
        size_t groups = 0, per_group = 0;   // the last batch (reef_spartan_eval_matrices_batch_last_info); groups == 0: none yet
    } evb;
    u64 gen = 0;                         // bumped by every call that changes the matrices or the running instance (or commits T)
    DevBuf z1, z2, E, step, run, pts, stage, counters;   // step: the rows W2 and T of the step's commitments, run: W and E (commit_running),
                                         // both two rows of row_len() canonical integers with zero tails; pts: two points
    bool running = false, committed = false, have_t = false, have_z2 = false;
    fe256 k254 = {};
    size_t row_len() const { return std::max(num_vars, num_cons); }
    fe256 *w2_row() { return step.template as<fe256>(); }
    fe256 *t_row() { return step.template as<fe256>() + row_len(); }      // T of the last commit_T / commit_step
};

// Every call enqueues on a pool stream and waits for it before it returns: the ctx holds no stream between calls
// (common.h: OnExit::WAIT_AND_IDLE).
template <int C> static void nifs_free(NifsCtx<C> *c) {
    if (!c) return;
    retire_device_ctx(c);
    for (int k = 0; k < 3; ++k)
        for (DevBuf *b : {&c->rowptr[k], &c->ent[k], &c->side[k], &c->colptr[k], &c->cent[k], &c->cside[k]}) b->release();
    c->rows.release();
    c->cols.release();
    spartan_release<C>(c->sp);
    for (DevBuf *b : {&c->z1, &c->z2, &c->E, &c->step, &c->run, &c->pts, &c->stage, &c->counters}) b->release();
    for (DevBuf *b : {&c->evw.pts, &c->evw.ex, &c->evw.zy, &c->evw.partial, &c->evw.out}) b->release();
    for (DevBuf *b : {&c->evb.pts, &c->evb.tab, &c->evb.partial, &c->evb.part, &c->evb.out}) b->release();
    delete c;
}

template <int C> static reef_status v_nifs_create(void **impl, size_t num_cons, size_t num_vars, size_t num_io, int device) {
    if (!impl || num_cons == 0 || num_cons >= (1ull << 31) || num_vars + 1 + num_io >= (1ull << 31)) {
        set_error("reef_nifs_create: need 0 < num_cons < 2^31 and num_vars + 1 + num_io < 2^31");
        return REEF_ERR_ARG;
    }
    return create_device_ctx<NifsCtx<C>>(impl, device, "reef_nifs_create", true, nifs_free<C>, [&](NifsCtx<C> *c) -> reef_status {
        c->num_cons = num_cons;
        c->num_vars = num_vars;
        c->num_io = num_io;
        c->nz = num_vars + 1 + num_io;
        fe x254 = fe_zero();
        x254.l[8] = 1u << 22;                // 2^(8 * 29 + 22)
        REEF_SET_BOUND(x254, 1.0);
        constexpr int F = NifsCtx<C>::F;
        c->k254 = fe_to_table<F>(fe_mul<F>(x254, fe_const<F>(FC<F>::C_R2, 1.0)));     // 2^254 R'
        for (DevBuf *b : {&c->z1, &c->z2}) REEF_TRY(b->ensure(c->nz * sizeof(fe256)));
        REEF_TRY(c->E.ensure(num_cons * sizeof(fe256)));
        REEF_TRY(c->step.ensure(2 * c->row_len() * sizeof(fe256)));
        REEF_HIP_TRY(hipMemset(c->step.p, 0, 2 * c->row_len() * sizeof(fe256)));   // the rows' tails: nothing writes them afterwards
        REEF_TRY(c->pts.ensure(2 * sizeof(jacobian256)));
        return c->counters.ensure(2 * sizeof(u32));
    });
}
template <int C> static void v_nifs_destroy(void *impl) { nifs_free((NifsCtx<C> *)impl); }

template <int C>
static reef_status v_nifs_set_matrix(void *impl, int which, const uint32_t *row, const uint32_t *col, const reef_fe *val, size_t nnz, bool is_mont) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    if (which < 0 || which > 2) { set_error("reef_nifs_set_matrix: which must be 0 (A), 1 (B) or 2 (C)"); return REEF_ERR_ARG; }
    if (nnz && (!row || !col || !val)) { set_error("null argument"); return REEF_ERR_ARG; }
    if (nnz >= (1ull << 32)) { set_error("reef_nifs_set_matrix: at most 2^32 - 1 entries per matrix"); return REEF_ERR_ARG; }
    // counting sort by row on the host (any order in, CSR out; duplicates stay separate entries: a dot product sums them)
    std::vector<u32> ptr(c->num_cons + 1, 0);
    for (size_t e = 0; e < nnz; ++e) {
        if (row[e] >= c->num_cons || col[e] >= c->nz) {
            set_error("reef_nifs_set_matrix: entry %zu (row %u, col %u) outside %zu x %zu", e, row[e], col[e], c->num_cons, c->nz);
            return REEF_ERR_ARG;
        }
        ++ptr[row[e] + 1];
    }
    for (size_t i = 0; i < c->num_cons; ++i) ptr[i + 1] += ptr[i];
    std::vector<u32> fill(ptr.begin(), ptr.end() - 1), cols(nnz);
    std::vector<reef_fe> vals(nnz);
    for (size_t e = 0; e < nnz; ++e) {
        const u32 p = fill[row[e]]++;
        cols[p] = col[e];
        vals[p] = val[e];
    }
    // and by column (row N5's ABC pass: one line per column of z), from the CSR so that a column's entries go by row
    std::vector<u32> cptr(c->nz + 1, 0), crows(nnz);
    std::vector<reef_fe> cvals(nnz);
    for (size_t e = 0; e < nnz; ++e) ++cptr[cols[e] + 1];
    for (size_t j = 0; j < c->nz; ++j) cptr[j + 1] += cptr[j];
    {
        std::vector<u32> cfill(cptr.begin(), cptr.end() - 1);
        for (size_t i = 0; i < c->num_cons; ++i)
            for (u32 e = ptr[i]; e < ptr[i + 1]; ++e) {
                const u32 p = cfill[cols[e]]++;
                crows[p] = (u32)i;
                cvals[p] = vals[e];
            }
    }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(call.enter());
    c->has[which] = false;
    c->rows.prepared = c->cols.prepared = false;
    ++c->gen;
    REEF_TRY(c->rowptr[which].ensure(ptr.size() * sizeof(u32)));
    REEF_TRY(c->ent[which].ensure(std::max<size_t>(1, nnz) * sizeof(uint2)));
    REEF_TRY(c->side[which].ensure(std::max<size_t>(1, nnz) * sizeof(fe256)));
    REEF_TRY(c->colptr[which].ensure(cptr.size() * sizeof(u32)));
    REEF_TRY(c->cent[which].ensure(std::max<size_t>(1, nnz) * sizeof(uint2)));
    REEF_TRY(c->cside[which].ensure(std::max<size_t>(1, nnz) * sizeof(fe256)));
    REEF_TRY(c->stage.ensure(std::max<size_t>(1, 2 * nnz) * sizeof(u32)));
    REEF_HIP_TRY(hipMemcpyAsync(c->rowptr[which].p, ptr.data(), ptr.size() * sizeof(u32), hipMemcpyHostToDevice, c->stream));
    if (nnz) {
        REEF_HIP_TRY(hipMemcpyAsync(c->stage.p, cols.data(), nnz * sizeof(u32), hipMemcpyHostToDevice, c->stream));
        REEF_HIP_TRY(hipMemcpyAsync(c->side[which].p, vals.data(), nnz * sizeof(fe256), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_nifs_classify<NifsCtx<C>::F>, dim3(ceil_div(nnz, 256)), dim3(256), 0, c->stream, c->stage.template as<u32>(), (u32)nnz,
                           (int)is_mont, c->ent[which].template as<uint2>(), c->side[which].template as<fe256>());
        u32 *srows = c->stage.template as<u32>() + nnz;
        REEF_HIP_TRY(hipMemcpyAsync(srows, crows.data(), nnz * sizeof(u32), hipMemcpyHostToDevice, c->stream));
        REEF_HIP_TRY(hipMemcpyAsync(c->cside[which].p, cvals.data(), nnz * sizeof(fe256), hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_nifs_classify<NifsCtx<C>::F>, dim3(ceil_div(nnz, 256)), dim3(256), 0, c->stream, (const u32 *)srows, (u32)nnz,
                           (int)is_mont, c->cent[which].template as<uint2>(), c->cside[which].template as<fe256>());
        REEF_HIP_TRY(hipGetLastError());
    }
    REEF_HIP_TRY(hipMemcpyAsync(c->colptr[which].p, cptr.data(), cptr.size() * sizeof(u32), hipMemcpyHostToDevice, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));   // the host vectors go out of scope
    c->h_rowptr[which].swap(ptr);
    c->h_colptr[which].swap(cptr);
    c->has[which] = true;
    return REEF_OK;
}

// the lines k_nifs_rows_short leaves to k_nifs_rows_long (after the matrices changed): rows of the CSR, or columns of the CSC
template <int C> static reef_status nifs_segments(NifsCtx<C> *c, const std::vector<u32> (&hptr)[3], size_t n, NifsSegs &sg) {
    if (sg.prepared) return REEF_OK;
    std::vector<u32> rows, seg_row, seg_first(1, 0);
    for (size_t i = 0; i < n; ++i) {
        size_t len = 0, longest = 0;
        for (int k = 0; k < 3; ++k) {
            const size_t lk = hptr[k][i + 1] - hptr[k][i];
            len += lk;
            longest = std::max(longest, lk);
        }
        if (len <= NIFS_LONG_ROW) continue;
        const u32 segs = (u32)((longest + NIFS_SEG - 1) / NIFS_SEG);
        seg_row.insert(seg_row.end(), segs, (u32)rows.size());
        rows.push_back((u32)i);
        seg_first.push_back(seg_first.back() + segs);
    }
    sg.nlong = (u32)rows.size();
    sg.nseg = (u32)seg_row.size();
    REEF_TRY(sg.long_rows.ensure(std::max<size_t>(1, rows.size()) * sizeof(u32)));
    REEF_TRY(sg.seg_row.ensure(std::max<size_t>(1, seg_row.size()) * sizeof(u32)));
    REEF_TRY(sg.seg_first.ensure(seg_first.size() * sizeof(u32)));
    REEF_TRY(sg.part.ensure(std::max<size_t>(1, seg_row.size()) * 6 * sizeof(fe_limbs)));
    if (!rows.empty()) {
        REEF_HIP_TRY(hipMemcpyAsync(sg.long_rows.p, rows.data(), rows.size() * sizeof(u32), hipMemcpyHostToDevice, c->stream));
        REEF_HIP_TRY(hipMemcpyAsync(sg.seg_row.p, seg_row.data(), seg_row.size() * sizeof(u32), hipMemcpyHostToDevice, c->stream));
        REEF_HIP_TRY(hipMemcpyAsync(sg.seg_first.p, seg_first.data(), seg_first.size() * sizeof(u32), hipMemcpyHostToDevice, c->stream));
        REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    }
    sg.prepared = true;
    return REEF_OK;
}
template <int C> static reef_status nifs_prepare(NifsCtx<C> *c) {
    if (!c->has[0] || !c->has[1] || !c->has[2]) { set_error("reef_nifs: set the matrices A, B and C first"); return REEF_ERR_ARG; }
    return nifs_segments(c, c->h_rowptr, c->num_cons, c->rows);
}

template <int C> static NifsArgs nifs_args(NifsCtx<C> *c) {
    NifsArgs a;
    memset(&a, 0, sizeof a);
    for (int k = 0; k < 3; ++k) a.m[k] = NifsMat{c->rowptr[k].template as<u32>(), c->ent[k].template as<uint2>(), c->side[k].template as<fe256>()};
    a.z1 = c->z1.template as<fe256>();
    a.z2 = c->z2.template as<fe256>();
    a.E = c->E.template as<fe256>();
    a.T = c->t_row();
    a.num_cons = (u32)c->num_cons;
    a.num_vars = (u32)c->num_vars;
    a.k254 = c->k254;
    a.viol = c->counters.template as<u32>();
    a.first_bad = a.viol + 1;
    a.long_rows = c->rows.long_rows.template as<u32>();
    a.nlong = c->rows.nlong;
    return a;
}
// one pass over the lines of a (the rows, or for MODE_ABC the columns: a.num_cons lines) with the long ones of sg
template <int C, int MODE> static reef_status nifs_line_pass(const NifsArgs &a, const NifsSegs &sg, hipStream_t s) {
    hipLaunchKernelGGL((k_nifs_rows_short<NifsCtx<C>::F, MODE>), dim3(ceil_div(a.num_cons, 256)), dim3(256), 0, s, a);
    if (sg.nlong) {
        const u32 *seg_row = sg.seg_row.template as<u32>(), *seg_first = sg.seg_first.template as<u32>();
        fe_limbs *part = sg.part.template as<fe_limbs>();
        hipLaunchKernelGGL((k_nifs_rows_long<NifsCtx<C>::F, MODE>), dim3(sg.nseg), dim3(256), 0, s, a, seg_row, seg_first, part);
        hipLaunchKernelGGL((k_nifs_rows_finish<NifsCtx<C>::F, MODE>), dim3(sg.nlong), dim3(64), 0, s, a, seg_first, (const fe_limbs *)part);
    }
    REEF_HIP_TRY(hipGetLastError());
    return REEF_OK;
}
template <int C, int MODE> static reef_status nifs_row_pass(NifsCtx<C> *c, hipStream_t s) { return nifs_line_pass<C, MODE>(nifs_args(c), c->rows, s); }

// n elements of the caller's (host or device) buffer into dst, in the caller's form: dst holds them raw until k_fe_import
template <int C> static reef_status nifs_copy_in(NifsCtx<C> *c, fe256 *dst, const reef_fe *src, size_t n, int loc) {
    if (!n) return REEF_OK;
    REEF_HIP_TRY(hipMemcpyAsync(dst, src, n * sizeof(fe256), loc == REEF_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    return REEF_OK;
}
// z = w || 1 (or u) || x, raw, then converted in place
template <int C>
static reef_status nifs_load_z(NifsCtx<C> *c, fe256 *z, const reef_fe *w, const reef_fe *u, const reef_fe *x, int loc, bool is_mont) {
    constexpr int F = NifsCtx<C>::F;
    REEF_TRY(nifs_copy_in(c, z, w, c->num_vars, loc));
    if (u) REEF_TRY(nifs_copy_in(c, z + c->num_vars, u, 1, loc));
    else {
        static fe256 one_raw[2];             // the one of z2 in either form: canonical 1, or pasta Montgomery form
        static std::once_flag once;
        std::call_once(once, [] {
            memset(one_raw, 0, sizeof one_raw);
            one_raw[0].w[0] = 1;
            one_raw[1] = fe_to_abi<F>(fe_one<F>());
        });
        REEF_HIP_TRY(hipMemcpyAsync(z + c->num_vars, &one_raw[is_mont ? 1 : 0], sizeof(fe256), hipMemcpyHostToDevice, c->stream));
    }
    REEF_TRY(nifs_copy_in(c, z + c->num_vars + 1, x, c->num_io, loc));
    hipLaunchKernelGGL(k_fe_import<F>, dim3(ceil_div(c->nz, 256)), dim3(256), 0, c->stream, z, (u64)c->nz, (int)is_mont, z);
    REEF_HIP_TRY(hipGetLastError());
    return REEF_OK;
}

template <int C>
static reef_status v_nifs_set_running(void *impl, const reef_fe *W, const reef_fe *E, const reef_fe *u, const reef_fe *X, int loc, bool is_mont) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    if ((c->num_vars && !W) || !u || (c->num_io && !X)) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(call.enter());
    c->running = c->committed = false;
    ++c->gen;
    fe256 *dE = c->E.template as<fe256>();
    REEF_TRY(nifs_load_z(c, c->z1.template as<fe256>(), W, u, X, loc, is_mont));
    if (E) {
        REEF_TRY(nifs_copy_in(c, dE, E, c->num_cons, loc));
        hipLaunchKernelGGL(k_fe_import<NifsCtx<C>::F>, dim3(ceil_div(c->num_cons, 256)), dim3(256), 0, c->stream, dE, (u64)c->num_cons, (int)is_mont, dE);
        REEF_HIP_TRY(hipGetLastError());
    } else {
        REEF_HIP_TRY(hipMemsetAsync(dE, 0, c->num_cons * sizeof(fe256), c->stream));     // zero is zero in every form
    }
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    c->running = true;
    return REEF_OK;
}

// T of the running instance and the fresh one (u2 = 1, E2 = 0), then comm_T = MSM(T, key) on the key ctx's stream: the row pass
// is enqueued there, behind the upload of z2, and the MSM reads T where the pass wrote it.
template <int C>
static reef_status v_nifs_commit_t(void *impl, void *key_impl, const reef_fe *W2, const reef_fe *X2, int loc, bool is_mont, reef_jacobian *comm_t) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    Ctx<C> *key = (Ctx<C> *)key_impl;
    if (!key || !comm_t || (c->num_vars && !W2) || (c->num_io && !X2)) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    if (!c->running) { set_error("reef_nifs_commit_T: no running instance (reef_nifs_set_running first)"); return REEF_ERR_ARG; }
    size_t key_n = 0;
    REEF_TRY(key_matches(key, c->device, "reef_nifs_commit_T", "NIFS", &key_n));
    if (key_n < c->num_cons) { set_error("reef_nifs_commit_T: the key holds %zu points, T has %zu entries", key_n, c->num_cons); return REEF_ERR_ARG; }
    REEF_TRY(call.enter());
    REEF_TRY(nifs_prepare(c));
    c->committed = false;
    ++c->gen;
    REEF_TRY(nifs_load_z(c, c->z2.template as<fe256>(), W2, nullptr, X2, loc, is_mont));
    hipStream_t ks = (hipStream_t)v_ctx_stream<C>(key);
    if (!ks) return REEF_ERR_HIP;
    REEF_HIP_TRY(hipEventRecord(c->ev, c->stream));
    REEF_HIP_TRY(hipStreamWaitEvent(ks, c->ev, 0));
    REEF_TRY((nifs_row_pass<C, NIFS_MODE_T>(c, ks)));
    c->have_t = c->have_z2 = true;
    REEF_TRY(v_msm<C>(key, (const reef_fe *)c->t_row(), c->num_cons, REEF_DEVICE, false, comm_t, REEF_HOST));
    REEF_HIP_TRY(hipStreamSynchronize(ks));
    c->committed = true;
    return REEF_OK;
}

// The key of a step's or the running instance's two commitments: of this device, without a window split, and long enough for both rows.
template <int C> static reef_status nifs_pair_key(NifsCtx<C> *c, Ctx<C> *key, const char *name) {
    size_t key_n = 0;
    REEF_TRY(key_matches(key, c->device, name, "NIFS", &key_n));
    if (key_n < c->row_len()) {
        set_error("%s: the key holds %zu points, the rows have %zu (num_vars) and %zu (num_cons) entries", name, key_n, c->num_vars, c->num_cons);
        return REEF_ERR_ARG;
    }
    u32 split = 1;
    {
        std::lock_guard<std::mutex> kl(key->mu);
        split = key->wsplit_world;
    }
    if (split > 1) { set_error("%s: the key has a window split set (its MSMs are partial sums)", name); return REEF_ERR_ARG; }
    return REEF_OK;
}
// MSM(rows[0 .. n0)) and MSM(rows[row_len .. row_len + n1)) over the key, on its stream, to the host: one wait.  The rows hold canonical
// integers and zero tails.  out0 or out1 may be NULL.  The two rows go through the key's row pipeline as one batch, whatever the key's
// kind: measured (profiles/r16_nifs_step_timing.txt), the batch is not slower than two single rows on a pre-shifted key, on a plain
// key, or on a key with byte tables (where v_msm_rows would serve a single row from the tables: wide_path).  A small key that serves
// single rows from its nibble tables (small_path; at most 1024 points, not measured) takes each row that way, as v_msm_rows would,
// with device results -- as does a lone row.
template <int C>
static reef_status nifs_commit_rows(NifsCtx<C> *c, Ctx<C> *key, hipStream_t ks, const fe256 *rows, size_t n0, size_t n1, reef_jacobian *out0,
                                    reef_jacobian *out1) {
    const size_t len = c->row_len();
    jacobian256 got[2];
    bool single = !out0 || !out1;
    if (!single) {
        std::lock_guard<std::mutex> kl(key->mu);
        single = small_path(key->key->small_tab, key->key->small_n, len, key->wsplit_world);
    }
    if (single) {
        jacobian256 *d = c->pts.template as<jacobian256>();
        if (out0) REEF_TRY(v_msm<C>(key, (const reef_fe *)rows, n0, REEF_DEVICE, false, (reef_jacobian *)d, REEF_DEVICE));
        if (out1) REEF_TRY(v_msm<C>(key, (const reef_fe *)(rows + len), n1, REEF_DEVICE, false, (reef_jacobian *)(d + 1), REEF_DEVICE));
        REEF_HIP_TRY(hipMemcpyAsync(got, d, sizeof got, hipMemcpyDeviceToHost, ks));
        REEF_HIP_TRY(hipStreamSynchronize(ks));
    } else {
        REEF_TRY(v_msm_rows<C>(key, (const reef_fe *)rows, 2, len, REEF_DEVICE, false, 255, nullptr, nullptr, (reef_jacobian *)got, REEF_HOST));
        REEF_HIP_TRY(hipStreamSynchronize(ks));
    }
    if (out0) memcpy(out0, &got[0], sizeof got[0]);
    if (out1) memcpy(out1, &got[1], sizeof got[1]);
    return REEF_OK;
}

// reef_nifs_commit_T and comm_W2 = MSM(W2, key) from one upload: k_nifs_import_step writes z2 and the integers of W2 (row 0 of `step`),
// the row pass writes T into row 1, and the two rows are committed together.  Row 0 is ordered behind the import and row 1 behind the
// row pass by the event on the key ctx's stream, where the row pass runs.
template <int C>
static reef_status v_nifs_commit_step(void *impl, void *key_impl, const reef_fe *W2, const reef_fe *X2, int loc, bool is_mont, reef_jacobian *comm_w2,
                                      reef_jacobian *comm_t) {
    constexpr int F = NifsCtx<C>::F;
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    Ctx<C> *key = (Ctx<C> *)key_impl;
    if (!key || !comm_w2 || !comm_t || (c->num_vars && !W2) || (c->num_io && !X2)) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    if (!c->running) { set_error("reef_nifs_commit_step: no running instance (reef_nifs_set_running first)"); return REEF_ERR_ARG; }
    REEF_TRY(nifs_pair_key(c, key, "reef_nifs_commit_step"));
    REEF_TRY(call.enter());
    REEF_TRY(nifs_prepare(c));
    c->committed = false;
    ++c->gen;
    fe256 *z2 = c->z2.template as<fe256>();
    const fe256 *w = (const fe256 *)W2, *x = (const fe256 *)X2;
    if (loc != REEF_DEVICE) {                // the raw W2 and X2 land in their places in z2 and are converted there; a device W2 is read where it is
        REEF_TRY(nifs_copy_in(c, z2, W2, c->num_vars, loc));
        REEF_TRY(nifs_copy_in(c, z2 + c->num_vars + 1, X2, c->num_io, loc));
        w = z2;
        x = z2 + c->num_vars + 1;
    }
    hipLaunchKernelGGL(k_nifs_import_step<F>, dim3(ceil_div(c->nz, 256)), dim3(256), 0, c->stream, w, x, (u32)c->num_vars, (u32)c->nz, (int)is_mont, z2,
                       c->w2_row());
    REEF_HIP_TRY(hipGetLastError());
    hipStream_t ks = (hipStream_t)v_ctx_stream<C>(key);
    if (!ks) return REEF_ERR_HIP;
    REEF_HIP_TRY(hipEventRecord(c->ev, c->stream));
    REEF_HIP_TRY(hipStreamWaitEvent(ks, c->ev, 0));
    REEF_TRY((nifs_row_pass<C, NIFS_MODE_T>(c, ks)));
    c->have_t = c->have_z2 = true;
    REEF_TRY(nifs_commit_rows(c, key, ks, c->w2_row(), c->num_vars, c->num_cons, comm_w2, comm_t));
    c->committed = true;
    return REEF_OK;
}

// comm_W and comm_E of the running instance as it stands: one kernel exports W and E as integers into rows of their own, the key commits
// them.  Reads only: no state of the ctx changes, and a prove or an opening in flight goes on.
template <int C> static reef_status v_nifs_commit_running(void *impl, void *key_impl, reef_jacobian *comm_w, reef_jacobian *comm_e) {
    constexpr int F = NifsCtx<C>::F;
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    Ctx<C> *key = (Ctx<C> *)key_impl;
    if (!key || (!comm_w && !comm_e)) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    if (!c->running) { set_error("reef_nifs_commit_running: no running instance (reef_nifs_set_running first)"); return REEF_ERR_ARG; }
    REEF_TRY(nifs_pair_key(c, key, "reef_nifs_commit_running"));
    REEF_TRY(call.enter());
    const size_t len = c->row_len();
    if (!c->run.p) {
        REEF_TRY(c->run.ensure(2 * len * sizeof(fe256)));
        REEF_HIP_TRY(hipMemsetAsync(c->run.p, 0, 2 * len * sizeof(fe256), c->stream));
    }
    fe256 *rows = c->run.template as<fe256>();
    hipLaunchKernelGGL(k_nifs_export_running<F>, dim3(ceil_div(len, 256)), dim3(256), 0, c->stream, (const fe256 *)c->z1.p, (const fe256 *)c->E.p,
                       (u32)c->num_vars, (u32)c->num_cons, rows, rows + len);
    REEF_HIP_TRY(hipGetLastError());
    hipStream_t ks = (hipStream_t)v_ctx_stream<C>(key);
    if (!ks) return REEF_ERR_HIP;
    REEF_HIP_TRY(hipEventRecord(c->ev, c->stream));
    REEF_HIP_TRY(hipStreamWaitEvent(ks, c->ev, 0));
    return nifs_commit_rows(c, key, ks, rows, c->num_vars, c->num_cons, comm_w, comm_e);
}

template <int C> static reef_status v_nifs_fold(void *impl, const reef_fe *r, bool is_mont) {
    constexpr int F = NifsCtx<C>::F;
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    if (!r) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    if (!c->committed) { set_error("reef_nifs_fold: no cross term of this step (reef_nifs_commit_T first)"); return REEF_ERR_ARG; }
    fe256 rp;
    memcpy(&rp, r, sizeof rp);
    const fe ri = fe_from_caller<F>(rp, is_mont);                                         // r R'
    const fe256 r_int = fe_to_table<F>(ri);
    const fe256 r_sq = fe_to_table<F>(fe_mul<F>(ri, fe_const<F>(FC<F>::C_R2, 1.0)));    // r R'^2: times an integer T gives r T R'
    REEF_TRY(call.enter());
    ++c->gen;
    hipLaunchKernelGGL(k_nifs_axpy<F>, dim3(ceil_div(c->nz, 256)), dim3(256), 0, c->stream, c->z1.template as<fe256>(), (const fe256 *)c->z2.p, (u32)c->nz, r_int);
    hipLaunchKernelGGL(k_nifs_axpy<F>, dim3(ceil_div(c->num_cons, 256)), dim3(256), 0, c->stream, c->E.template as<fe256>(), (const fe256 *)c->t_row(),
                       (u32)c->num_cons, r_sq);
    REEF_HIP_TRY(hipGetLastError());
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    c->committed = false;                    // the next fold needs the next step's T
    return REEF_OK;
}

// which: 0 W, 1 E, 2 T, 3 u, 4 X
template <int C> static reef_status v_nifs_read(void *impl, int which, size_t count, reef_fe *out, bool to_mont) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    if (count && !out) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    const fe256 *src = nullptr;
    size_t len = 0;
    switch (which) {
    case 0: src = c->z1.template as<fe256>(); len = c->num_vars; break;
    case 1: src = c->E.template as<fe256>(); len = c->num_cons; break;
    case 2: src = c->t_row(); len = c->num_cons; break;
    case 3: src = c->z1.template as<fe256>() + c->num_vars; len = 1; break;
    case 4: src = c->z1.template as<fe256>() + c->num_vars + 1; len = c->num_io; break;
    default: set_error("reef_nifs_read: which must be 0 (W), 1 (E), 2 (T), 3 (u) or 4 (X)"); return REEF_ERR_ARG;
    }
    if (count > len) { set_error("reef_nifs_read: %zu entries asked, the vector has %zu", count, len); return REEF_ERR_ARG; }
    if (which == 2 ? !c->have_t : !c->running) { set_error("reef_nifs_read: nothing to read yet"); return REEF_ERR_ARG; }
    if (!count) return REEF_OK;
    REEF_TRY(call.enter());
    REEF_TRY(c->stage.ensure(count * sizeof(fe256)));
    hipLaunchKernelGGL(k_fe_export<NifsCtx<C>::F>, dim3(ceil_div(count, 256)), dim3(256), 0, c->stream, src, (u64)count, (int)(which == 2), (int)to_mont,
                       c->stage.template as<fe256>());
    REEF_HIP_TRY(hipGetLastError());
    REEF_HIP_TRY(hipMemcpyAsync(out, c->stage.p, count * sizeof(fe256), hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    return REEF_OK;
}

template <int C> static reef_status v_nifs_check(void *impl, uint64_t *violations, uint64_t *first_bad_row) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    if (!c->running) { set_error("reef_nifs_check_relaxed: no running instance (reef_nifs_set_running first)"); return REEF_ERR_ARG; }
    REEF_TRY(call.enter());
    REEF_TRY(nifs_prepare(c));
    const u32 init[2] = {0u, 0xffffffffu};
    REEF_HIP_TRY(hipMemcpyAsync(c->counters.p, init, sizeof init, hipMemcpyHostToDevice, c->stream));
    REEF_TRY((nifs_row_pass<C, NIFS_MODE_CHECK>(c, c->stream)));
    u32 got[2] = {0, 0};
    REEF_HIP_TRY(hipMemcpyAsync(got, c->counters.p, sizeof got, hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    if (violations) *violations = got[0];
    if (first_bad_row) *first_bad_row = got[0] ? (uint64_t)got[1] : UINT64_MAX;
    return REEF_OK;
}

// AZ2 o BZ2 == CZ2 on the fresh instance (W2, 1, X2) of the last commit_T / commit_step: the row pass over z2.  Reads only.
template <int C> static reef_status v_nifs_check_fresh(void *impl, uint64_t *violations, uint64_t *first_bad_row) {
    NifsCtx<C> *c = (NifsCtx<C> *)impl;
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    if (!c->have_z2) { set_error("reef_nifs_check_fresh: no fresh instance (reef_nifs_commit_T or reef_nifs_commit_step first)"); return REEF_ERR_ARG; }
    REEF_TRY(call.enter());
    REEF_TRY(nifs_prepare(c));
    const u32 init[2] = {0u, 0xffffffffu};
    REEF_HIP_TRY(hipMemcpyAsync(c->counters.p, init, sizeof init, hipMemcpyHostToDevice, c->stream));
    NifsArgs a = nifs_args(c);
    a.z1 = a.z2;
    REEF_TRY((nifs_line_pass<C, NIFS_MODE_FRESH>(a, c->rows, c->stream)));
    u32 got[2] = {0, 0};
    REEF_HIP_TRY(hipMemcpyAsync(got, c->counters.p, sizeof got, hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    if (violations) *violations = got[0];
    if (first_bad_row) *first_bad_row = got[0] ? (uint64_t)got[1] : UINT64_MAX;
    return REEF_OK;
}

template <int C> NifsVTable make_nifs_vtable() {
    return NifsVTable{v_nifs_create<C>, v_nifs_destroy<C>, v_nifs_set_matrix<C>, v_nifs_set_running<C>, v_nifs_commit_t<C>, v_nifs_fold<C>,
                      v_nifs_read<C>, v_nifs_check<C>, v_nifs_commit_step<C>, v_nifs_commit_running<C>, v_nifs_check_fresh<C>};
}

}  // namespace reef
