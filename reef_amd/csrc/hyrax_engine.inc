// Host side of the Hyrax consistency argument (hyrax_kernels.inc; include/reef_msm.h 3i) on a resident document; included after
// proof_order.h (the HY_* phases and the call order) and ipa_engine.inc.  create -> eval_begin -> [eval_comm] -> ipa_begin ->
// ipa_round x (right - 1) -> finish, right = num_vars - left_vars; eval_begin may come at any time and starts the argument over.  The
// rounds are IpaRun's, driven from this ctx's stream.  commit (the row commitments of the resident document, HyraxPC::commit) is in no
// call order; eval_comm_own stands where eval_comm does.
namespace reef {

template <int C> struct HyraxCtx : DeviceCtx {   // ev: orders the key ctx's stream after this one (IpaRun::ipa_cross)
    static constexpr int F = 1 - C;      // scalar field of curve C
    DevBuf z, rb;                        // Z (n entries of eb bytes; 32-byte entries as canonical integers); the row blinds (integers)
    DevBuf eqs, part, dot, pts, lint, stage;   // eq(point[..left]) || eq(point[left..]) || 1 (fe_limbs); bound-row partial sums;
                                               // limb sums then eval, lz_blind; eq factors; L as integers (eval_comm); read staging
    size_t n = 0;
    int eb = 0;
    u32 left = 0, right = 0, rows = 0, cols = 0, chunks = 0, rpc = 0, bchunks = 0, brpc = 0;
    bool has_blinds = false;
    std::vector<fe> pt;                  // the point of the argument (internal form), from eval_begin
    IpaRun<C> ip;                        // a = LZ, b = eq(point[left..]) and the rounds
    Ctx<C> *comms = nullptr;             // a plain key over the row commitments, made by the first eval_comm
    std::vector<reef_affine> comms_host; // the host row commitments that key holds (empty: device bases, compared never)
    std::vector<uint8_t> comms_bytes;    // or the host rows it was decoded from, 32 bytes each (eval_comm_compressed); at most one of the two is set
    DevBuf cenc, cdec, cstat;            // eval_comm_compressed: the encodings of host rows, the decoded rows the key is built from, the decode's two counters
                                         // commit: the encoded rows, the affine rows the key is built from, the OR of the symbols
    DevBuf cjac;                         // commit: the row sums as they leave the row route (Jacobian)
    u32 sym_bits = 0;                    // elem_bytes 1 / 2 / 4: the bit length of the largest resident symbol, at least 1 (0: not measured yet)
    bool own = false, committed = false; // comms holds the rows commit made of this document (eval_comm_own); commit has succeeded at least once
    int phase = HY_NONE;
    u32 rounds = 0;
    size_t n_small = 0;                  // reef_hyrax_set_small_key: the arguments begun from now on move to a folded key at this length (0: never)
};

// Every call enqueues on a pool stream and waits for it before it returns (common.h: OnExit::WAIT_AND_IDLE)
template <int C> static void hyrax_free(HyraxCtx<C> *c) {
    if (!c) return;
    retire_device_ctx(c);
    for (DevBuf *b : {&c->z, &c->rb, &c->eqs, &c->part, &c->dot, &c->pts, &c->lint, &c->stage, &c->cenc, &c->cdec, &c->cstat, &c->cjac}) b->release();
    c->ip.release();
    if (c->comms) v_ctx_destroy<C>(c->comms);
    delete c;
}

// The call `name` may come now (proof_order.h: REEF_ERR_ARG naming the next call otherwise)
template <int C> static reef_status hy_expect(HyraxCtx<C> *c, const char *name) {
    const OrderVerdict v = hy_check(name, c->phase, c->rounds, c->right);
    if (!v.ok) { set_error("%s", v.text); return REEF_ERR_ARG; }
    return REEF_OK;
}
template <int C>
static reef_status v_hyrax_create(void **impl, const void *z, size_t n, int elem_bytes, int z_loc, bool is_mont, size_t num_vars, size_t left_vars,
                                  const reef_fe *row_blinds, int device) {
    constexpr int F = HyraxCtx<C>::F;
    if (!impl || (n && !z)) { set_error("null argument"); return REEF_ERR_ARG; }
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 32) { set_error("reef_hyrax_create: elem_bytes must be 1, 2, 4 or 32"); return REEF_ERR_ARG; }
    if (num_vars > 28 || left_vars < 1 || left_vars >= num_vars) {
        set_error("reef_hyrax_create: need num_vars <= 28 and 1 <= left_vars < num_vars (num_vars %zu, left_vars %zu)", num_vars, left_vars);
        return REEF_ERR_ARG;
    }
    if (n > ((size_t)1 << num_vars)) { set_error("reef_hyrax_create: n = %zu exceeds 2^num_vars", n); return REEF_ERR_ARG; }
    const u32 rows = 1u << left_vars, cols = 1u << (num_vars - left_vars);
    u32 chunks = 0, rpc = 0, bchunks = 0, brpc = 0;
    REEF_TRY(mle_plan(rows, cols, elem_bytes, &chunks, &rpc));
    if (row_blinds) {   // the blinds as a one-column table: rows of up to 1024 per chunk once there are more than 4096
        brpc = std::min<u32>(1024, ceil_div(rows, 4096u));
        bchunks = ceil_div(rows, brpc);
        if (bchunks > 65535) { set_error("reef_hyrax_create: row blinds need left_vars <= 25 (%u row chunks)", bchunks); return REEF_ERR_ARG; }
    }
    std::vector<fe256> blinds(row_blinds ? rows : 0);
    if (row_blinds) REEF_TRY(fe_import_all<F>(row_blinds, rows, is_mont, "reef_hyrax_create", "row_blinds", blinds.data()));
    return create_device_ctx<HyraxCtx<C>>(impl, device, "reef_hyrax_create", true, hyrax_free<C>, [&](HyraxCtx<C> *c) -> reef_status {
        c->n = n;
        c->eb = elem_bytes;
        c->left = (u32)left_vars;
        c->right = (u32)(num_vars - left_vars);
        c->rows = rows;
        c->cols = cols;
        c->chunks = chunks;
        c->rpc = rpc;
        c->bchunks = bchunks;
        c->brpc = brpc;
        c->has_blinds = row_blinds != nullptr;
        // z holds whole rows, in whole 16-byte words: the tail past the document is zeroed, so that commit's row route and width measure read no
        // further than the allocation and see the padding the matrix has there
        const size_t bytes = n * (size_t)elem_bytes;
        const size_t zbytes = std::max<size_t>(round_up((u64)ceil_div(n, cols) * cols * (u64)elem_bytes, 16), 16);
        REEF_TRY(c->z.ensure(zbytes));
        if (c->has_blinds) REEF_TRY(c->rb.ensure(rows * sizeof(fe256)));
        REEF_TRY(c->eqs.ensure(((size_t)rows + cols + 1) * sizeof(fe_limbs)));
        REEF_TRY(c->part.ensure(std::max<size_t>((size_t)chunks * cols, bchunks) * sizeof(fe256)));   // bchunks: 0 without blinds
        REEF_TRY(c->dot.ensure(20 * sizeof(u64) + 2 * sizeof(fe256)));
        REEF_TRY(c->pts.ensure(2 * std::max(c->left, c->right) * sizeof(fe256)));
        REEF_TRY(c->lint.ensure(rows * sizeof(fe256)));
        REEF_TRY(ipa_alloc(&c->ip, cols, 0));
        DeviceScope scope(c, OnExit::WAIT_AND_IDLE);
        REEF_TRY(scope.enter());
        if (hipMemsetAsync((char *)c->z.p + bytes, 0, zbytes - bytes, c->stream) != hipSuccess) {
            set_error("reef_hyrax_create: clearing the tail of z failed");
            return REEF_ERR_HIP;
        }
        if (bytes && hipMemcpyAsync(c->z.p, z, bytes, z_loc == REEF_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream) != hipSuccess) {
            set_error("reef_hyrax_create: the copy of z failed");
            return REEF_ERR_HIP;
        }
        if (elem_bytes == 32 && is_mont && n) {    // to canonical integers: every sum then comes out as one
            fe256 *zz = c->z.template as<fe256>();
            hipLaunchKernelGGL(k_fe_import<F>, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, (const fe256 *)zz, (u64)n, 1, zz);
            hipLaunchKernelGGL(k_fe_export<F>, dim3(ceil_div(n, 256)), dim3(256), 0, c->stream, (const fe256 *)zz, (u64)n, 0, 0, zz);
            if (hipGetLastError() != hipSuccess) { set_error("reef_hyrax_create: launch failed"); return REEF_ERR_HIP; }
        }
        if (c->has_blinds && hipMemcpyAsync(c->rb.p, blinds.data(), rows * sizeof(fe256), hipMemcpyHostToDevice, c->stream) != hipSuccess) {
            set_error("reef_hyrax_create: the copy of the row blinds failed");
            return REEF_ERR_HIP;
        }
        if (hipStreamSynchronize(c->stream) != hipSuccess) { set_error("reef_hyrax_create: %s", hipGetErrorString(hipGetLastError())); return REEF_ERR_HIP; }
        return REEF_OK;
    });
}
template <int C> static void v_hyrax_destroy(void *impl) { hyrax_free((HyraxCtx<C> *)impl); }

template <int C>
static reef_status v_hyrax_eval_begin(void *impl, void *key_impl, const reef_fe *point, bool is_mont, reef_fe *eval, reef_fe *lz_blind) {
    constexpr int F = HyraxCtx<C>::F;
    HyraxCtx<C> *c = (HyraxCtx<C> *)impl;
    Ctx<C> *key = (Ctx<C> *)key_impl;
    if (!key || !point) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    const u32 nv = c->left + c->right;
    std::vector<fe> pt(nv);
    REEF_TRY(fe_import_all<F>(point, nv, is_mont, "reef_hyrax_eval_begin", "point", pt.data()));
    size_t key_n = 0;
    REEF_TRY(key_matches(key, c->device, "reef_hyrax_eval_begin", "Hyrax", &key_n));
    if (key_n != c->cols) {
        set_error("reef_hyrax_eval_begin: the key holds %zu points, the argument needs exactly 2^(num_vars - left_vars) = %u", key_n, c->cols);
        return REEF_ERR_ARG;
    }
    REEF_TRY(call.enter(&c->phase));
    c->pt = pt;
    REEF_TRY(ipa_alloc(&c->ip, c->cols, c->n_small));
    MlePoint mp;
    memset(&mp, 0, sizeof mp);
    memcpy(mp.r, point, nv * sizeof(fe256));
    fe_limbs *Leq = c->eqs.template as<fe_limbs>(), *Req = Leq + c->rows, *one = Req + c->cols;
    unsigned long long *dot = c->dot.template as<unsigned long long>();
    fe256 *res = reinterpret_cast<fe256 *>(dot + 20);          // eval, lz_blind: canonical integers
    hipStream_t st = c->stream;
    hipLaunchKernelGGL(k_mle_eq<F>, dim3(ceil_div(c->rows, 256)), dim3(256), 0, st, mp, 0u, c->left, (int)is_mont, Leq);
    hipLaunchKernelGGL(k_mle_eq<F>, dim3(ceil_div(c->cols, 256)), dim3(256), 0, st, mp, c->left, c->right, (int)is_mont, Req);
    hipLaunchKernelGGL(k_mle_eq<F>, dim3(1), dim3(256), 0, st, mp, 0u, 0u, (int)is_mont, one);
    REEF_HIP_TRY(hipMemsetAsync(dot, 0, 20 * sizeof(u64) + 2 * sizeof(fe256), st));
    fe256 *part = c->part.template as<fe256>();
    if (c->has_blinds) {   // the blinds as a one-column table: sum_i L_i blind_i
        mle_launch_bound_any<C>(st, 32, c->rb.p, c->rows, c->rows, 1, c->brpc, c->bchunks, Leq, part);
        hipLaunchKernelGGL((k_mle_finish<F, false>), dim3(1), dim3(256), 0, st, (const fe256 *)part, c->bchunks, 1u, (const fe_limbs *)one, 0,
                           (fe256 *)nullptr, dot + 10);
        hipLaunchKernelGGL((k_mle_eval_final<F, false>), dim3(1), dim3(64), 0, st, dot + 10, 0, res + 1);
    }
    mle_launch_bound_any<C>(st, c->eb, c->z.p, c->n, c->rows, c->cols, c->rpc, c->chunks, Leq, part);
    fe256 *a = c->ip.a.template as<fe256>();
    if (c->eb == 32) {
        hipLaunchKernelGGL((k_mle_finish<F, false>), dim3(ceil_div(c->cols, 256)), dim3(256), 0, st, (const fe256 *)part, c->chunks, c->cols,
                           (const fe_limbs *)Req, 0, a, dot);
        hipLaunchKernelGGL((k_mle_eval_final<F, false>), dim3(1), dim3(64), 0, st, dot, 0, res);
    } else {
        hipLaunchKernelGGL((k_mle_finish<F, true>), dim3(ceil_div(c->cols, 256)), dim3(256), 0, st, (const fe256 *)part, c->chunks, c->cols,
                           (const fe_limbs *)Req, 0, a, dot);
        hipLaunchKernelGGL((k_mle_eval_final<F, true>), dim3(1), dim3(64), 0, st, dot, 0, res);
    }
    REEF_HIP_TRY(hipGetLastError());
    REEF_TRY(fe_eq_table<F>(st, c->pts, c->pt.data() + c->left, c->right, c->ip.b.template as<fe256>()));   // b = eq(point[left..]); waits
    fe256 h[2];
    REEF_HIP_TRY(hipMemcpyAsync(h, res, sizeof h, hipMemcpyDeviceToHost, st));
    REEF_HIP_TRY(hipStreamSynchronize(st));
    reef_fe *outs[2] = {eval, lz_blind};
    for (int k = 0; k < 2; ++k) {
        if (!outs[k]) continue;
        const fe256 o = fe_to_caller<F>(fe_from_integer<F>(h[k]), is_mont);
        memcpy(outs[k], &o, sizeof o);
    }
    c->ip.key = key;
    c->rounds = 0;
    return call.done(HY_EVAL);
}

// the weights of comm_LZ where the MSM reads them: lint = eq(point[..left]) as canonical integers.  Inside the ctx's scope; waits.
template <int C> static reef_status hy_row_weights(HyraxCtx<C> *c) {
    constexpr int F = HyraxCtx<C>::F;
    fe256 *l = c->lint.template as<fe256>();
    REEF_TRY(fe_eq_table<F>(c->stream, c->pts, c->pt.data(), c->left, l));                 // L = eq(point[..left]), then canonical integers in place
    hipLaunchKernelGGL(k_fe_export<F>, dim3(ceil_div(c->rows, 256)), dim3(256), 0, c->stream, (const fe256 *)l, (u64)c->rows, 0, 0, l);
    REEF_HIP_TRY(hipGetLastError());
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    return REEF_OK;
}
// the plain key over the row commitments, from `rows` affine points in loc memory: made by the first call, re-keyed by the others
template <int C> static reef_status hy_set_comms(HyraxCtx<C> *c, const reef_affine *row_comms, int loc) {
    if (c->comms) return v_ctx_rekey<C>(c->comms, row_comms, c->rows, loc);
    reef_msm_opts o;
    memset(&o, 0, sizeof o);
    o.byte_tables = 2;                                           // a plain key: the bases change with every document
    o.device = c->device;
    void *k = nullptr;
    REEF_TRY(v_ctx_create<C>(&k, row_comms, c->rows, loc, &o));
    c->comms = (Ctx<C> *)k;
    return REEF_OK;
}

template <int C> static reef_status v_hyrax_eval_comm(void *impl, const reef_affine *row_comms, int loc, reef_jacobian *comm_lz) {
    HyraxCtx<C> *c = (HyraxCtx<C> *)impl;
    if (!row_comms || !comm_lz) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(hy_expect(c, "reef_hyrax_eval_comm"));
    REEF_TRY(call.enter());
    REEF_TRY(hy_row_weights(c));
    call.leave();                                             // the rest is the key ctx's own work, on its stream
    const bool same = loc != REEF_DEVICE && c->comms && c->comms_host.size() == c->rows &&
                      memcmp(c->comms_host.data(), row_comms, c->rows * sizeof(reef_affine)) == 0;
    if (!same) c->comms_bytes.clear();
    if (same) {
        // the key already holds these row commitments: no upload
    } else {
        REEF_TRY(hy_set_comms(c, row_comms, loc));
    }
    if (!same) {
        c->own = false;                                       // the caller's rows replace those of reef_hyrax_commit
        if (loc != REEF_DEVICE) c->comms_host.assign(row_comms, row_comms + c->rows);
        else c->comms_host.clear();
    }
    return v_msm<C>(c->comms, (const reef_fe *)c->lint.p, c->rows, REEF_DEVICE, false, comm_lz, REEF_HOST);
}

// reef_hyrax_eval_comm from the rows as Reef holds them: the 32-byte encodings are decoded on this ctx's device (k_decompress) into cdec and
// the key is made or re-keyed from there -- no affine point visits the host.  An invalid row changes nothing: the key is touched only
// after the whole batch has decoded.
template <int C> static reef_status v_hyrax_eval_comm_compressed(void *impl, const uint8_t *row_comms32, int loc, reef_jacobian *comm_lz) {
    HyraxCtx<C> *c = (HyraxCtx<C> *)impl;
    if (!row_comms32 || !comm_lz) { set_error("null argument"); return REEF_ERR_ARG; }
    if (loc == REEF_DEVICE && ((uintptr_t)row_comms32 & 15)) { set_error("reef_hyrax_eval_comm_compressed: device rows must be 16-byte aligned"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(hy_expect(c, "reef_hyrax_eval_comm_compressed"));
    const size_t bytes = (size_t)c->rows * 32;
    const bool same = loc != REEF_DEVICE && c->comms && c->comms_bytes.size() == bytes && memcmp(c->comms_bytes.data(), row_comms32, bytes) == 0;
    REEF_TRY(call.enter());
    REEF_TRY(hy_row_weights(c));
    if (!same) {
        REEF_TRY(c->cdec.ensure(c->rows * sizeof(affine256)));
        REEF_TRY(c->cstat.ensure(2 * sizeof(u64)));
        const fe256 *enc = (const fe256 *)row_comms32;
        if (loc != REEF_DEVICE) {
            REEF_TRY(c->cenc.ensure(bytes));
            REEF_HIP_TRY(hipMemcpyAsync(c->cenc.p, row_comms32, bytes, hipMemcpyHostToDevice, c->stream));
            enc = c->cenc.template as<fe256>();
        }
        decompress_launch<C>(c->stream, enc, c->rows, c->cdec.template as<affine256>(), c->cstat.template as<unsigned long long>());
        REEF_HIP_TRY(hipGetLastError());
        u64 stats[2] = {0, 0};
        REEF_HIP_TRY(hipMemcpyAsync(stats, c->cstat.p, sizeof stats, hipMemcpyDeviceToHost, c->stream));
        REEF_HIP_TRY(hipStreamSynchronize(c->stream));
        if (stats[0]) {
            set_error("reef_hyrax_eval_comm_compressed: row %llu is not the encoding of a point (%llu such rows); the row commitments of the previous call stay",
                      (unsigned long long)stats[1], (unsigned long long)stats[0]);
            return REEF_ERR_ARG;
        }
    }
    call.leave();                                             // the rest is the key ctx's own work, on its stream
    if (!same) {
        c->comms_host.clear();
        c->comms_bytes.clear();
        c->own = false;                                       // the caller's rows replace those of reef_hyrax_commit
        REEF_TRY(hy_set_comms(c, (const reef_affine *)c->cdec.p, REEF_DEVICE));
        if (loc != REEF_DEVICE) c->comms_bytes.assign(row_comms32, row_comms32 + bytes);
    }
    return v_msm<C>(c->comms, (const reef_fe *)c->lint.p, c->rows, REEF_DEVICE, false, comm_lz, REEF_HOST);
}

// HyraxPC::commit (commitment.rs:187) of the resident document: C_i = <Z_i, key> (+ blind_i h) for every row of the matrix, through K2's row
// routes on the key ctx's stream with z and rb where create left them.  The rows that hold document entries go through the route of their
// element width (the symbol width is the measured one); the rows wholly beyond n start as the identity; one k_add_blind_tab launch adds
// blind_i h to all of them, one k_normalize launch writes the affine rows (cdec) and the encodings.  The key ctx's stream is waited for
// before the comms key is touched, so that an error leaves the ctx with the row commitments it had.
template <int C>
static reef_status hy_commit_finish(HyraxCtx<C> *c, Ctx<C> *key, size_t used, const reef_affine *h, uint8_t *comms32, reef_affine *comms_affine, int out_loc) {
    std::lock_guard<std::mutex> lk(key->mu);
    CtxScope<C> scope(key);
    REEF_TRY(scope.enter());
    hipStream_t st = key->stream;
    jacobian256 *jac = c->cjac.template as<jacobian256>();
    if (used < c->rows) REEF_HIP_TRY(hipMemsetAsync(jac + used, 0, (c->rows - used) * sizeof(jacobian256), st));
    if (h) {
        struct HostH {                                        // launch_blind takes h's nibble table from key->h_host (rebuilt only when h changes)
            Ctx<C> *k;
            ~HostH() { k->h_host = nullptr; }
        } host_h{key};
        key->h_host = h;
        REEF_TRY(launch_blind<C>(key, jac, c->rb.template as<fe256>(), nullptr, false, c->rows));
    }
    affine256 *aff = c->cdec.template as<affine256>();
    fe256 *enc = !comms32 ? nullptr : out_loc == REEF_DEVICE ? (fe256 *)comms32 : c->cenc.template as<fe256>();
    hipLaunchKernelGGL(k_normalize<C>, dim3(ceil_div(ceil_div(c->rows, NORM_PER), 256)), dim3(256), 0, st, (const jacobian256 *)jac, c->rows, aff, enc);
    REEF_HIP_TRY(hipGetLastError());
    const hipMemcpyKind kind = out_loc == REEF_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (comms_affine) REEF_HIP_TRY(hipMemcpyAsync(comms_affine, aff, c->rows * sizeof(affine256), kind, st));
    if (comms32 && out_loc != REEF_DEVICE) REEF_HIP_TRY(hipMemcpyAsync(comms32, enc, (size_t)c->rows * 32, kind, st));
    REEF_HIP_TRY(hipStreamSynchronize(st));
    return REEF_OK;
}
template <int C>
static reef_status v_hyrax_commit(void *impl, void *key_impl, const reef_affine *h, uint8_t *comms32, reef_affine *comms_affine, int out_loc) {
    HyraxCtx<C> *c = (HyraxCtx<C> *)impl;
    Ctx<C> *key = (Ctx<C> *)key_impl;
    if (!key) { set_error("null argument"); return REEF_ERR_ARG; }
    if (out_loc == REEF_DEVICE && (((uintptr_t)comms32 | (uintptr_t)comms_affine) & 15)) { set_error("reef_hyrax_commit: device outputs must be 16-byte aligned"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    if (c->has_blinds && !h) { set_error("reef_hyrax_commit: the ctx holds row blinds, the commitment needs their point h"); return REEF_ERR_ARG; }
    if (!c->has_blinds && h) { set_error("reef_hyrax_commit: h given, but reef_hyrax_create took no row blinds"); return REEF_ERR_ARG; }
    size_t key_n = 0;
    REEF_TRY(key_matches(key, c->device, "reef_hyrax_commit", "Hyrax", &key_n));
    if (key_n != c->cols) {
        set_error("reef_hyrax_commit: the key holds %zu points, a row has exactly 2^(num_vars - left_vars) = %u", key_n, c->cols);
        return REEF_ERR_ARG;
    }
    u32 split = 1;
    {
        std::lock_guard<std::mutex> kl(key->mu);
        split = key->wsplit_world;
    }
    if (split > 1) { set_error("reef_hyrax_commit: the key has a window split set (its MSMs are partial sums)"); return REEF_ERR_ARG; }
    REEF_TRY(call.enter());                                   // the phase, a, b and the rounds of an argument in flight stay as they are
    if (c->eb != 32 && !c->sym_bits) {                        // the width of the document's symbols, once per ctx
        REEF_TRY(c->cstat.ensure(2 * sizeof(u64)));
        u32 *d_or = c->cstat.template as<u32>(), w = 0;
        const u64 n16 = round_up((u64)ceil_div(c->n, c->cols) * c->cols * (u64)c->eb, 16) / 16;   // the whole rows create zero-padded
        REEF_HIP_TRY(hipMemsetAsync(d_or, 0, sizeof(u32), c->stream));
        if (n16) hipLaunchKernelGGL(k_hy_sym_or, dim3((u32)std::min<u64>(1024, ceil_div(n16, (u64)256))), dim3(256), 0, c->stream, (const uint4 *)c->z.p, n16, d_or);
        REEF_HIP_TRY(hipGetLastError());
        REEF_HIP_TRY(hipMemcpyAsync(&w, d_or, sizeof(u32), hipMemcpyDeviceToHost, c->stream));
        REEF_HIP_TRY(hipStreamSynchronize(c->stream));
        if (c->eb <= 2) w |= w >> 16;                         // the OR of the words' halves, then of their bytes: the OR of the symbols
        if (c->eb == 1) w |= w >> 8;
        w &= c->eb == 1 ? 0xffu : c->eb == 2 ? 0xffffu : ~0u;
        c->sym_bits = w ? 32u - (u32)__builtin_clz(w) : 1u;
    }
    REEF_TRY(c->cjac.ensure(c->rows * sizeof(jacobian256)));
    REEF_TRY(c->cdec.ensure(c->rows * sizeof(affine256)));
    if (comms32 && out_loc != REEF_DEVICE) REEF_TRY(c->cenc.ensure((size_t)c->rows * 32));
    call.leave();                                             // the rest is the key ctx's work, on its stream; z and rb have been at rest since create
    const size_t used = ceil_div(c->n, (size_t)c->cols);      // the rows that hold document entries (the last one zero-padded)
    reef_jacobian *jac = c->cjac.template as<reef_jacobian>();
    if (used && c->eb == 32)
        REEF_TRY(v_msm_rows<C>(key, (const reef_fe *)c->z.p, used, c->cols, REEF_DEVICE, false, 0, nullptr, nullptr, jac, REEF_DEVICE));
    else if (used && c->eb == 1)
        REEF_TRY(v_msm_rows_symbols<C>(key, (const uint8_t *)c->z.p, used, c->cols, REEF_DEVICE, c->sym_bits, nullptr, nullptr, false, jac, REEF_DEVICE));
    else if (used)
        REEF_TRY(v_msm_rows_symbols_wide<C>(key, c->z.p, (u32)c->eb, used, c->cols, REEF_DEVICE, c->sym_bits, nullptr, nullptr, false, jac, REEF_DEVICE));
    REEF_TRY(hy_commit_finish(c, key, used, h, comms32, comms_affine, out_loc));
    REEF_TRY(hy_set_comms(c, (const reef_affine *)c->cdec.p, REEF_DEVICE));   // device to device: no affine point visits the host unless asked for
    c->comms_host.clear();
    c->comms_bytes.clear();
    c->own = c->committed = true;
    return REEF_OK;
}

// reef_hyrax_eval_comm over the rows reef_hyrax_commit left in the comms key: no argument, no upload
template <int C> static reef_status v_hyrax_eval_comm_own(void *impl, reef_jacobian *comm_lz) {
    HyraxCtx<C> *c = (HyraxCtx<C> *)impl;
    if (!comm_lz) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(hy_expect(c, "reef_hyrax_eval_comm_own"));
    if (!c->own || !c->comms) {
        set_error(c->committed ? "reef_hyrax_eval_comm_own: a later reef_hyrax_eval_comm[_compressed] replaced the ctx's own row commitments; reef_hyrax_commit makes them again"
                               : "reef_hyrax_eval_comm_own: the ctx has no row commitments of its own yet; reef_hyrax_commit makes them");
        return REEF_ERR_ARG;
    }
    REEF_TRY(call.enter());
    REEF_TRY(hy_row_weights(c));
    call.leave();                                             // the rest is the key ctx's own work, on its stream
    return v_msm<C>(c->comms, (const reef_fe *)c->lint.p, c->rows, REEF_DEVICE, false, comm_lz, REEF_HOST);
}

template <int C>
static reef_status v_hyrax_ipa_begin(void *impl, const reef_affine *q, const reef_affine *h, const reef_fe *blinds, bool is_mont, reef_jacobian *L,
                                     reef_jacobian *R) {
    constexpr int F = HyraxCtx<C>::F;
    HyraxCtx<C> *c = (HyraxCtx<C> *)impl;
    if (!q || !L || !R) { set_error("null argument"); return REEF_ERR_ARG; }
    const bool with_h = h && blinds;
    fe256 b2[2] = {};
    if (with_h) REEF_TRY(fe_import_all<F>(blinds, 2, is_mont, "reef_hyrax_ipa_begin", "blinds", b2));
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(hy_expect(c, "reef_hyrax_ipa_begin"));
    REEF_TRY(call.enter(&c->phase));
    IpaRun<C> *ip = &c->ip;
    ip->q = *q;
    ip->with_h = false;
    if (with_h) {
        REEF_TRY(ipa_set_h(ip, h));
        REEF_TRY(ipa_set_blinds(ip, c->stream, b2));
    }
    const u32 half = c->cols / 2, grid = sp_grid(half);
    hipLaunchKernelGGL(k_hy_sums<F>, dim3(grid), dim3(SP_THREADS), 0, c->stream, (const fe256 *)ip->a.p, (const fe256 *)ip->b.p, half,
                       ip->partial.template as<unsigned long long>());
    ipa_sums(ip, c->stream, grid, 2, 1);                      // round 0's c_L, c_R where ipa_cross reads them
    REEF_HIP_TRY(hipGetLastError());
    REEF_TRY(ipa_cross(ip, c->stream, c->ev, L, R));
    c->rounds = 0;
    return call.done(HY_IPA);
}

template <int C>
static reef_status v_hyrax_ipa_round(void *impl, const reef_fe *r, const reef_fe *blinds, bool is_mont, reef_jacobian *L, reef_jacobian *R) {
    constexpr int F = HyraxCtx<C>::F;
    HyraxCtx<C> *c = (HyraxCtx<C> *)impl;
    fe ri;
    REEF_TRY(fe_challenge<F>(r, is_mont, "reef_hyrax_ipa_round", ri, true));
    if (!L || !R) { set_error("null argument"); return REEF_ERR_ARG; }
    fe256 b2[2] = {};
    if (blinds) REEF_TRY(fe_import_all<F>(blinds, 2, is_mont, "reef_hyrax_ipa_round", "blinds", b2));
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(hy_expect(c, "reef_hyrax_ipa_round"));
    if (blinds && !c->ip.with_h) { set_error("reef_hyrax_ipa_round: blinds given, but reef_hyrax_ipa_begin took no h term"); return REEF_ERR_ARG; }
    REEF_TRY(call.enter(&c->phase));
    if (c->ip.with_h) REEF_TRY(ipa_set_blinds(&c->ip, c->stream, b2));   // NULL: zero blinds this round
    REEF_TRY(ipa_round(&c->ip, c->stream, c->ev, ri, L, R));
    ++c->rounds;
    return call.done(HY_IPA);
}

template <int C> static reef_status v_hyrax_finish(void *impl, const reef_fe *r_last, bool is_mont, reef_fe *a_hat, reef_fe *b_hat) {
    HyraxCtx<C> *c = (HyraxCtx<C> *)impl;
    fe ri;
    REEF_TRY(fe_challenge<HyraxCtx<C>::F>(r_last, is_mont, "reef_hyrax_finish", ri, true));
    if (!a_hat) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(hy_expect(c, "reef_hyrax_finish"));
    REEF_TRY(call.enter(&c->phase));
    REEF_TRY(ipa_last(&c->ip, c->stream, ri, is_mont, a_hat, b_hat));
    return call.done(HY_DONE);
}

// which: 0 a, 1 b, the first `count` of their current length
template <int C> static reef_status v_hyrax_read(void *impl, int which, size_t count, reef_fe *out, bool to_mont) {
    HyraxCtx<C> *c = (HyraxCtx<C> *)impl;
    if (count && !out) { set_error("null argument"); return REEF_ERR_ARG; }
    if (which != 0 && which != 1) { set_error("reef_hyrax_read: which must be 0 (a) or 1 (b)"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(hy_expect(c, "reef_hyrax_read"));
    if (count > c->ip.len) { set_error("reef_hyrax_read: %zu entries asked, the vector has %zu", count, c->ip.len); return REEF_ERR_ARG; }
    if (!count) return REEF_OK;
    REEF_TRY(call.enter());
    return ipa_read(&c->ip, c->stream, c->stage, which, count, out, to_mont);
}

// n_small (0 or a power of two: api.cpp checks) holds for the arguments begun (eval_begin) after the call; no device work
template <int C> static reef_status v_hyrax_set_small_key(void *impl, size_t n_small) {
    HyraxCtx<C> *c = (HyraxCtx<C> *)impl;
    std::lock_guard<std::mutex> lk(c->mu);
    c->n_small = n_small;
    return REEF_OK;
}

template <int C> HyraxVTable make_hyrax_vtable() {
    return HyraxVTable{v_hyrax_create<C>, v_hyrax_destroy<C>, v_hyrax_eval_begin<C>, v_hyrax_eval_comm<C>, v_hyrax_ipa_begin<C>,
                       v_hyrax_ipa_round<C>, v_hyrax_finish<C>, v_hyrax_read<C>, v_hyrax_eval_comm_compressed<C>, v_hyrax_commit<C>, v_hyrax_eval_comm_own<C>,
                       v_hyrax_set_small_key<C>};
}

}  // namespace reef
