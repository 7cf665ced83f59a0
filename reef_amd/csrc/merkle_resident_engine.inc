// Host side of the resident Poseidon Merkle tree (include/reef_msm.h 3d, reef_merkle_create ...); included after fe_host.inc.  The tree is
// built by merkle_engine.inc's helpers -- the kernels, level layout and sparse-constant cache of reef_merkle_commit -- into buffers the ctx
// keeps: the document, all levels in table form, the constants.  No exported copy of the tree exists anywhere; openings are gathered from
// it (k_merkle_open) and claimed openings are hashed back to the root (k_pos_paths).  Every call waits for its work before it returns.
namespace reef {

template <int C> struct MerkleCtx : DeviceCtx {
    static constexpr int F = 1 - C;      // scalar field of curve C
    DevBuf doc, tree, cst, raw;          // the symbols (u32); all levels, level 0 first (table form); the constants and tags; their staging, then the root's
    DevBuf qin, stage;                   // a call's packed inputs; its packed outputs
    std::vector<unsigned char> host;     // the host end of both (grow-only)
    MerkleShape sh{};
    u64 total = 0;
    bool is_mont = false;
    PosSetup<F> ps;
    reef_fe root{};                      // in the caller's form
};

template <int C> static void merkle_free(MerkleCtx<C> *c) {
    if (!c) return;
    retire_device_ctx(c);
    for (DevBuf *b : {&c->doc, &c->tree, &c->cst, &c->raw, &c->qin, &c->stage}) b->release();
    delete c;
}

template <int C>
static reef_status v_merkle_create(void **impl, const reef_poseidon_params *pp, const uint32_t *doc, size_t n, int doc_loc, bool is_mont, int device) {
    constexpr int F = MerkleCtx<C>::F;
    if (!impl || !pp || !pp->round_constants || !pp->mds || (n && !doc)) { set_error("null argument"); return REEF_ERR_ARG; }
    REEF_TRY(merkle_check_params(pp));
    if (n == 0 || n >= (1ull << 33)) { set_error("document length out of range"); return REEF_ERR_ARG; }
    const std::vector<u64> sizes = merkle_level_sizes(n);
    return create_device_ctx<MerkleCtx<C>>(impl, device, "reef_merkle_create", false, merkle_free<C>, [&](MerkleCtx<C> *c) -> reef_status {
        c->is_mont = is_mont;
        c->sh.n = n;
        c->sh.levels = (u32)sizes.size();
        for (size_t h = 0; h < sizes.size(); ++h) {
            c->sh.off[h] = c->total;
            c->sh.len[h] = sizes[h];
            c->total += sizes[h];
        }
        REEF_TRY(c->doc.ensure_exact(n * sizeof(u32)));                 // 0.5 GiB + 4 GiB at 2^27 symbols: no head-room
        REEF_TRY(c->tree.ensure_exact(c->total * sizeof(fe256)));
        DeviceScope scope(c, OnExit::WAIT_AND_IDLE);
        REEF_TRY(scope.enter());
        REEF_HIP_TRY(hipMemcpyAsync(c->doc.p, doc, n * sizeof(u32), doc_loc == REEF_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
        REEF_TRY(pos_setup<F>(c->stream, pp, is_mont, [&](int which, void **p, size_t bytes) -> reef_status {
            DevBuf &b = which == 0 ? c->cst : c->raw;
            REEF_TRY(b.ensure(bytes));
            *p = b.p;
            return REEF_OK;
        }, c->ps));
        fe256 *tree = c->tree.template as<fe256>();
        merkle_hash_levels<F>(c->stream, c->doc.template as<u32>(), n, 0, sizes, c->ps, tree);
        hipLaunchKernelGGL(k_fe_export<F>, dim3(1), dim3(256), 0, c->stream, (const fe256 *)(tree + (c->total - 1)), (u64)1, 0, (int)is_mont, c->raw.template as<fe256>());
        REEF_HIP_TRY(hipGetLastError());
        REEF_HIP_TRY(hipMemcpyAsync(&c->root, c->raw.p, sizeof(fe256), hipMemcpyDeviceToHost, c->stream));
        REEF_HIP_TRY(hipStreamSynchronize(c->stream));
        return REEF_OK;
    });
}
template <int C> static void v_merkle_destroy(void *impl) { merkle_free((MerkleCtx<C> *)impl); }

template <int C> static reef_status v_merkle_info(void *impl, uint64_t *n, uint32_t *levels, uint64_t *nodes, reef_fe *root) {
    MerkleCtx<C> *c = (MerkleCtx<C> *)impl;
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);          // the lock alone: nothing here touches the device
    if (n) *n = c->sh.n;
    if (levels) *levels = c->sh.levels;
    if (nodes) *nodes = c->total;
    if (root) *root = c->root;
    return REEF_OK;
}

// the first idx[j] that is no symbol of the document: REEF_ERR_ARG in the words of the call `name`
template <int C> static reef_status merkle_check_idx(MerkleCtx<C> *c, const char *name, const uint64_t *idx, size_t k) {
    for (size_t j = 0; j < k; ++j)
        if (idx[j] >= c->sh.n) {
            set_error("%s: idx[%zu] = %llu, the document has %llu symbols", name, j, (unsigned long long)idx[j], (unsigned long long)c->sh.n);
            return REEF_ERR_ARG;
        }
    return REEF_OK;
}

template <int C>
static reef_status v_merkle_open(void *impl, const uint64_t *idx, size_t k, uint32_t *symbols, uint64_t *opposite_idx, reef_fe *opposite, reef_fe *path) {
    constexpr int F = MerkleCtx<C>::F;
    MerkleCtx<C> *c = (MerkleCtx<C> *)impl;
    if (k == 0) return REEF_OK;
    if (!idx || !opposite) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(merkle_check_idx(c, "reef_merkle_open", idx, k));
    const size_t L = c->sh.levels, fes = k * L * sizeof(fe256);
    const size_t o_path = fes, o_oidx = o_path + (path ? fes : 0), o_sym = o_oidx + k * sizeof(u64), bytes = o_sym + k * sizeof(u32);
    REEF_TRY(call.enter());
    REEF_TRY(c->qin.ensure(k * sizeof(u64)));
    REEF_TRY(c->stage.ensure(bytes));
    c->host.resize(std::max(c->host.size(), bytes));
    unsigned char *d = c->stage.template as<unsigned char>(), *h = c->host.data();
    REEF_HIP_TRY(hipMemcpyAsync(c->qin.p, idx, k * sizeof(u64), hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_merkle_open<F>, dim3((u32)ceil_div((u64)(k * L), (u64)256)), dim3(256), 0, c->stream, (const u32 *)c->doc.p, (const fe256 *)c->tree.p, c->sh,
                       (const u64 *)c->qin.p, (u64)k, (int)c->is_mont, path ? 1 : 0, (fe256 *)d, (fe256 *)(d + o_path), (u64 *)(d + o_oidx), (u32 *)(d + o_sym));
    REEF_HIP_TRY(hipGetLastError());
    REEF_HIP_TRY(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    memcpy(opposite, h, fes);
    if (path) memcpy(path, h + o_path, fes);
    if (opposite_idx) memcpy(opposite_idx, h + o_oidx, k * sizeof(u64));
    if (symbols) memcpy(symbols, h + o_sym, k * sizeof(u32));
    return REEF_OK;
}

template <int C>
static reef_status v_merkle_read_level(void *impl, uint32_t level, uint64_t first, uint64_t count, reef_fe *out, int out_loc) {
    constexpr int F = MerkleCtx<C>::F;
    MerkleCtx<C> *c = (MerkleCtx<C> *)impl;
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    if (level >= c->sh.levels) { set_error("reef_merkle_read_level: level %u of a tree of %u", level, c->sh.levels); return REEF_ERR_ARG; }
    const u64 len = c->sh.len[level];
    if (first > len || count > len - first) {
        set_error("reef_merkle_read_level: nodes [%llu, %llu + %llu) of a level of %llu", (unsigned long long)first, (unsigned long long)first, (unsigned long long)count,
                  (unsigned long long)len);
        return REEF_ERR_ARG;
    }
    if (count == 0) return REEF_OK;
    if (!out) { set_error("null argument"); return REEF_ERR_ARG; }
    REEF_TRY(call.enter());
    fe256 *dst = (fe256 *)out;
    if (out_loc != REEF_DEVICE) {
        REEF_TRY(c->stage.ensure(count * sizeof(fe256)));
        dst = c->stage.template as<fe256>();
    }
    const fe256 *src = c->tree.template as<fe256>() + c->sh.off[level] + first;
    hipLaunchKernelGGL(k_fe_export<F>, dim3((u32)ceil_div(count, (u64)256)), dim3(256), 0, c->stream, src, count, 0, (int)c->is_mont, dst);
    REEF_HIP_TRY(hipGetLastError());
    if (out_loc != REEF_DEVICE) REEF_HIP_TRY(hipMemcpyAsync(out, dst, count * sizeof(fe256), hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    return REEF_OK;
}

template <int C>
static reef_status v_merkle_check_paths(void *impl, const uint64_t *idx, const uint32_t *symbols, const uint64_t *opposite_idx, const reef_fe *opposite, size_t k,
                                        uint32_t *accept) {
    constexpr int F = MerkleCtx<C>::F;
    MerkleCtx<C> *c = (MerkleCtx<C> *)impl;
    if (k == 0) return REEF_OK;
    if (!idx || !symbols || !opposite_idx || !opposite || !accept) { set_error("null argument"); return REEF_ERR_ARG; }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);
    REEF_TRY(merkle_check_idx(c, "reef_merkle_check_paths", idx, k));
    const size_t L = c->sh.levels, fes = k * L * sizeof(fe256);
    for (size_t i = 0; i < k * L; ++i)
        if (!fe_valid(opposite + i, F)) { set_error("reef_merkle_check_paths: opposite[%zu] is not below the modulus", i); return REEF_ERR_ARG; }
    const size_t o_idx = fes, o_oidx = o_idx + k * sizeof(u64), o_sym = o_oidx + k * sizeof(u64), bytes = o_sym + k * sizeof(u32);
    REEF_TRY(call.enter());
    REEF_TRY(c->qin.ensure(bytes));
    REEF_TRY(c->stage.ensure(k * sizeof(u32)));
    c->host.resize(std::max(c->host.size(), bytes));
    unsigned char *d = c->qin.template as<unsigned char>(), *h = c->host.data();
    memcpy(h, opposite, fes);
    memcpy(h + o_idx, idx, k * sizeof(u64));
    memcpy(h + o_oidx, opposite_idx, k * sizeof(u64));
    memcpy(h + o_sym, symbols, k * sizeof(u32));
    REEF_HIP_TRY(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, c->stream));
    const fe256 *root = c->tree.template as<fe256>() + (c->total - 1);
    u32 *acc = c->stage.template as<u32>();
    // k <= 12 * (the CUs of the chip) paths cost one chain of L hashes whatever k is; more than the five-lane form fills the chip with: a thread per path
    if (pos_spread_form<F>(c->ps, k))
        hipLaunchKernelGGL(k_pos_paths<F>, dim3((u32)ceil_div((u64)k, (u64)POS_SPREAD_PER_WAVE)), dim3(64), 0, c->stream, (const u64 *)(d + o_idx), (const u32 *)(d + o_sym),
                           (const u64 *)(d + o_oidx), (const fe256 *)d, (u64)k, (u32)L, (int)c->is_mont, c->ps.pd, c->ps.tags[0], c->ps.tags[1], root, acc);
    else
        hipLaunchKernelGGL(k_pos_paths_wide<F>, dim3((u32)ceil_div((u64)k, (u64)256)), dim3(256), 0, c->stream, (const u64 *)(d + o_idx), (const u32 *)(d + o_sym),
                           (const u64 *)(d + o_oidx), (const fe256 *)d, (u64)k, (u32)L, (int)c->is_mont, c->ps.pd, c->ps.tags[0], c->ps.tags[1], root, acc);
    REEF_HIP_TRY(hipGetLastError());
    REEF_HIP_TRY(hipMemcpyAsync(accept, acc, k * sizeof(u32), hipMemcpyDeviceToHost, c->stream));
    REEF_HIP_TRY(hipStreamSynchronize(c->stream));
    return REEF_OK;
}

template <int C> MerkleVTable make_merkle_vtable() {
    return MerkleVTable{v_merkle_create<C>, v_merkle_destroy<C>, v_merkle_info<C>, v_merkle_open<C>, v_merkle_read_level<C>, v_merkle_check_paths<C>};
}

}  // namespace reef
