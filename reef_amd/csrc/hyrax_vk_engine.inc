// The verifier's key of a committed document (include/reef_msm.h 3n): the 2^left row commitments decoded and keyed once, then
// comm_LZ = sum_i eq(point[..left])_i C_i for any number of points per call.  Included after hyrax_engine.inc.  A call is three
// steps on the stream of the vk's own key ctx, one after the other with no host wait between them: one k_mle_eq_batch launch writes
// the m x 2^left weights as canonical integers, the row pipeline (v_msm_rows: rows = m, row_len = 2^left, device scalars, no blinds)
// sums them over the resident key, one k_normalize launch encodes the m results; then the copies to the host and the call's one wait.
namespace reef {

template <int C> struct HyraxVk : DeviceCtx {   // mu serialises the calls on one vk; the stream is create's (the decode)
    static constexpr int F = 1 - C;      // scalar field of curve C
    u32 left = 0, rows = 0;
    Ctx<C> *key = nullptr;               // the key over the decoded rows.  Nobody else holds it: no window split can be set on it
    DevBuf enc, dec, stat;               // create: the encodings of host rows, the decoded rows the key is built from, the decode's two counters
    DevBuf pts, wts, jac, out32;         // comm_lz: the m points as uploaded, the m x 2^left weights, the m sums, their encodings (grow-only)
};

template <int C> static void hyrax_vk_free(HyraxVk<C> *c) {
    if (!c) return;
    retire_device_ctx(c);
    if (c->key) v_ctx_destroy<C>(c->key);            // waits for its stream first: nothing reads the buffers below any more
    for (DevBuf *b : {&c->enc, &c->dec, &c->stat, &c->pts, &c->wts, &c->jac, &c->out32}) b->release();
    delete c;
}

template <int C>
static reef_status v_hyrax_vk_create(void **impl, const uint8_t *row_comms32, size_t left_vars, int loc, int device, const reef_msm_opts *key_opts) {
    if (!impl || !row_comms32) { set_error("null argument"); return REEF_ERR_ARG; }
    if (left_vars < 1 || left_vars > 25) { set_error("reef_hyrax_vk_create: left_vars = %zu is outside 1 .. 25", left_vars); return REEF_ERR_ARG; }
    if (loc == REEF_DEVICE && ((uintptr_t)row_comms32 & 15)) { set_error("reef_hyrax_vk_create: device rows must be 16-byte aligned"); return REEF_ERR_ARG; }
    if (device < 0) REEF_HIP_TRY(hipGetDevice(&device));
    const u32 rows = 1u << left_vars;
    reef_msm_opts o;
    memset(&o, 0, sizeof o);
    if (key_opts) o = *key_opts;
    o.device = device;
    REEF_TRY(plan_for(rows, o.window_bits, o.bucket_groups, nullptr, nullptr, nullptr, nullptr));   // an impossible key is refused before any device work
    return create_device_ctx<HyraxVk<C>>(impl, device, "reef_hyrax_vk_create", false, hyrax_vk_free<C>, [&](HyraxVk<C> *c) -> reef_status {
        c->left = (u32)left_vars;
        c->rows = rows;
        const size_t bytes = (size_t)rows * 32;
        REEF_TRY(c->dec.ensure_exact(rows * sizeof(affine256)));
        REEF_TRY(c->stat.ensure(2 * sizeof(u64)));
        {
            DeviceScope scope(c, OnExit::WAIT_AND_IDLE);
            REEF_TRY(scope.enter());
            const fe256 *enc = (const fe256 *)row_comms32;
            if (loc != REEF_DEVICE) {
                REEF_TRY(c->enc.ensure_exact(bytes));
                REEF_HIP_TRY(hipMemcpyAsync(c->enc.p, row_comms32, bytes, hipMemcpyHostToDevice, c->stream));
                enc = c->enc.template as<fe256>();
            }
            decompress_launch<C>(c->stream, enc, rows, c->dec.template as<affine256>(), c->stat.template as<unsigned long long>());
            REEF_HIP_TRY(hipGetLastError());
            u64 stats[2] = {0, 0};
            REEF_HIP_TRY(hipMemcpyAsync(stats, c->stat.p, sizeof stats, hipMemcpyDeviceToHost, c->stream));
            REEF_HIP_TRY(hipStreamSynchronize(c->stream));
            if (stats[0]) {
                set_error("reef_hyrax_vk_create: row %llu is not the encoding of a point (%llu such rows)", (unsigned long long)stats[1],
                          (unsigned long long)stats[0]);
                return REEF_ERR_ARG;
            }
        }
        void *k = nullptr;
        REEF_TRY(v_ctx_create<C>(&k, (const reef_affine *)c->dec.p, rows, REEF_DEVICE, &o));   // device to device; waits for the tables
        c->key = (Ctx<C> *)k;
        for (DevBuf *b : {&c->enc, &c->dec, &c->stat}) b->release();                           // the key holds the rows from here on
        return REEF_OK;
    });
}
template <int C> static void v_hyrax_vk_destroy(void *impl) { hyrax_vk_free((HyraxVk<C> *)impl); }

template <int C>
static reef_status v_hyrax_vk_comm_lz(void *impl, const reef_fe *points, size_t m, bool is_mont, reef_jacobian *comm_lz, uint8_t *comm_lz32) {
    constexpr int F = HyraxVk<C>::F;
    HyraxVk<C> *c = (HyraxVk<C> *)impl;
    if (!comm_lz && !comm_lz32) { set_error("reef_hyrax_vk_comm_lz: comm_lz and comm_lz32 are both NULL"); return REEF_ERR_ARG; }
    if (m == 0) return REEF_OK;
    if (!points) { set_error("null argument"); return REEF_ERR_ARG; }
    if (m >= ((size_t)1 << (31 - c->left))) {
        set_error("reef_hyrax_vk_comm_lz: m * 2^left_vars = %zu * %u reaches 2^31", m, c->rows);
        return REEF_ERR_ARG;
    }
    for (size_t t = 0; t < m; ++t)
        for (u32 j = 0; j < c->left; ++j)
            if (!fe_valid(points + t * c->left + j, F)) {
                set_error("reef_hyrax_vk_comm_lz: points[%zu][%u] is not below the modulus", t, j);
                return REEF_ERR_ARG;
            }
    DeviceCall call(c, OnExit::WAIT_AND_IDLE);                // the vk's lock alone: the work below runs on the key ctx's stream, so the
    REEF_ON_DEVICE(c->device);                                // vk's own scope is never entered and the call has the one wait at its end
    Ctx<C> *key = c->key;
    const size_t N = m * (size_t)c->rows;
    {
        std::lock_guard<std::mutex> kl(key->mu);
        CtxScope<C> scope(key);
        REEF_TRY(scope.enter());
        REEF_TRY(c->pts.ensure(m * c->left * sizeof(fe256)));
        REEF_TRY(c->wts.ensure(N * sizeof(fe256)));
        REEF_TRY(c->jac.ensure(m * sizeof(jacobian256)));
        if (comm_lz32) REEF_TRY(c->out32.ensure(m * sizeof(fe256)));
        REEF_HIP_TRY(hipMemcpyAsync(c->pts.p, points, m * c->left * sizeof(fe256), hipMemcpyHostToDevice, key->stream));
        hipLaunchKernelGGL(k_mle_eq_batch<F>, dim3(ceil_div(c->rows, 256), (u32)std::min<size_t>(m, 65535)), dim3(256), 0, key->stream,
                           (const fe256 *)c->pts.p, (u32)m, c->left, (int)is_mont, c->wts.template as<fe256>());
        REEF_HIP_TRY(hipGetLastError());
    }
    // full-width scalars (max_bits = 255: the route measures nothing and waits for nothing), results left on the device
    REEF_TRY(v_msm_rows<C>(key, (const reef_fe *)c->wts.p, m, c->rows, REEF_DEVICE, false, 255, nullptr, nullptr, c->jac.template as<reef_jacobian>(),
                           REEF_DEVICE));
    std::lock_guard<std::mutex> kl(key->mu);
    CtxScope<C> scope(key);
    REEF_TRY(scope.enter());
    hipStream_t st = key->stream;
    if (comm_lz32) {
        hipLaunchKernelGGL(k_normalize<C>, dim3(ceil_div(ceil_div(m, NORM_PER), 256)), dim3(256), 0, st, (const jacobian256 *)c->jac.p, (u32)m,
                           (affine256 *)nullptr, c->out32.template as<fe256>());
        REEF_HIP_TRY(hipGetLastError());
        REEF_HIP_TRY(hipMemcpyAsync(comm_lz32, c->out32.p, m * sizeof(fe256), hipMemcpyDeviceToHost, st));
    }
    if (comm_lz) REEF_HIP_TRY(hipMemcpyAsync(comm_lz, c->jac.p, m * sizeof(jacobian256), hipMemcpyDeviceToHost, st));
    REEF_HIP_TRY(hipStreamSynchronize(st));
    return REEF_OK;
}

template <int C> HyraxVkVTable make_hyrax_vk_vtable() { return HyraxVkVTable{v_hyrax_vk_create<C>, v_hyrax_vk_destroy<C>, v_hyrax_vk_comm_lz<C>}; }

}  // namespace reef
