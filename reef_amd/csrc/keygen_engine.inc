// Host side of commitment-key derivation (row N1); included after merkle_engine.inc.
#include "keccak.h"
#include "fe_scalars_host.inc"   // fe_valid
namespace reef {

// out[i] = hash_to_curve(SHAKE256(label)[32 i .. 32 i + 32)) for i < n, affine ABI points of curve C (identity = (0, 0)).
template <int C>
static reef_status v_derive_generators(const uint8_t *label, size_t label_len, size_t n, const reef_keygen_params *kp, bool is_mont, reef_affine *out,
                                       int out_loc) {
    if (!kp || !out || (label_len && !label) || (kp->dst_len && !kp->dst)) { set_error("null argument"); return REEF_ERR_ARG; }
    if (kp->dst_len > 255) { set_error("domain separation string longer than 255 bytes (RFC 9380 5.3.3 asks for a hashed tag then)"); return REEF_ERR_ARG; }
    if (n == 0 || n >= (1ull << 27)) { set_error("generator count out of range"); return REEF_ERR_ARG; }
    const reef_fe *const named[3] = {&kp->a, &kp->b, &kp->z};      // the 16 field elements, in either form, are below the modulus of field C
    for (u32 i = 0; i < 3; ++i)
        if (!fe_valid(named[i], C)) { set_error("reef_derive_generators: %s is not below the modulus", i == 0 ? "a" : i == 1 ? "b" : "z"); return REEF_ERR_ARG; }
    for (u32 i = 0; i < 13; ++i)
        if (!fe_valid(kp->iso + i, C)) { set_error("reef_derive_generators: iso[%u] is not below the modulus", i); return REEF_ERR_ARG; }
    ScratchStream ss;
    REEF_TRY(ss.init());
    constexpr u32 NCONST = 16;                     // a, b, z, iso[13]
    std::vector<uint8_t> up(NCONST * sizeof(fe256) + 256, 0);
    memcpy(up.data(), &kp->a, sizeof(fe256));
    memcpy(up.data() + sizeof(fe256), &kp->b, sizeof(fe256));
    memcpy(up.data() + 2 * sizeof(fe256), &kp->z, sizeof(fe256));
    memcpy(up.data() + 3 * sizeof(fe256), kp->iso, 13 * sizeof(fe256));
    if (kp->dst_len) memcpy(up.data() + NCONST * sizeof(fe256), kp->dst, kp->dst_len);
    void *raw = nullptr, *cst = nullptr, *chunks = nullptr, *tmp = nullptr;
    REEF_TRY(ss.alloc(&raw, up.size()));
    REEF_TRY(ss.alloc(&cst, NCONST * sizeof(fe256)));
    REEF_TRY(ss.alloc(&chunks, n * 32));
    REEF_TRY(ss.alloc(&tmp, n * sizeof(xyzz_mem)));
    REEF_HIP_TRY(hipMemcpyAsync(raw, up.data(), up.size(), hipMemcpyHostToDevice, ss.s));
    hipLaunchKernelGGL(k_fe_import<C>, dim3(1), dim3(256), 0, ss.s, (const fe256 *)raw, NCONST, (int)is_mont, (fe256 *)cst);   // coordinates: field C
    KeygenDev kd{(const fe256 *)cst, (const unsigned char *)raw + NCONST * sizeof(fe256), kp->dst_len, kp->little_endian ? 1u : 0u};
    // The XOF stream is sequential and produced by this thread; it is squeezed in pieces so that the maps of one piece run on
    // the GPU while the next piece is being squeezed.  A piece's kernel is a latency chain (~2.5 ms whatever the count, on half
    // of the chip's SIMDs) and the sponge now delivers a piece in 1.6 ms, so consecutive pieces go to two streams and their
    // kernels run side by side: the wall time is the stream plus ONE kernel, not the sum of the kernels.
    constexpr size_t PIECE = 32768;                // generators per piece: 1 MiB of stream, 1024 workgroups of one wave (two lanes per generator)
    std::vector<uint8_t> stream(n * 32);
    Shake256 xof(label, label_len);
    hipStream_t lanes[2] = {ss.s, ss.s};
    hipEvent_t *ev = nullptr;
    const bool two = n > PIECE;
    if (two) {
        REEF_TRY(ss.side(&lanes[1], &ev));
        REEF_HIP_TRY(hipEventRecord(ev[0], ss.s));                       // the constants are imported on the first stream
        REEF_HIP_TRY(hipStreamWaitEvent(lanes[1], ev[0], 0));
    }
    size_t piece = 0;
    for (size_t at = 0; at < n; at += PIECE, ++piece) {
        const size_t cnt = std::min(PIECE, n - at);
        hipStream_t st = lanes[piece & 1];
        xof.squeeze(stream.data() + at * 32, cnt * 32);
        REEF_HIP_TRY(hipMemcpyAsync((uint8_t *)chunks + at * 32, stream.data() + at * 32, cnt * 32, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_hash_to_curve<C>, dim3((u32)ceil_div(2 * cnt, 64)), dim3(64), 0, st, (const unsigned char *)chunks + at * 32, (u32)cnt, kd,
                           (xyzz_mem *)tmp + at);
    }
    if (two) {                                                           // the normalisation reads what both streams wrote
        REEF_HIP_TRY(hipEventRecord(ev[1], lanes[1]));
        REEF_HIP_TRY(hipStreamWaitEvent(ss.s, ev[1], 0));
    }
    affine256 *d_out = (affine256 *)out;
    if (out_loc != REEF_DEVICE) {
        void *o = nullptr;
        REEF_TRY(ss.alloc(&o, n * sizeof(affine256)));
        d_out = (affine256 *)o;
    }
    hipLaunchKernelGGL((k_xyzz_normalize<C, true>), dim3((u32)ceil_div(ceil_div(n, NORM_PER), 256)), dim3(256), 0, ss.s, (const xyzz_mem *)tmp, (u32)n, d_out);
    REEF_HIP_TRY(hipGetLastError());
    if (out_loc != REEF_DEVICE) REEF_HIP_TRY(hipMemcpyAsync(out, d_out, n * sizeof(affine256), hipMemcpyDeviceToHost, ss.s));
    REEF_HIP_TRY(hipStreamSynchronize(ss.s));      // `stream`, `up` leave scope
    return REEF_OK;
}

}  // namespace reef
