// Host side of row N3 (bound rows / evaluation of a multilinear table); included after engine.inc.
namespace reef {

template <int C, int EB>
static void mle_launch_bound(hipStream_t st, const void *d_z, u64 n, u32 rows, u32 cols, u32 rows_per_chunk, u32 chunks,
                             const fe_limbs *Leq, fe256 *part) {
    hipLaunchKernelGGL((k_mle_bound<1 - C, EB>), dim3(ceil_div(cols, 256), chunks), dim3(256), 0, st, d_z, n, rows, cols, rows_per_chunk, Leq,
                       part);
}

// The row chunks of k_mle_bound: enough (column, row-chunk) threads to fill the chip; 32-bit symbols: short chunks (limb sums stay
// below 2^64).  REEF_ERR_ARG when the matrix is too tall for one pass.
static reef_status mle_plan(u32 rows, u32 cols, int elem_bytes, u32 *chunks_out, u32 *rows_per_chunk_out) {
    u32 chunks = (u32)std::min<u64>(rows, std::max<u64>(1, 262144 / cols));
    u32 rows_per_chunk = ceil_div(rows, chunks);
    if (elem_bytes == 4) rows_per_chunk = std::min<u32>(rows_per_chunk, 128);
    if (elem_bytes == 32) rows_per_chunk = std::min<u32>(rows_per_chunk, 1024);   // bound of the lazy 18-column reduction
    chunks = ceil_div(rows, rows_per_chunk);
    if (chunks > 65535) { set_error("matrix too tall for one pass (%u row chunks)", chunks); return REEF_ERR_ARG; }
    *chunks_out = chunks;
    *rows_per_chunk_out = rows_per_chunk;
    return REEF_OK;
}
template <int C>
static void mle_launch_bound_any(hipStream_t st, int elem_bytes, const void *d_z, u64 n, u32 rows, u32 cols, u32 rows_per_chunk, u32 chunks,
                                 const fe_limbs *Leq, fe256 *part) {
    switch (elem_bytes) {
    case 1: mle_launch_bound<C, 1>(st, d_z, n, rows, cols, rows_per_chunk, chunks, Leq, part); break;
    case 2: mle_launch_bound<C, 2>(st, d_z, n, rows, cols, rows_per_chunk, chunks, Leq, part); break;
    case 4: mle_launch_bound<C, 4>(st, d_z, n, rows, cols, rows_per_chunk, chunks, Leq, part); break;
    default: mle_launch_bound<C, 32>(st, d_z, n, rows, cols, rows_per_chunk, chunks, Leq, part); break;
    }
}

// lz_out[j] = sum_i eq(point[..left], i) * Z[i*2^(m-left) + j]   (2^(m-left) values; may be null)
// eval_out  = sum_j lz[j] * eq(point[left..], j)                  (host; may be null)
template <int C>
static reef_status v_mle_bound(const void *z, size_t n, int elem_bytes, int z_loc, bool is_mont, const reef_fe *point, size_t num_vars,
                               size_t left_vars, reef_fe *lz_out, int out_loc, reef_fe *eval_out) {
    constexpr int F = 1 - C;
    if ((n && !z) || (num_vars && !point) || (!lz_out && !eval_out)) { set_error("null argument"); return REEF_ERR_ARG; }
    if (num_vars > 28 || left_vars > num_vars) { set_error("num_vars must be <= 28 and left_vars <= num_vars"); return REEF_ERR_ARG; }
    if (n > ((size_t)1 << num_vars)) { set_error("n = %zu exceeds 2^num_vars", n); return REEF_ERR_ARG; }
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 32) { set_error("elem_bytes must be 1, 2, 4 or 32"); return REEF_ERR_ARG; }
    const u32 rows = 1u << left_vars, cols = 1u << (num_vars - left_vars);
    ScratchStream ss;
    REEF_TRY(ss.init());
    const unsigned char *d_z = nullptr;
    if (n) REEF_TRY(stage_in<unsigned char>(ss, &d_z, z, n * (size_t)elem_bytes, z_loc));
    MlePoint pt;
    memset(&pt, 0, sizeof pt);
    if (num_vars) memcpy(pt.r, point, num_vars * sizeof(fe256));
    void *p_eq = nullptr, *p_part = nullptr, *p_dot = nullptr;
    REEF_TRY(ss.alloc(&p_eq, ((size_t)rows + cols) * sizeof(fe_limbs)));
    fe_limbs *Leq = (fe_limbs *)p_eq, *Req = Leq + rows;
    hipLaunchKernelGGL(k_mle_eq<F>, dim3(ceil_div(rows, 256)), dim3(256), 0, ss.s, pt, 0u, (u32)left_vars, (int)is_mont, Leq);
    hipLaunchKernelGGL(k_mle_eq<F>, dim3(ceil_div(cols, 256)), dim3(256), 0, ss.s, pt, (u32)left_vars, (u32)(num_vars - left_vars), (int)is_mont, Req);
    u32 chunks = 0, rows_per_chunk = 0;
    REEF_TRY(mle_plan(rows, cols, elem_bytes, &chunks, &rows_per_chunk));
    REEF_TRY(ss.alloc(&p_part, (size_t)chunks * cols * sizeof(fe256)));
    REEF_TRY(ss.alloc(&p_dot, 9 * sizeof(u64) + sizeof(fe256)));
    fe256 *part = (fe256 *)p_part;
    unsigned long long *dot = (unsigned long long *)p_dot;
    fe256 *d_eval = (fe256 *)(dot + 9);
    REEF_HIP_TRY(hipMemsetAsync(dot, 0, 9 * sizeof(u64), ss.s));
    mle_launch_bound_any<C>(ss.s, elem_bytes, d_z, n, rows, cols, rows_per_chunk, chunks, Leq, part);
    fe256 *d_lz = nullptr;
    if (lz_out) REEF_TRY(stage_out<fe256>(ss, &d_lz, lz_out, cols, out_loc));
    if (elem_bytes == 32) {
        hipLaunchKernelGGL((k_mle_finish<F, false>), dim3(ceil_div(cols, 256)), dim3(256), 0, ss.s, part, chunks, cols, Req, (int)is_mont, d_lz, dot);
        hipLaunchKernelGGL((k_mle_eval_final<F, false>), dim3(1), dim3(64), 0, ss.s, dot, (int)is_mont, d_eval);
    } else {
        hipLaunchKernelGGL((k_mle_finish<F, true>), dim3(ceil_div(cols, 256)), dim3(256), 0, ss.s, part, chunks, cols, Req, (int)is_mont, d_lz, dot);
        hipLaunchKernelGGL((k_mle_eval_final<F, true>), dim3(1), dim3(64), 0, ss.s, dot, (int)is_mont, d_eval);
    }
    REEF_HIP_TRY(hipGetLastError());
    if (eval_out) REEF_HIP_TRY(hipMemcpyAsync(eval_out, d_eval, sizeof(fe256), hipMemcpyDeviceToHost, ss.s));
    if (lz_out && out_loc != REEF_DEVICE) REEF_HIP_TRY(hipMemcpyAsync(lz_out, d_lz, cols * sizeof(fe256), hipMemcpyDeviceToHost, ss.s));
    REEF_HIP_TRY(hipStreamSynchronize(ss.s));
    return REEF_OK;
}

}  // namespace reef
