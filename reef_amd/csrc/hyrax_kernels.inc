// The Hyrax consistency argument (include/reef_msm.h 3i): HyraxPC::prove_eval [R] over the resident document.  hyrax_engine.inc
// drives it with the kernels of 3c and 3h; the one kernel here is the first round's sums, which 3h takes from its fold:
//
//   eval_begin  L = eq(point[..left]), a = LZ = L^T Z (k_mle_eq, k_mle_bound, k_mle_finish), eval = <a, b>;
//               b = eq(point[left..]) (k_sp_eq); the blinds as a one-column table give sum_i L_i blind_i
//   ipa_begin   round 0's c_L = <a_lo, b_hi>, c_R = <a_hi, b_lo>                                        (k_hy_sums)
//   rounds      3h's IpaRun: k_op_round, the cross-term MSMs, k_op_last
//
// a holds canonical integers, b the internal form, as in 3h.  The sums go through sp_block_sums / k_sp_finish.
//
//   commit      the width of the resident symbols (k_hy_sym_or, once per ctx); the row sums are K2's, the blinds k_add_blind_tab's,
//               the affine and the encoded rows k_normalize's

namespace reef {

// The OR of the document's 32-bit words into *out: the bit length of the largest symbol is the bit length of the OR of them all, so
// the words need not be taken apart here (the host folds the bytes or halves of *out).  z: n16 16-byte words, the tail past the
// document zeroed (reef_hyrax_create).  One atomic per wave that saw a set bit.
static __global__ void __launch_bounds__(256) k_hy_sym_or(const uint4 *__restrict__ z, u64 n16, u32 *__restrict__ out) {
    u32 acc = 0;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (u64)gridDim.x * blockDim.x) {
        const uint4 v = z[i];
        acc |= v.x | v.y | v.z | v.w;
    }
    for (int d = 32; d > 0; d >>= 1) acc |= (u32)__shfl_xor(acc, d, WAVE);
    if ((threadIdx.x & 63) == 0 && acc) atomicOr(out, acc);
}

// c_L = sum_{i < h} a[i] b[i + h], c_R = sum_{i < h} a[i + h] b[i] -> partial[block][27], values 0 and 1
template <int F>
__global__ void __launch_bounds__(SP_THREADS) k_hy_sums(const fe256 *__restrict__ a, const fe256 *__restrict__ b, u32 h,
                                                        unsigned long long *__restrict__ partial) {
    u64 acc[2][9];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int i = 0; i < 9; ++i) acc[k][i] = 0;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < h; i += gridDim.x * blockDim.x) {
        const fe a0 = fe_from_integer<F>(load_fe256(a + i)), a1 = fe_from_integer<F>(load_fe256(a + i + h));
        sp_acc(acc[0], fe_mul<F>(a0, fe_from_table(load_fe256(b + i + h))));
        sp_acc(acc[1], fe_mul<F>(a1, fe_from_table(load_fe256(b + i))));
    }
    sp_block_sums<2>(acc, partial);
}

}  // namespace reef
