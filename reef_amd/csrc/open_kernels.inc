// The batched IPA opening of the final SNARK (include/reef_msm.h 3h): nova-snark's EE::prove_batch over [E, W] [R] --
// NIFSForInnerProduct's fold of the two instances, then InnerProductArgument::prove -- on the vectors row N5 leaves on a NIFS ctx.
// open_engine.inc drives them; the cross terms L, R are the existing IPA MSMs (ipa_cross_run in engine.inc) over the resident key.
//
//   begin   cross = <E, eq(r_y[1..])> + <W, eq(r_x)> over the common prefixes                          (k_op_cross)
//   fold    a = E + r W, b = eq(r_x) + r eq(r_y[1..]), zero-padded to n; c = <a, b> and round 0's c_L, c_R  (k_op_fold)
//   round   a' = a_lo r + a_hi r^-1, b' = b_lo r^-1 + b_hi r, fused with the next round's c_L, c_R       (k_op_round)
//   finish  the last fold: a_hat = a[0]                                                                    (k_op_last)
//
// a holds canonical integers (what the cross-term MSM reads), b the resident internal form.  The sums go through
// sp_block_sums / k_sp_finish (spartan_kernels.inc): partial[block][27], values 0 c, 1 c_L, 2 c_R.

namespace reef {

// x[i] for i < len, else 0 (internal form)
__device__ __forceinline__ fe op_load(const fe256 *x, u32 i, u32 len) { return i < len ? fe_from_table(load_fe256(x + i)) : fe_zero(); }

// <E, e2> over i < nE plus <W, e1> over i < nW: one value
template <int F>
__global__ void __launch_bounds__(SP_THREADS) k_op_cross(const fe256 *__restrict__ E, const fe256 *__restrict__ e2, u32 nE, const fe256 *__restrict__ W,
                                                         const fe256 *__restrict__ e1, u32 nW, unsigned long long *__restrict__ partial) {
    u64 acc[1][9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[0][i] = 0;
    const u32 n = nE > nW ? nE : nW;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        if (i < nE) sp_acc(acc[0], fe_mul<F>(fe_from_table(load_fe256(E + i)), fe_from_table(load_fe256(e2 + i))));
        if (i < nW) sp_acc(acc[0], fe_mul<F>(fe_from_table(load_fe256(W + i)), fe_from_table(load_fe256(e1 + i))));
    }
    sp_block_sums<1>(acc, partial);
}

struct OpFold {
    const fe256 *E, *W, *e1, *e2;    // E (nE entries), W (nW), eq(r_x) (n1), eq(r_y[1..]) (n2): internal form
    u32 nE, nW, n1, n2, h;           // h = n / 2
    fe256 r;                         // internal form
    fe256 *a, *b;                    // n entries each
    unsigned long long *partial;
};
// Thread i < h writes a[i], a[i + h], b[i], b[i + h] and adds a b at both (c), a[i] b[i + h] (c_L) and a[i + h] b[i] (c_R).
template <int F>
__global__ void __launch_bounds__(SP_THREADS) k_op_fold(OpFold p) {
    const fe r = fe_from_table(p.r);
    u64 acc[3][9];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < 9; ++i) acc[k][i] = 0;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < p.h; i += gridDim.x * blockDim.x) {
        fe a[2], b[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const u32 j = i + s * p.h;
            a[s] = fe_canon<F>(fe_add<F>(op_load(p.E, j, p.nE), fe_mul<F>(r, op_load(p.W, j, p.nW))));
            b[s] = fe_canon<F>(fe_add<F>(op_load(p.e1, j, p.n1), fe_mul<F>(r, op_load(p.e2, j, p.n2))));
            store_fe256(p.a + j, fe_to_integer<F>(a[s]));
            store_fe256(p.b + j, fe_pack(b[s]));
        }
        sp_acc(acc[0], fe_mul<F>(a[0], b[0]));
        sp_acc(acc[0], fe_mul<F>(a[1], b[1]));
        sp_acc(acc[1], fe_mul<F>(a[0], b[1]));
        sp_acc(acc[2], fe_mul<F>(a[1], b[0]));
    }
    sp_block_sums<3>(acc, p.partial);
}

// x r1 + y r2, canonical
template <int F> __device__ __forceinline__ fe op_fold2(const fe &x, const fe &r1, const fe &y, const fe &r2) {
    return fe_canon<F>(fe_add<F>(fe_mul<F>(x, r1), fe_mul<F>(y, r2)));
}

struct OpRound {
    fe256 *a, *b;                    // 4 q entries before the fold, 2 q after
    u32 q;
    fe256 r, rinv;                   // internal form
    unsigned long long *partial;
};
// One IPA fold fused with the next round's sums.  Thread i < q reads a[i + t q], b[i + t q] (t < 4), writes the folded entries i
// and i + q of both (in place: no other thread reads them) and adds a'[i] b'[i + q] (c_L) and a'[i + q] b'[i] (c_R).
template <int F>
__global__ void __launch_bounds__(SP_THREADS) k_op_round(OpRound p) {
    const fe r = fe_from_table(p.r), ri = fe_from_table(p.rinv);
    u64 acc[2][9];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int i = 0; i < 9; ++i) acc[k][i] = 0;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < p.q; i += gridDim.x * blockDim.x) {
        fe a[2], b[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const u32 j = i + s * p.q;
            a[s] = op_fold2<F>(fe_from_integer<F>(load_fe256(p.a + j)), r, fe_from_integer<F>(load_fe256(p.a + j + 2 * p.q)), ri);
            b[s] = op_fold2<F>(fe_from_table(load_fe256(p.b + j)), ri, fe_from_table(load_fe256(p.b + j + 2 * p.q)), r);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            store_fe256(p.a + i + s * p.q, fe_to_integer<F>(a[s]));
            store_fe256(p.b + i + s * p.q, fe_pack(b[s]));
        }
        sp_acc(acc[0], fe_mul<F>(a[0], b[1]));
        sp_acc(acc[1], fe_mul<F>(a[1], b[0]));
    }
    sp_block_sums<2>(acc, p.partial);
}

// The last fold (two entries left): a[0] = a[0] r + a[1] r^-1, b[0] = b[0] r^-1 + b[1] r; out = a[0] in `form`.  One thread.
template <int F>
__global__ void __launch_bounds__(64) k_op_last(fe256 *__restrict__ a, fe256 *__restrict__ b, fe256 r_, fe256 rinv_, int form, fe256 *__restrict__ out) {
    if (threadIdx.x != 0) return;
    const fe r = fe_from_table(r_), ri = fe_from_table(rinv_);
    const fe av = op_fold2<F>(fe_from_integer<F>(load_fe256(a)), r, fe_from_integer<F>(load_fe256(a + 1)), ri);
    const fe bv = op_fold2<F>(fe_from_table(load_fe256(b)), ri, fe_from_table(load_fe256(b + 1)), r);
    store_fe256(a, fe_to_integer<F>(av));
    store_fe256(b, fe_pack(bv));
    store_fe256(out, sp_out<F>(av, form));
}

}  // namespace reef
