// The Hyrax consistency arguments of many proofs over one resident document, advanced in lock-step (include/reef_msm.h 3p);
// hyrax_batch_engine.inc drives them.  Every kernel is the counterpart of one the single argument (3i) runs, with the proof index in
// blockIdx.y (or one thread per proof) and whatever differs per proof -- the point, the challenges -- read from device memory:
//
//   eval_begin  eq tables of a group of points (k_hyb_eq); per point 3c's k_mle_bound / k_mle_finish with LZ written into row i of a;
//               eval and lz_blind of all proofs (k_hyb_eval_final)
//   ipa_begin   round 0's c_L, c_R per proof (k_hyb_sums, k_hyb_finish)
//   round       the fold fused with the next round's sums (k_hyb_round, k_hyb_finish); the 2 m x n scalars of L and R over the
//               original key (k_hyb_coef, k_hyb_expand) for ONE pass of the row pipeline; c_L q_i, c_R q_i and the h term of all
//               2 m results in one launch (k_hyb_blind)
//   finish      the last fold of every proof (k_hyb_last)
//
// a holds canonical integers, b the internal form, as in 3h and 3i: row i of either is proof i's vector, `stride` entries apart.
// Every value a kernel stores is canonical, so proof i's outputs are bit for bit the single argument's.

namespace reef {

// k_mle_eq for the points t0 + blockIdx.y (nv entries each, in the caller's form): the `vars` coordinates from `first` on.
// eq[(blockIdx.y << vars) + i] as strictly reduced limbs (what k_mle_bound and k_mle_finish read); with btab also row t of b.
template <int F>
__global__ void __launch_bounds__(256) k_hyb_eq(const fe256 *__restrict__ pts, u32 nv, u32 first, u32 vars, int is_mont, u32 t0,
                                                fe_limbs *__restrict__ eq, fe256 *__restrict__ btab, u32 stride) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1u << vars)) return;
    const u32 t = t0 + blockIdx.y;
    const fe256 *p = pts + (size_t)t * nv + first;
    fe acc = fe_one<F>();
    for (u32 k = 0; k < vars; ++k) {
        const fe r = fe_from_caller<F>(load_fe256(p + k), is_mont);
        const fe one_minus = fe_sub<F, 2>(fe_one<F>(), r);
        const bool bit = (i >> (vars - 1 - k)) & 1u;
        acc = fe_mul<F>(acc, bit ? r : one_minus);
    }
    const fe c = fe_canon<F>(acc);
    fe_limbs o;
#pragma unroll
    for (int k = 0; k < 9; ++k) o.l[k] = c.l[k];
    eq[((size_t)blockIdx.y << vars) + i] = o;
    if (btab) store_fe256(btab + (size_t)t * stride + i, fe_pack(c));
}

// k_mle_eval_final for all proofs: thread 2 t folds proof t's limb sums of <LZ, R> (dot + 20 t), thread 2 t + 1 those of
// sum_i L_i blind_i (dot + 20 t + 10) -> res[2 t], res[2 t + 1], canonical integers.  compact: the document holds symbols.
template <int F>
__global__ void __launch_bounds__(256) k_hyb_eval_final(const unsigned long long *__restrict__ dot, u32 m, int compact, fe256 *__restrict__ res) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * m) return;
    const unsigned long long *d = dot + (size_t)(t >> 1) * 20 + (t & 1u) * 10;
    fe_wide w;
#pragma unroll
    for (int k = 0; k < 9; ++k) w.l[k] = d[k];
    const fe s = fe_from_wide<F>(w);
    store_fe256(res + t, (compact && !(t & 1u)) ? fe_to_integer<F>(s) : fe_pack(fe_canon<F>(s)));
}

// k_hy_sums per proof: c_L = sum_{i < h} a[i] b[i + h], c_R = sum_{i < h} a[i + h] b[i] -> partial[proof][block][27]
template <int F>
__global__ void __launch_bounds__(SP_THREADS) k_hyb_sums(const fe256 *__restrict__ a_, const fe256 *__restrict__ b_, u32 stride, u32 h,
                                                         unsigned long long *__restrict__ partial) {
    const fe256 *a = a_ + (size_t)blockIdx.y * stride, *b = b_ + (size_t)blockIdx.y * stride;
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
    sp_block_sums<2>(acc, partial + (size_t)blockIdx.y * gridDim.x * 27);
}

struct HybRound {
    fe256 *a, *b;                    // row i: 4 q entries before the fold, 2 q after
    u32 stride, q;
    const fe256 *r, *rinv;           // m entries each, internal form
    unsigned long long *partial;     // partial[proof][block][27]
};
// k_op_round with the proof in blockIdx.y: its r and r^-1 come from device memory, its block sums go to its own rows of partial
template <int F>
__global__ void __launch_bounds__(SP_THREADS) k_hyb_round(HybRound p) {
    const u32 t = blockIdx.y;
    const fe r = fe_from_table(load_fe256(p.r + t)), ri = fe_from_table(load_fe256(p.rinv + t));
    fe256 *pa = p.a + (size_t)t * p.stride, *pb = p.b + (size_t)t * p.stride;
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
            a[s] = op_fold2<F>(fe_from_integer<F>(load_fe256(pa + j)), r, fe_from_integer<F>(load_fe256(pa + j + 2 * p.q)), ri);
            b[s] = op_fold2<F>(fe_from_table(load_fe256(pb + j)), ri, fe_from_table(load_fe256(pb + j + 2 * p.q)), r);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            store_fe256(pa + i + s * p.q, fe_to_integer<F>(a[s]));
            store_fe256(pb + i + s * p.q, fe_pack(b[s]));
        }
        sp_acc(acc[0], fe_mul<F>(a[0], b[1]));
        sp_acc(acc[1], fe_mul<F>(a[1], b[0]));
    }
    sp_block_sums<2>(acc, p.partial + (size_t)t * gridDim.x * 27);
}

// k_sp_finish with one block per proof: out[2 t], out[2 t + 1] = c_L, c_R of proof t, canonical integers (the blinds of the q term)
template <int F>
__global__ void __launch_bounds__(SP_THREADS) k_hyb_finish(const unsigned long long *__restrict__ partial, u32 nblocks, fe256 *__restrict__ out) {
    sp_finish_body<F>(partial + (size_t)blockIdx.x * nblocks * 27, nblocks, 2u, (int)SP_FORM_INTEGER, out + 2 * (size_t)blockIdx.x);
}

// k_op_last, one thread per proof: a[0] = a[0] r + a[1] r^-1, b[0] = b[0] r^-1 + b[1] r; out[t] = a[0], out[m + t] = b[0] in `form`
template <int F>
__global__ void __launch_bounds__(256) k_hyb_last(fe256 *__restrict__ a_, fe256 *__restrict__ b_, u32 stride, u32 m, const fe256 *__restrict__ r_,
                                                  const fe256 *__restrict__ rinv_, int form, fe256 *__restrict__ out) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    fe256 *a = a_ + (size_t)t * stride, *b = b_ + (size_t)t * stride;
    const fe r = fe_from_table(load_fe256(r_ + t)), ri = fe_from_table(load_fe256(rinv_ + t));
    const fe av = op_fold2<F>(fe_from_integer<F>(load_fe256(a)), r, fe_from_integer<F>(load_fe256(a + 1)), ri);
    const fe bv = op_fold2<F>(fe_from_table(load_fe256(b)), ri, fe_from_table(load_fe256(b + 1)), r);
    store_fe256(a, fe_to_integer<F>(av));
    store_fe256(b, fe_pack(bv));
    store_fe256(out + t, sp_out<F>(av, form));
    store_fe256(out + m + t, sp_out<F>(bv, form));
}

// k_ipa_coef per proof, the challenges in device memory: chal[(2 j + 0) * m + t] = r of round j and proof t, [(2 j + 1) * m + t] its
// inverse (internal form).  coef[(t << k) + s] = prod_j (bit_{k-1-j}(s) ? r_j : r_j^-1), internal form.
template <int C>
__global__ void __launch_bounds__(256) k_hyb_coef(const fe256 *__restrict__ chal, u32 m, u32 k, fe256 *__restrict__ coef) {
    constexpr int F = 1 - C;
    const u32 s = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (s >= (1u << k)) return;
    fe acc = fe_one<F>();
    for (u32 j = 0; j < k; ++j) {
        const bool hi = (s >> (k - 1 - j)) & 1u;
        acc = fe_mul<F>(acc, fe_from_table(load_fe256(chal + (size_t)(2 * j + (hi ? 0u : 1u)) * m + t)));
    }
    store_fe256(coef + ((size_t)t << k) + s, fe_to_table<F>(acc));
}
// k_ipa_expand per proof: rows 2 t and 2 t + 1 of s (n canonical integers each) are proof t's L and R scalars over the original key,
// from its a (n_k entries, canonical integers) and its 2^k coefficients; half of either row is zero.
template <int C>
__global__ void __launch_bounds__(256) k_hyb_expand(const fe256 *__restrict__ a_, u32 stride, u32 n_k, const fe256 *__restrict__ coef_, u32 k, u32 n,
                                                    fe256 *__restrict__ s) {
    constexpr int F = 1 - C;
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (j >= n) return;
    const fe256 *a = a_ + (size_t)t * stride, *coef = coef_ + ((size_t)t << k);
    const u32 half = n_k >> 1;
    const u32 i = j & (n_k - 1u), c = j / n_k;
    const bool upper = i >= half;                       // upper half of its block: belongs to L (with a_lo)
    const fe x = fe_from_integer<F>(load_fe256(a + (upper ? i - half : i + half)));
    const fe256 out = fe_to_integer<F>(fe_mul<F>(x, fe_from_table(load_fe256(coef + c))));
    fe256 zero;
#pragma unroll
    for (int w = 0; w < 8; ++w) zero.w[w] = 0;
    fe256 *sl = s + (size_t)(2 * t) * n, *sr = sl + n;
    store_fe256(sl + j, upper ? out : zero);
    store_fe256(sr + j, upper ? zero : out);
}

// The nibble tables of the batch's points -- q_0 .. q_{m-1}, then h -- are built HYB_TAB_CHUNK points at a time by the small-key table
// builder, so point p sits in table p / HYB_TAB_CHUNK as its point p % HYB_TAB_CHUNK:
//   tabs[chunk * HYB_TAB_CHUNK * 960 + (w * 15 + d - 1) * n_chunk + i] = d 16^w P,  n_chunk = the points of that chunk.
static constexpr u32 HYB_TAB_CHUNK = 256;
// k_add_blind_tab over the batch's 2 m results, each with the table of its own proof: out[r] += cq[r] q_{r / 2} (+ hb[r] h when hb is
// given; h is point `hidx`).  BLIND_LANES lanes share a row, as there; cq and hb are canonical integers.
template <int C>
__global__ void __launch_bounds__(64) k_hyb_blind(jacobian256 *__restrict__ out, const fe256 *__restrict__ cq, const fe256 *__restrict__ hb,
                                                 const affine256 *__restrict__ tabs, u32 npts, u32 hidx, u32 nres) {
    latency_critical();
    constexpr u32 PER = SMALL_WINDOWS / BLIND_LANES;           // nibbles per lane: half a 32-bit word
    static_assert(PER == 4, "a lane's nibbles sit in one word of the scalar");
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 r = t / BLIND_LANES, sub = t % BLIND_LANES;
    const bool live = r < nres;
    xyzz acc = xyzz_identity();
#pragma unroll 1
    for (u32 term = 0; term < (hb ? 2u : 1u); ++term) {
        const u32 p = term ? hidx : (live ? r >> 1 : 0u);
        const u32 chunk = p / HYB_TAB_CHUNK, i = p % HYB_TAB_CHUNK;
        const u32 nc = min(HYB_TAB_CHUNK, npts - chunk * HYB_TAB_CHUNK);
        const affine256 *tab = tabs + (size_t)chunk * HYB_TAB_CHUNK * (SMALL_WINDOWS * SMALL_DIGITS) + i;
        const fe256 k = load_fe256((term ? hb : cq) + (live ? r : 0u));
        u32 word = k.w[0];
#pragma unroll
        for (u32 j = 1; j < 8; ++j) word = (sub >> 1) == j ? k.w[j] : word;
        word = live ? (word >> ((sub & 1u) * 16u)) & 0xFFFFu : 0u;
#pragma unroll 1
        for (u32 j = 0; j < PER; ++j) {
            const u32 d = (word >> (4u * j)) & 15u, w = sub * PER + j;
            if (__any(d != 0)) {
                affine pt;
                pt.x = fe_zero(); pt.y = fe_zero();
                if (d) pt = load_table_point(tab + (size_t)(w * SMALL_DIGITS + d - 1) * nc);
                acc = xyzz_madd<C>(acc, pt);                   // the identity (0, 0) adds nothing
            }
        }
    }
#pragma unroll 1
    for (u32 off = BLIND_LANES / 2; off >= 1; off >>= 1)
        acc = xyzz_add<C>(acc, shfl_xyzz(acc, (int)((threadIdx.x & 63u) ^ off)));
    if (live && sub == 0)
        store_jacobian256(out + r, xyzz_to_abi_jacobian<C>(xyzz_add<C>(xyzz_from_abi_jacobian<C>(load_jacobian256(out + r)), acc)));
}

}  // namespace reef
