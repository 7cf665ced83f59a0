// Row N5: the two sum-checks of the final SNARK, nova-snark's RelaxedR1CSSNARK::prove [R] (Reef: S1 / S2,
// src/backend/framework.rs:7-8, CompressedSNARK::prove :695-698), over the scalar field of curve C, on the running relaxed
// instance a NIFS ctx holds (nifs_engine.inc).  spartan_engine.inc drives them, one device call per round:
//
//   begin        AZ, BZ, CZ, D = u CZ + E     (the NIFS row pass, MODE_SPARTAN) and eq(tau)      (k_sp_eq)
//   outer rounds sum eq (AZ BZ - D) at 0, 2, 3 over the low / high halves, fused with the bind of the round before (k_sp_round<F, 1>)
//   outer claims AZ(r_x), BZ(r_x): the last bind; CZ(r_x), E(r_x): dot products with eq(r_x)   (k_sp_bind_last, k_sp_dot)
//   ABC          sum_row eq(r_x)[row] (A + r B + r^2 C)[row][col] per column (the NIFS row pass over the CSC copy, MODE_ABC)
//   inner rounds sum ABC z at 0 and 2                                                              (k_sp_round<F, 0>)
//   inner claims ABC(r_y), z(r_y): the last bind; eval_W = W . eq(r_y[1..])
// and, for the verifier, without a prove (3k): A~, B~, C~ at (r_x, r_y) over the CSR      (k_sp_eq_cols, k_sp_eval_short, k_sp_eval_long)
// and the same at many points in one pass (3o), two points a thread          (k_sp_eq_batch, k_sp_eq_cols_batch, k_sp_*_pair, k_sp_finish_batch)
//
// Tables hold the resident internal form, canonical and packed (fe_to_table), like the NIFS vectors.  Round sums are lazy: each
// term is one product (< 2M, exact 29-bit limbs) whose limbs go into 64-bit column sums per thread, then per wave (DPP), per block
// (LDS) into partial[block][27]; k_sp_finish adds the blocks' sums and reduces them once (fe_from_limb_sums) -- a second launch,
// no grid hand-over inside the round kernel.

namespace reef {

static constexpr u32 SP_BLOCKS = 1024;   // round and dot kernels: at most this many blocks, so a thread adds <= 2^23 / 2^18 terms
static constexpr u32 SP_THREADS = 256;

// eq(p)[i] = prod_j (bit_{ell-1-j}(i) ? p_j : 1 - p_j) (p_0 pairs with the most significant bit, as EqPolynomial::evals [R]).
// f[2 j] = 1 - p_j, f[2 j + 1] = p_j (internal form); one thread per entry, ell - 1 products.
template <int F> __device__ __forceinline__ fe256 sp_eq_at(const fe256 *__restrict__ f, u32 ell, u32 i) {
    fe acc = fe_from_table(load_fe256(f + ((i >> (ell - 1)) & 1u)));
    for (u32 j = 1; j < ell; ++j) acc = fe_mul<F>(acc, fe_from_table(load_fe256(f + 2 * j + ((i >> (ell - 1 - j)) & 1u))));
    return fe_to_table<F>(acc);
}
template <int F>
__global__ void __launch_bounds__(256) k_sp_eq(const fe256 *__restrict__ f, u32 ell, u32 n, fe256 *__restrict__ out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    store_fe256(out + i, sp_eq_at<F>(f, ell, i));
}
// out[c] = eq(p)[c'] for the n matrix columns in their own numbering, c' = renumber(c) of R1CSShape::pad [R]: c' = c for c < num_vars,
// c + shift otherwise (c' < 2^ell is the caller's pad rule).  The column weights of k_sp_eval_short: a row gathers out + col, no shift.
template <int F>
__global__ void __launch_bounds__(256) k_sp_eq_cols(const fe256 *__restrict__ f, u32 ell, u32 n, u32 num_vars, u32 shift, fe256 *__restrict__ out) {
    const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n) return;
    store_fe256(out + c, sp_eq_at<F>(f, ell, c + (c >= num_vars ? shift : 0u)));
}

// the value at t of the line through lo (t = 0) and hi (t = 1), canonical: lo + t (hi - lo) for t = 2, 3
template <int F> __device__ __forceinline__ void sp_line(const fe &lo, const fe &hi, fe &v2, fe &v3) {
    const fe d = fe_sub<F, 2>(hi, lo);                         // < 3M
    v2 = fe_canon<F>(fe_add<F>(hi, d));
    v3 = fe_canon<F>(fe_add<F>(v2, d));
}
// X[b] + r (X[b + off] - X[b]), canonical
template <int F> __device__ __forceinline__ fe sp_bind(const fe256 *X, u32 b, u32 off, const fe &r) {
    const fe a0 = fe_from_table(load_fe256(X + b)), a1 = fe_from_table(load_fe256(X + b + off));
    return fe_canon<F>(fe_add<F>(a0, fe_mul<F>(r, fe_sub<F, 2>(a1, a0))));
}
__device__ __forceinline__ void sp_acc(u64 (&acc)[9], const fe &x) {   // x: exact 29-bit limbs
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[i] += x.l[i];
}

// The limb sums of NV values per thread -> partial[blockIdx.x][27] (slots 9 k .. 9 k + 8 for value k).  Every thread of the block
// calls it (the DPP sums need whole waves); a thread's column sums stay below 2^46.
template <int NV> __device__ __forceinline__ void sp_block_sums(u64 (&acc)[NV][9], unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long bs[27];
    if (threadIdx.x < 27) bs[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const unsigned long long s = wave_sum63(acc[k][i]);
            if ((threadIdx.x & 63) == 63) atomicAdd(&bs[9 * k + i], s);
        }
    __syncthreads();
    if (threadIdx.x < 27) partial[(size_t)blockIdx.x * 27 + threadIdx.x] = bs[threadIdx.x];
}

struct SpRound {
    fe256 *t[4];             // cubic: eq, AZ, BZ, D.  quadratic: ABC, z
    u32 h;                   // pairs (b, b + h) summed this round: the tables hold 2h entries after the bind
    int bind;                // bind with r first: the tables hold 4h entries before it, (b, b + 2h) -> b
    fe256 r;                 // internal form
    unsigned long long *partial;
};
// One round: the bind of the round before (if any) fused with this round's sums, one pass over the tables.  Thread b < h binds the
// entries b and b + h of every table (their partners at + 2h), writes them, and uses them as the pair (lo, hi) of this round:
//   cubic      e0 = sum eq AZ BZ - eq D at lo,   e2, e3: the same at lo + t (hi - lo) for t = 2, 3   (prove_cubic_with_additive_term)
//   quadratic  e0 = sum ABC z at lo,             e2: at t = 2                                        (prove_quad)
// A thread reads b, b + h, b + 2h, b + 3h and writes b, b + h only: binding in place is safe.
template <int F, int CUBIC>
__global__ void __launch_bounds__(SP_THREADS) k_sp_round(SpRound a) {
    constexpr int NT = CUBIC ? 4 : 2, NV = CUBIC ? 3 : 2;
    const fe r = fe_from_table(a.r);
    u64 acc[NV][9];
#pragma unroll
    for (int k = 0; k < NV; ++k)
#pragma unroll
        for (int i = 0; i < 9; ++i) acc[k][i] = 0;
    for (u32 b = blockIdx.x * blockDim.x + threadIdx.x; b < a.h; b += gridDim.x * blockDim.x) {
        fe lo[NT], hi[NT];
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            if (a.bind) {
                lo[k] = sp_bind<F>(a.t[k], b, 2 * a.h, r);
                hi[k] = sp_bind<F>(a.t[k], b + a.h, 2 * a.h, r);
                store_fe256(a.t[k] + b, fe_pack(lo[k]));
                store_fe256(a.t[k] + b + a.h, fe_pack(hi[k]));
            } else {
                lo[k] = fe_from_table(load_fe256(a.t[k] + b));
                hi[k] = fe_from_table(load_fe256(a.t[k] + b + a.h));
            }
        }
        if constexpr (CUBIC) {
            fe v2[4], v3[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) sp_line<F>(lo[k], hi[k], v2[k], v3[k]);
            // eq (AZ BZ + 2M - D): fe_mul_sub < 4M, times eq < M
            sp_acc(acc[0], fe_mul<F>(lo[0], fe_mul_sub<F, 2>(lo[1], lo[2], lo[3])));
            sp_acc(acc[1], fe_mul<F>(v2[0], fe_mul_sub<F, 2>(v2[1], v2[2], v2[3])));
            sp_acc(acc[2], fe_mul<F>(v3[0], fe_mul_sub<F, 2>(v3[1], v3[2], v3[3])));
        } else {
            fe a2, a3, z2, z3;
            sp_line<F>(lo[0], hi[0], a2, a3);
            sp_line<F>(lo[1], hi[1], z2, z3);
            sp_acc(acc[0], fe_mul<F>(lo[0], lo[1]));
            sp_acc(acc[1], fe_mul<F>(a2, z2));
        }
    }
    sp_block_sums<NV>(acc, a.partial);
}

// Dot products x . y0 (and x . y1) over n entries -> partial[block][27]
template <int F>
__global__ void __launch_bounds__(SP_THREADS) k_sp_dot(const fe256 *__restrict__ x, const fe256 *__restrict__ y0, const fe256 *__restrict__ y1,
                                                       u32 n, unsigned long long *__restrict__ partial) {
    u64 acc[2][9];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int i = 0; i < 9; ++i) acc[k][i] = 0;
    for (u32 b = blockIdx.x * blockDim.x + threadIdx.x; b < n; b += gridDim.x * blockDim.x) {
        const fe xv = fe_from_table(load_fe256(x + b));
        sp_acc(acc[0], fe_mul<F>(xv, fe_from_table(load_fe256(y0 + b))));
        if (y1) sp_acc(acc[1], fe_mul<F>(xv, fe_from_table(load_fe256(y1 + b))));
    }
    sp_block_sums<2>(acc, partial);
}

// a canonical internal value in the caller's form: 0 the internal table form, 1 canonical integer, 2 pasta Montgomery form
enum { SP_FORM_TABLE = 0, SP_FORM_INTEGER = 1, SP_FORM_MONT = 2 };
template <int F> __device__ __forceinline__ fe256 sp_out(const fe &x, int form) {
    return form == SP_FORM_TABLE ? fe_to_table<F>(x) : fe_to_caller<F>(x, form == SP_FORM_MONT);
}

// out[k] = the sum over nblocks blocks of value k (k < nv), in `form`.  One block: every thread adds its blocks' 9 nv slots, LDS
// atomics add the threads; value k's limb sums (< 2^24 terms of < 2^29 each) are reduced once.
template <int F>
__device__ __forceinline__ void sp_finish_body(const unsigned long long *__restrict__ partial, u32 nblocks, u32 nv, int form, fe256 *__restrict__ out) {
    __shared__ unsigned long long tot[27];
    if (threadIdx.x < 27) tot[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long s[27];
#pragma unroll
    for (int i = 0; i < 27; ++i) s[i] = 0;
    for (u32 b = threadIdx.x; b < nblocks; b += blockDim.x)
#pragma unroll
        for (int i = 0; i < 27; ++i)
            if (i < (int)(9 * nv)) s[i] += partial[(size_t)b * 27 + i];
#pragma unroll
    for (int i = 0; i < 27; ++i)
        if (s[i]) atomicAdd(&tot[i], s[i]);
    __syncthreads();
    if (threadIdx.x >= nv) return;
    fe_wide w;
#pragma unroll
    for (int i = 0; i < 9; ++i) w.l[i] = tot[9 * threadIdx.x + i];
    store_fe256(out + threadIdx.x, sp_out<F>(fe_from_limb_sums<F>(w), form));
}
template <int F>
__global__ void __launch_bounds__(SP_THREADS) k_sp_finish(const unsigned long long *__restrict__ partial, u32 nblocks, u32 nv, int form,
                                                          fe256 *__restrict__ out) {
    sp_finish_body<F>(partial, nblocks, nv, form, out);
}

// The last bind (two entries left): t[k][0] = t[k][0] + r (t[k][1] - t[k][0]) for k < nt, and out[k] = that value in `form`
template <int F>
__global__ void __launch_bounds__(64) k_sp_bind_last(SpRound a, u32 nt, int form, fe256 *__restrict__ out) {
    const u32 k = threadIdx.x;
    if (k >= nt) return;
    const fe v = sp_bind<F>(a.t[k], 0, 1, fe_from_table(a.r));
    store_fe256(a.t[k], fe_pack(v));
    store_fe256(out + k, sp_out<F>(v, form));
}

// ---- the verifier's matrix evaluations (include/reef_msm.h 3k): M~(r_x, r_y) = sum_entries val eq(r_x)[row] eq(r_y)[col'] for M = A, B, C.
// One product per ENTRY goes into the row's dot product with the column weights zy (k_sp_eq_cols) -- nifs_dot, with its +-1 adds and
// one-word magnitudes -- then three products per ROW with ex = eq(r_x)[row], whose limbs are summed over the rows as the round sums
// are: per wave, per block into partial[block][27], once over the blocks by k_sp_finish.  No per-row table is written.
// a: the CSR (m, num_cons, long_rows, k254) with z1 = z2 = zy.  One thread per row; a row of more than NIFS_LONG_ROW entries, a row
// past num_cons and an empty row add zero HERE and stay in the block: sp_block_sums needs whole waves and has two barriers, so no
// thread returns before it.
// Bound: at most 2^24 rows (the pad rule), long rows included, each adding one product with limbs < 2^29 to a value's nine columns:
// a block's column < 2^37, the columns k_sp_finish adds up < 2^53, inside its stated bound (< 2^24 terms of < 2^29 each).
template <int F>
__global__ void __launch_bounds__(SP_THREADS) k_sp_eval_short(NifsArgs a, const fe256 *__restrict__ ex, unsigned long long *__restrict__ partial) {
    const u32 row = blockIdx.x * blockDim.x + threadIdx.x;
    u64 acc[3][9];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int i = 0; i < 9; ++i) acc[k][i] = 0;
    u32 b[3] = {0, 0, 0}, e[3] = {0, 0, 0};
    if (row < a.num_cons) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { b[k] = a.m[k].rowptr[row]; e[k] = a.m[k].rowptr[row + 1]; }
    }
    const u32 len = (e[0] - b[0]) + (e[1] - b[1]) + (e[2] - b[2]);
    if (len != 0 && len <= NIFS_LONG_ROW) {                 // a predicate, not a return
        const fe k254 = fe_from_table(a.k254);
        const fe w = fe_from_table(load_fe256(ex + row));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            fe d;
            nifs_dot<F, 0>(a.m[k], b[k], e[k], 1, a.z1, a.z2, k254, &d);
            sp_acc(acc[k], fe_mul<F>(w, d));
        }
    }
    sp_block_sums<3>(acc, partial);
}
// One wave per long row, after k_nifs_rows_long left its segments' sums in part: the row's three dot products, times eq(r_x)[row], as
// one more row of partial (lane 0 writes all 27 slots): rows[l] of `partial` here is the caller's row (blocks of k_sp_eval_short) + l.
template <int F>
__global__ void __launch_bounds__(64) k_sp_eval_long(NifsArgs a, const u32 *__restrict__ seg_first, const fe_limbs *__restrict__ part,
                                                     const fe256 *__restrict__ ex, unsigned long long *__restrict__ partial) {
    const u32 l = blockIdx.x, row = a.long_rows[l];
    const u32 s0 = seg_first[l], s1 = seg_first[l + 1];
    fe d[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        d[j] = fe_zero();
        for (u32 s = s0 + threadIdx.x; s < s1; s += WAVE) d[j] = fe_canon<F>(fe_add<F>(d[j], fe_from_limbs(part[(size_t)s * 3 + j], 1.0)));
        nifs_wave_sum<F>(d[j]);
    }
    if (threadIdx.x != 0) return;
    const fe w = fe_from_table(load_fe256(ex + row));
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const fe p = fe_mul<F>(w, d[k]);
#pragma unroll
        for (int i = 0; i < 9; ++i) partial[(size_t)l * 27 + 9 * k + i] = p.l[i];
    }
}

// ---- the same at many points in one pass (include/reef_msm.h 3o).  A group of npts points has plain tables per point -- ex[t][row],
// zy[t][col], partial[t][rows][27] -- and is walked two points a thread: pair q = blockIdx.y holds the points 2q and 2q + 1, and every
// CSR entry, its class and its general coefficient are read once for both (nifs_dot<F, 1>, as a folding step reads them for z1 and
// z2).  An odd last point is a pair with t1 = t0: the row kernels walk it with one vector (nifs_dot<F, 0>, a branch on blockIdx alone),
// so it costs what the single call's row pass costs, and nothing is written for a second point.  Entries of the tables and every sum
// are what the single call forms for the point alone: the results are bit-identical.  The launches of a group do not depend on npts.
struct SpBatch {
    const fe256 *f;              // eq factors of point t at f + t fstride: r_x's 2 ell_x, then r_y's 2 ell_y
    fe256 *ex, *zy;              // ex + t num_cons, zy + t nz
    unsigned long long *partial; // partial + t rows 27: a row per block of the row pass, then a row per long row
    fe_limbs *part;              // the long rows' segment sums of pair q at part + q nseg 6 (k_nifs_rows_long's MODE_T layout)
    u32 npts, fstride, ell_x, ell_y, nz, rows, nseg;
};
__device__ __forceinline__ u32 sp_pair_second(const SpBatch &g, u32 t0) { return t0 + 1 < g.npts ? t0 + 1 : t0; }

// k_sp_eq and k_sp_eq_cols with the point in blockIdx.y (as k_mle_eq_batch beside k_mle_eq): the same sp_eq_at per entry
template <int F>
__global__ void __launch_bounds__(256) k_sp_eq_batch(SpBatch g, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (i >= n) return;
    store_fe256(g.ex + (size_t)t * n + i, sp_eq_at<F>(g.f + (size_t)t * g.fstride, g.ell_x, i));
}
template <int F>
__global__ void __launch_bounds__(256) k_sp_eq_cols_batch(SpBatch g, u32 num_vars, u32 shift) {
    const u32 c = blockIdx.x * blockDim.x + threadIdx.x, t = blockIdx.y;
    if (c >= g.nz) return;
    store_fe256(g.zy + (size_t)t * g.nz + c, sp_eq_at<F>(g.f + (size_t)t * g.fstride + 2 * g.ell_x, g.ell_y, c + (c >= num_vars ? shift : 0u)));
}

// k_sp_eval_short for the pair blockIdx.y: a row's three dot products with BOTH column tables from one walk over its entries, then the
// six products with the pair's two ex[row], summed per point as sp_block_sums does.  The predicate-not-return rule holds as there; the
// branch around the second block sum is on blockIdx alone, so whole blocks take it.
// Bound, per point: as k_sp_eval_short's -- a thread adds one product (limbs < 2^29) to each of the point's 27 columns.
template <int F>
__global__ void __launch_bounds__(SP_THREADS) k_sp_eval_short_pair(NifsArgs a, SpBatch g) {
    const u32 row = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 t0 = 2 * blockIdx.y, t1 = sp_pair_second(g, t0);
    u64 acc[2][3][9];
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int i = 0; i < 9; ++i) acc[v][k][i] = 0;
    u32 b[3] = {0, 0, 0}, e[3] = {0, 0, 0};
    if (row < a.num_cons) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { b[k] = a.m[k].rowptr[row]; e[k] = a.m[k].rowptr[row + 1]; }
    }
    const u32 len = (e[0] - b[0]) + (e[1] - b[1]) + (e[2] - b[2]);
    if (len != 0 && len <= NIFS_LONG_ROW) {                 // a predicate, not a return
        const fe k254 = fe_from_table(a.k254);
        const fe256 *z1 = g.zy + (size_t)t0 * g.nz, *z2 = g.zy + (size_t)t1 * g.nz;
        const fe w0 = fe_from_table(load_fe256(g.ex + (size_t)t0 * a.num_cons + row));
        const fe w1 = fe_from_table(load_fe256(g.ex + (size_t)t1 * a.num_cons + row));
        if (t1 != t0) {                                     // on blockIdx alone: whole blocks go one way
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                fe d[2];
                nifs_dot<F, 1>(a.m[k], b[k], e[k], 1, z1, z2, k254, d);
                sp_acc(acc[0][k], fe_mul<F>(w0, d[0]));
                sp_acc(acc[1][k], fe_mul<F>(w1, d[1]));
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                fe d;
                nifs_dot<F, 0>(a.m[k], b[k], e[k], 1, z1, z1, k254, &d);
                sp_acc(acc[0][k], fe_mul<F>(w0, d));
            }
        }
    }
    sp_block_sums<3>(acc[0], g.partial + (size_t)t0 * g.rows * 27);
    if (t1 != t0) sp_block_sums<3>(acc[1], g.partial + (size_t)t1 * g.rows * 27);
}
// The long rows' segment pass for the pair blockIdx.y: k_nifs_rows_long<F, NIFS_MODE_T> on the pair's column tables, six sums a segment
// (d[2 k + v]: matrix k, point v) into the pair's own slice of part.  Its text is that kernel's, not a body shared with it: behind a shared
// __device__ function k_nifs_rows_long compiled to ten more SGPRs, and it is a kernel of every folding step.
template <int F>
__global__ void __launch_bounds__(256) k_sp_rows_long_pair(NifsArgs a, const u32 *__restrict__ seg_row, const u32 *__restrict__ seg_first, SpBatch g) {
    __shared__ fe_limbs wsum[4][6];
    const u32 t0 = 2 * blockIdx.y, t1 = sp_pair_second(g, t0);
    const fe256 *z1 = g.zy + (size_t)t0 * g.nz, *z2 = g.zy + (size_t)t1 * g.nz;
    fe_limbs *part = g.part + (size_t)blockIdx.y * g.nseg * 6;
    const u32 l = seg_row[blockIdx.x], row = a.long_rows[l], seg = blockIdx.x - seg_first[l];
    const u32 lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const fe k254 = fe_from_table(a.k254);
    fe d[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const u32 b = a.m[k].rowptr[row], e = a.m[k].rowptr[row + 1];
        const u32 sb = min(e, b + seg * NIFS_SEG), se = min(e, sb + NIFS_SEG);
        if (t1 != t0) nifs_dot<F, 1>(a.m[k], sb + threadIdx.x, se, blockDim.x, z1, z2, k254, d + 2 * k);
        else {                                              // the odd last point: one vector, its twin's sums are zero and are not read
            nifs_dot<F, 0>(a.m[k], sb + threadIdx.x, se, blockDim.x, z1, z1, k254, d + 2 * k);
            d[2 * k + 1] = fe_zero();
        }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        nifs_wave_sum<F>(d[j]);
        if (lane == 0) wsum[wave][j] = fe_to_limbs(d[j]);
    }
    __syncthreads();
    if (threadIdx.x >= 6) return;
    fe v = fe_from_limbs(wsum[0][threadIdx.x], 1.0);
    for (int w = 1; w < (int)(blockDim.x / WAVE); ++w) v = fe_canon<F>(fe_add<F>(v, fe_from_limbs(wsum[w][threadIdx.x], 1.0)));
    part[(size_t)blockIdx.x * 6 + threadIdx.x] = fe_to_limbs(v);
}
// k_sp_eval_long for the pair blockIdx.y: the six sums of long row l (d[2 k + v]: matrix k, point v of the pair), times each point's
// eq(r_x)[row], as row (rows - nlong) + l of each point's partial
template <int F>
__global__ void __launch_bounds__(64) k_sp_eval_long_pair(NifsArgs a, const u32 *__restrict__ seg_first, SpBatch g) {
    const u32 l = blockIdx.x, row = a.long_rows[l];
    const u32 t0 = 2 * blockIdx.y, t1 = sp_pair_second(g, t0);
    const u32 s0 = seg_first[l], s1 = seg_first[l + 1];
    const fe_limbs *part = g.part + (size_t)blockIdx.y * g.nseg * 6;
    fe d[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
        d[j] = fe_zero();
        for (u32 s = s0 + threadIdx.x; s < s1; s += WAVE) d[j] = fe_canon<F>(fe_add<F>(d[j], fe_from_limbs(part[(size_t)s * 6 + j], 1.0)));
        nifs_wave_sum<F>(d[j]);
    }
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int v = 0; v < 2; ++v) {
        const u32 t = v ? t1 : t0;
        if (v && t1 == t0) continue;
        const fe w = fe_from_table(load_fe256(g.ex + (size_t)t * a.num_cons + row));
        unsigned long long *dst = g.partial + ((size_t)t * g.rows + (g.rows - a.nlong) + l) * 27;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const fe p = fe_mul<F>(w, d[2 * k + v]);
#pragma unroll
            for (int i = 0; i < 9; ++i) dst[9 * k + i] = p.l[i];
        }
    }
}
// k_sp_finish with one block per point of the group: out[3 t ..] = the three sums of point t's partial, in `form`
template <int F>
__global__ void __launch_bounds__(SP_THREADS) k_sp_finish_batch(const unsigned long long *__restrict__ partial, u32 rows, int form, fe256 *__restrict__ out) {
    sp_finish_body<F>(partial + (size_t)blockIdx.x * rows * 27, rows, 3u, form, out + 3 * (size_t)blockIdx.x);
}

}  // namespace reef
