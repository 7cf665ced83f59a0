// Row N3: O(N) field passes over the committed document at proof end, as HBM-streaming kernels
// over the scalar field of curve C (field 1-C).
//
//   doc_poly.evaluate(&running_q)                  src/backend/commitment.rs:357
//   hyrax_gen.prove_eval(&doc_poly, .., &running_q, ..)   src/backend/commitment.rs:371-391
//     -> L, R = eq-evaluations of the two halves of the point,  LZ = L^T * Z  (bound rows),
//        eval = <LZ, R>;  the dot-product IPA over LZ then runs on the MSM kernels
//   verifier_mle_eval(table, q')                   src/backend/commitment.rs:236 (r1cs_helper.rs:637-641)
//
// Z is the row-major 2^left x 2^right matrix view of the 2^m-entry table (index = row*2^right + col;
// point[0] pairs with the most significant index bit, as in prover_mle_partial_eval,
// r1cs_helper.rs:577-592).  Entries are either 32-byte field elements or compact unsigned symbols
// (1/2/4 bytes: document symbols are < |alphabet|+3, framework.rs:978-1011).
//
// Forms: 32-byte entries are multiplied as they come (mont(v, L') = v*L with L' in internal form),
// so sums come out in the form they went in (ABI Montgomery or canonical) with no conversion per
// entry; compact symbols give internal-form sums, converted once per output.

namespace reef {

// (fe_limbs / fe_from_limbs: sumcheck_kernels.inc)

struct MlePoint {   // by-value kernel argument: the evaluation point, as handed over (ABI form or canonical)
    fe256 r[28];
};

// eq[t] = prod_k (bit_k(t) ? r_k : 1 - r_k), bit_k = bit (vars-1-k) of t, for the `vars` coordinates
// starting at r[first].  Strictly reduced internal form.
template <int F>
__global__ void __launch_bounds__(256) k_mle_eq(MlePoint pt, u32 first, u32 vars, int is_mont, fe_limbs *__restrict__ eq) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (1u << vars)) return;
    fe acc = fe_one<F>();
    for (u32 k = 0; k < vars; ++k) {
        const fe r = fe_from_caller<F>(pt.r[first + k], is_mont);
        const fe one_minus = fe_sub<F, 2>(fe_one<F>(), r);
        const bool bit = (t >> (vars - 1 - k)) & 1u;
        acc = fe_mul<F>(acc, bit ? r : one_minus);
    }
    const fe c = fe_canon<F>(acc);
    fe_limbs o;
#pragma unroll
    for (int i = 0; i < 9; ++i) o.l[i] = c.l[i];
    eq[t] = o;
}

// k_mle_eq over a batch of points that live in device memory (m x vars, row-major, in the caller's form), written where an MSM reads
// its scalars: w[t * 2^vars + i] = eq(pts[t])_i as a canonical integer.  Grid: x over the entries, y over the points (a stride loop
// past 65535 of them).  The products are k_mle_eq's, in its order.
template <int F>
__global__ void __launch_bounds__(256) k_mle_eq_batch(const fe256 *__restrict__ pts, u32 m, u32 vars, int is_mont, fe256 *__restrict__ w) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (1u << vars)) return;
    for (u32 t = blockIdx.y; t < m; t += gridDim.y) {
        const fe256 *p = pts + (u64)t * vars;
        fe acc = fe_one<F>();
        for (u32 k = 0; k < vars; ++k) {
            const fe r = fe_from_caller<F>(load_fe256(p + k), is_mont);
            const fe one_minus = fe_sub<F, 2>(fe_one<F>(), r);
            const bool bit = (i >> (vars - 1 - k)) & 1u;
            acc = fe_mul<F>(acc, bit ? r : one_minus);
        }
        store_fe256(w + ((u64)t << vars) + i, fe_to_integer<F>(fe_canon<F>(acc)));
    }
}

template <int EB> struct MleElem;
template <> struct MleElem<1> { typedef unsigned char type; };
template <> struct MleElem<2> { typedef unsigned short type; };
template <> struct MleElem<4> { typedef u32 type; };

// (wide_zero / wide_carry: sumcheck_kernels.inc)

// Partial bound rows: thread = column j, blockIdx.y = chunk of rows.  part[chunk][j] =
// sum_{i in chunk} L[i] * Z[i*cols + j], stored packed (canonical).
// Entries with index >= n are zero (the table is zero-padded to 2^m).
template <int F, int EB>
__global__ void __launch_bounds__(256) k_mle_bound(const void *__restrict__ z, u64 n, u32 rows, u32 cols, u32 rows_per_chunk,
                                                   const fe_limbs *__restrict__ Leq, fe256 *__restrict__ part) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cols) return;
    const u32 i0 = blockIdx.y * rows_per_chunk;
    // rows of this column below the zero padding: i*cols + j < n
    const u32 live = j < n ? (u32)((n - j + cols - 1) / cols) : 0u;
    const u32 i1 = min(min(rows, i0 + rows_per_chunk), live);
    fe_wide acc;
    wide_zero(acc);
    if constexpr (EB == 32) {
        const fe256 *zz = (const fe256 *)z;
        fe_wide18 w;
#pragma unroll
        for (int k = 0; k < 18; ++k) w.c[k] = 0;
        // four rows per trip: their loads are issued together (four 32-byte reads in flight per lane), their products share
        // one carry pass (four products of < 2^58 per column fit between carries)
        u32 i = i0;
        for (; i + 4 <= i1; i += 4) {
            const fe256 r0 = load_fe256(zz + (u64)i * cols + j), r1 = load_fe256(zz + (u64)(i + 1) * cols + j);
            const fe256 r2 = load_fe256(zz + (u64)(i + 2) * cols + j), r3 = load_fe256(zz + (u64)(i + 3) * cols + j);
            wide18_mac(w, fe_unpack(r0).l, Leq[i].l);
            wide18_mac(w, fe_unpack(r1).l, Leq[i + 1].l);
            wide18_mac(w, fe_unpack(r2).l, Leq[i + 2].l);
            wide18_mac(w, fe_unpack(r3).l, Leq[i + 3].l);
            wide18_carry(w);
        }
        for (; i < i1; ++i) {                                            // at most three rows: still below the carry bound
            const fe v = fe_unpack(load_fe256(zz + (u64)i * cols + j));   // any 256-bit value
            wide18_mac(w, v.l, Leq[i].l);
        }
        wide18_carry(w);
        const fe s = fe_canon<F>(wide18_reduce<F>(w));
        store_fe256(part + (size_t)blockIdx.y * cols + j, fe_pack(s));
        return;
    } else {
        typedef typename MleElem<EB>::type elem;
        const elem *zz = (const elem *)z;
        u32 since = 0;
#pragma unroll 4
        for (u32 i = i0; i < i1; ++i) {
            const u32 v = zz[(u64)i * cols + j];
            const fe_limbs l = Leq[i];
#pragma unroll
            for (int k = 0; k < 9; ++k) acc.l[k] += (u64)v * l.l[k];
            if (EB == 4 && ++since == 4) {             // 32-bit symbols: 4 products of < 2^61 per column, then carry
                wide_carry(acc);
                since = 0;
            }
        }
    }
    const fe s = fe_canon<F>(fe_from_wide<F>(acc));
    store_fe256(part + (size_t)blockIdx.y * cols + j, fe_pack(s));
}

// lz[j] = sum over chunks (in the output form), and the block's share of <lz, R> as 9 limb sums.
// COMPACT: partial sums are internal form and are converted to the requested output form here.
template <int F, bool COMPACT>
__global__ void __launch_bounds__(256) k_mle_finish(const fe256 *__restrict__ part, u32 chunks, u32 cols, const fe_limbs *__restrict__ Req,
                                                    int is_mont, fe256 *__restrict__ lz, unsigned long long *__restrict__ dot) {
    __shared__ unsigned long long acc[9];
    if (threadIdx.x < 9) acc[threadIdx.x] = 0;
    __syncthreads();
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    fe_wide w;
    wide_zero(w);
    if (j < cols) {
        for (u32 c = 0; c < chunks; ++c) {
            const fe v = fe_from_table(load_fe256(part + (size_t)c * cols + j));
#pragma unroll
            for (int k = 0; k < 9; ++k) w.l[k] += v.l[k];
        }
        fe s;
        if (chunks == 1) {
            s = fe_from_table(load_fe256(part + j));
        } else {
            s = fe_from_wide<F>(w);
        }
        fe256 out;
        if (COMPACT) out = fe_to_caller<F>(s, is_mont);
        else out = fe_pack(fe_canon<F>(s));
        if (lz) store_fe256(lz + j, out);
        const fe p = fe_mul<F>(s, fe_from_limbs(Req[j], 1.0));
#pragma unroll
        for (int k = 0; k < 9; ++k) w.l[k] = p.l[k];
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        unsigned long long a = w.l[k];
        for (int d = 32; d > 0; d >>= 1) a += __shfl_down(a, d, WAVE);
        if ((threadIdx.x & 63) == 0) atomicAdd(&acc[k], a);
    }
    __syncthreads();
    if (threadIdx.x < 9) atomicAdd(&dot[threadIdx.x], acc[threadIdx.x]);
}

// eval = the 9 limb sums folded back, in the output form.
template <int F, bool COMPACT>
__global__ void k_mle_eval_final(unsigned long long *__restrict__ dot, int is_mont, fe256 *__restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    fe_wide w;
#pragma unroll
    for (int k = 0; k < 9; ++k) w.l[k] = dot[k];
    const fe s = fe_from_wide<F>(w);
    fe256 o;
    if (COMPACT) o = fe_to_caller<F>(s, is_mont);
    else o = fe_pack(fe_canon<F>(s));
    store_fe256(out, o);
}

}  // namespace reef
