// Row N6: the vector work of nova-snark's NIFS::prove [R] (Reef: RecursiveSNARK::prove_step, src/backend/framework.rs:668-675)
// over the scalar field of curve C (field F = 1 - C), one folding step at a time:
//
//   AZ, BZ, CZ = A z, B z, C z        for the running z1 = W1 || u1 || X1 and the fresh z2 = W2 || 1 || X2
//   T          = AZ1 o BZ2 + AZ2 o BZ1 - u1 CZ2 - CZ1       (k_nifs_rows_short / k_nifs_rows_long, MODE_T)
//   W, E, u, X = W1 + r W2, E1 + r T, u1 + r, X1 + r X2       (k_nifs_axpy: z1 += r z2 covers W, u and X at once)
//   relaxed    : AZ o BZ == u CZ + E                           (the same row pass, MODE_CHECK)
//
// AZ, BZ and CZ are never written for these: one pass per row computes its dot products and the row's epilogue.  Row N5
// (spartan_kernels.inc) adds two epilogues: MODE_SPARTAN writes AZ, BZ, CZ and D = u CZ + E of the running instance as
// tables, and MODE_ABC runs the same kernels over the column-major copy of the matrices, with eq(r_x) in place of z.
//
// Device form of a matrix (nifs_engine.inc builds it once per shape): CSR row pointers and one 8-byte word per entry,
// {col, class}.  The class says how the entry's coefficient multiplies z[col]:
//   bit 31 set         a general coefficient: side[entry] holds it (internal form), one Montgomery product per entry
//   bit 30 = sign      otherwise: a coefficient of magnitude m = class & 0xffff (m = 1: an addition, else a one-word product)
// Sums of a row are lazy: limb products go into nine 64-bit column accumulators and are reduced once per row (nifs_reduce),
// a negative entry adds 2M - z (BIAS2: every limb stays below 2^32).
//
// Resident vectors (z1, z2, E) hold the internal form, canonical and packed (fe_to_table); T is kept as canonical
// INTEGERS: that is what the MSM of comm_T reads (is_mont = false), and the fold reads it with a pre-scaled r.
//
// The step's two commitments (reef_nifs_commit_step) read one buffer of two rows of max(num_vars, num_cons) canonical integers:
// row 0 is W2, written by k_nifs_import_step in the pass that converts the raw z2, row 1 is T, written by the MODE_T row pass.
// MODE_FRESH is MODE_CHECK on the fresh instance (z2, u = 1, E = 0): AZ2 o BZ2 == CZ2.

namespace reef {

static constexpr u32 NIFS_GENERAL = 1u << 31, NIFS_NEG = 1u << 30, NIFS_MAG = 0xffffu;
static constexpr u32 NIFS_LONG_ROW = 128;        // rows with more entries (A + B + C) go to k_nifs_rows_long, one block each
enum { NIFS_MODE_T = 0, NIFS_MODE_CHECK = 1, NIFS_MODE_SPARTAN = 2, NIFS_MODE_ABC = 3, NIFS_MODE_FRESH = 4 };

struct NifsMat {
    const u32 *rowptr;       // num_cons + 1
    const uint2 *ent;        // {col, class}
    const fe256 *side;       // general coefficients, indexed by entry (internal form)
};
struct NifsArgs {
    NifsMat m[3];            // A, B, C
    const fe256 *z1, *z2;    // num_vars + 1 + num_io each; z[num_vars] = u.  MODE_FRESH: z1 is the fresh z2
    const fe256 *E;          // MODE_CHECK
    fe256 *T;                // MODE_T
    u32 num_cons, num_vars;
    fe256 k254;              // internal form of the integer 2^254 (nifs_reduce)
    u32 *viol, *first_bad;   // MODE_CHECK counters
    const u32 *long_rows;
    u32 nlong;
    fe256 *out[4];           // MODE_SPARTAN: AZ, BZ, CZ, D by row.  MODE_ABC: out[0] by renumbered column
    fe256 r1, r2;            // MODE_ABC: r, r^2 (internal form)
    u32 shift;               // MODE_ABC: a column >= num_vars lands at column + shift (num_vars_pad - num_vars)
};

// Host triples -> device form: the raw coefficient (ABI form or canonical integer) sits in side[e]; this writes ent[e] and,
// for a general coefficient, side[e] in internal form.
template <int F>
__global__ void __launch_bounds__(256) k_nifs_classify(const u32 *__restrict__ cols, u32 nnz, int is_mont, uint2 *__restrict__ ent,
                                                       fe256 *__restrict__ side) {
    const u32 e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nnz) return;
    const fe256 raw = load_fe256(side + e);
    const fe256 v = is_mont ? fe_abi_to_integer<F>(raw) : fe_pack(fe_canon<F>(fe_unpack(raw)));   // canonical integer
    const fe256 n = fe_pack(fe_canon<F>(fe_sub<F, 2>(fe_zero(), fe_unpack(v))));                  // M - v (0 for v = 0)
    bool hi_v = false, hi_n = false;
#pragma unroll
    for (int w = 1; w < 8; ++w) { hi_v |= v.w[w] != 0; hi_n |= n.w[w] != 0; }
    u32 cls;
    if (!hi_v && v.w[0] <= NIFS_MAG) cls = v.w[0];
    else if (!hi_n && n.w[0] <= NIFS_MAG) cls = NIFS_NEG | n.w[0];
    else {
        cls = NIFS_GENERAL;
        store_fe256(side + e, fe_to_table<F>(fe_from_integer<F>(v)));
    }
    ent[e] = make_uint2(cols[e], cls);
}

// The fresh z2 = W2 || 1 || X2 from the caller's W2 and X2 (raw, in the caller's form; they may be the raw entries of z2 itself:
// every thread reads its own element before it writes it) in one pass: z2 in internal form for the row pass, and the canonical
// integers of W2 into w_int (row 0 of the step's commitment rows; its tail beyond num_vars is not touched).
template <int F>
__global__ void __launch_bounds__(256) k_nifs_import_step(const fe256 *w, const fe256 *x, u32 num_vars, u32 nz, int is_mont, fe256 *z2,
                                                          fe256 *__restrict__ w_int) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nz) return;
    if (i == num_vars) { store_fe256(z2 + i, fe_to_table<F>(fe_one<F>())); return; }
    const fe256 raw = load_fe256(i < num_vars ? w + i : x + (i - num_vars - 1));
    store_fe256(z2 + i, fe_to_table<F>(fe_from_caller<F>(raw, is_mont)));
    if (i < num_vars) store_fe256(w_int + i, is_mont ? fe_abi_to_integer<F>(raw) : fe_pack(fe_canon<F>(fe_unpack(raw))));
}
// W (the first num_vars entries of z1) and E of the running instance as canonical integers: the two rows reef_nifs_commit_running
// commits.  The rows' tails are not touched.
template <int F>
__global__ void __launch_bounds__(256) k_nifs_export_running(const fe256 *__restrict__ z1, const fe256 *__restrict__ E, u32 num_vars, u32 num_cons,
                                                             fe256 *__restrict__ w_int, fe256 *__restrict__ e_int) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < num_vars) store_fe256(w_int + i, fe_to_integer<F>(fe_from_table(load_fe256(z1 + i))));
    if (i < num_cons) store_fe256(e_int + i, fe_to_integer<F>(fe_from_table(load_fe256(E + i))));
}

// dst[i] = dst[i] + r * src[i], r pre-scaled so that the product lands in internal form (r R' against an internal src,
// r R'^2 against an integer src)
template <int F>
__global__ void __launch_bounds__(256) k_nifs_axpy(fe256 *__restrict__ dst, const fe256 *__restrict__ src, u32 n, fe256 r) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const fe p = fe_mul<F>(fe_from_table(r), fe_from_table(load_fe256(src + i)));
    store_fe256(dst + i, fe_to_table<F>(fe_add<F>(fe_from_table(load_fe256(dst + i)), p)));
}

// Nine 64-bit column accumulators (value V = sum acc[i] 2^(29 i), every column < 2^63) -> canonical fe congruent to V.
// V = lo + hi 2^254 with lo < 2^254 < M and hi < 2^42: lo + hi * k254, one product.
template <int F> __device__ __forceinline__ fe nifs_reduce(u64 (&acc)[9], const fe &k254) {
    fe lo;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        acc[i + 1] += acc[i] >> LIMB_BITS;
        lo.l[i] = (u32)acc[i] & LIMB_MASK;
    }
    lo.l[8] = (u32)acc[8] & ((1u << 22) - 1u);
    const u64 hi = acc[8] >> 22;
    fe h = fe_zero();
    h.l[0] = (u32)hi & LIMB_MASK;
    h.l[1] = (u32)(hi >> LIMB_BITS);
    REEF_SET_BOUND(lo, 1.0);
    REEF_SET_BOUND(h, 1.0);
    return fe_canon<F>(fe_add<F>(lo, fe_mul<F>(h, k254)));
}

// The dot products of one matrix row with z1 (and z2) over entries b, b + step, ... < e: canonical results.  A thread sees at
// most NIFS_LONG_ROW entries (a long row is cut into segments), each adds < 2^48 to a column: no column reaches 2^63.
template <int F, int TWO>
__device__ __forceinline__ void nifs_dot(const NifsMat &m, u32 b, u32 e, u32 step, const fe256 *__restrict__ z1, const fe256 *__restrict__ z2,
                                         const fe &k254, fe *out) {
    constexpr int NV = TWO ? 2 : 1;
    u64 acc[NV][9];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int i = 0; i < 9; ++i) acc[v][i] = 0;
    for (u32 k = b; k < e; k += step) {
        const uint2 en = m.ent[k];
        fe x[NV];
        x[0] = fe_from_table(load_fe256(z1 + en.x));
        if constexpr (TWO) x[1] = fe_from_table(load_fe256(z2 + en.x));
        if (en.y & NIFS_GENERAL) {
            const fe g = fe_from_table(load_fe256(m.side + k));
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                const fe p = fe_mul<F>(g, x[v]);
#pragma unroll
                for (int i = 0; i < 9; ++i) acc[v][i] += p.l[i];
            }
        } else {
            const u32 mag = en.y & NIFS_MAG;
            const bool neg = (en.y & NIFS_NEG) != 0;
#pragma unroll
            for (int v = 0; v < NV; ++v) {
#pragma unroll
                for (int i = 0; i < 9; ++i) {
                    const u32 t = neg ? FC<F>::BIAS2[i] - x[v].l[i] : x[v].l[i];
                    acc[v][i] += (mag == 1) ? (u64)t : (u64)t * mag;
                }
            }
        }
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) out[v] = nifs_reduce<F>(acc[v], k254);
}

// The row's epilogue on its canonical dot products d: MODE_T d = {AZ1, AZ2, BZ1, BZ2, CZ1, CZ2}, MODE_CHECK, MODE_FRESH and
// MODE_SPARTAN d = {AZ, BZ, CZ}.
template <int F, int MODE>
__device__ __forceinline__ void nifs_epilogue(const NifsArgs &a, u32 row, const fe *d, const fe &u1) {
    if constexpr (MODE == NIFS_MODE_T) {
        const fe m = fe_mul2_add<F>(d[0], d[3], d[1], d[2]);                  // AZ1 BZ2 + AZ2 BZ1, < 2M
        const fe s = fe_add<F>(fe_mul<F>(u1, d[5]), d[4]);                      // u1 CZ2 + CZ1, < 3M
        store_fe256(a.T + row, fe_to_integer<F>(fe_sub<F, 4>(m, s)));
    } else if constexpr (MODE == NIFS_MODE_CHECK) {
        const fe lhs = fe_mul<F>(d[0], d[1]);
        const fe rhs = fe_add<F>(fe_mul<F>(u1, d[2]), fe_from_table(load_fe256(a.E + row)));
        const fe diff = fe_canon<F>(fe_sub<F, 4>(lhs, rhs));
        bool nz = false;
#pragma unroll
        for (int i = 0; i < 9; ++i) nz |= diff.l[i] != 0;
        if (nz) {
            atomicAdd(a.viol, 1u);
            atomicMin(a.first_bad, row);
        }
    } else if constexpr (MODE == NIFS_MODE_FRESH) {
        const fe diff = fe_canon<F>(fe_sub<F, 2>(fe_mul<F>(d[0], d[1]), d[2]));
        bool nz = false;
#pragma unroll
        for (int i = 0; i < 9; ++i) nz |= diff.l[i] != 0;
        if (nz) {
            atomicAdd(a.viol, 1u);
            atomicMin(a.first_bad, row);
        }
    } else if constexpr (MODE == NIFS_MODE_SPARTAN) {
#pragma unroll
        for (int k = 0; k < 3; ++k) store_fe256(a.out[k] + row, fe_pack(d[k]));
        const fe D = fe_add<F>(fe_mul<F>(u1, d[2]), fe_from_table(load_fe256(a.E + row)));
        store_fe256(a.out[3] + row, fe_to_table<F>(D));
    } else {                                 // MODE_ABC: `row` is a column, d = its dot products with eq(r_x) in A, B, C
        const fe v = fe_add<F>(d[0], fe_mul2_add<F>(fe_from_table(a.r1), d[1], fe_from_table(a.r2), d[2]));
        store_fe256(a.out[0] + row + (row >= a.num_vars ? a.shift : 0u), fe_to_table<F>(v));
    }
}
// u of the running instance (MODE_ABC has no z: its `z1` is eq(r_x), and the epilogue takes no u; nor does MODE_FRESH's, u2 = 1)
template <int MODE> __device__ __forceinline__ fe nifs_u1(const NifsArgs &a) {
    return MODE == NIFS_MODE_ABC || MODE == NIFS_MODE_FRESH ? fe_zero() : fe_from_table(load_fe256(a.z1 + a.num_vars));
}

// One thread per row; rows with more than NIFS_LONG_ROW entries are left to k_nifs_rows_long.  The products of A and B are
// taken before the C row is read (fewer live registers than the six dot products of nifs_epilogue).
template <int F, int MODE>
__global__ void __launch_bounds__(256) k_nifs_rows_short(NifsArgs a) {
    const u32 row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= a.num_cons) return;
    u32 b[3], e[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { b[k] = a.m[k].rowptr[row]; e[k] = a.m[k].rowptr[row + 1]; }
    if ((e[0] - b[0]) + (e[1] - b[1]) + (e[2] - b[2]) > NIFS_LONG_ROW) return;
    const fe k254 = fe_from_table(a.k254);
    if constexpr (MODE == NIFS_MODE_T) {
        fe az[2], bz[2], cz[2];
        nifs_dot<F, 1>(a.m[0], b[0], e[0], 1, a.z1, a.z2, k254, az);
        nifs_dot<F, 1>(a.m[1], b[1], e[1], 1, a.z1, a.z2, k254, bz);
        const fe m = fe_mul2_add<F>(az[0], bz[1], az[1], bz[0]);              // AZ1 BZ2 + AZ2 BZ1, < 2M
        nifs_dot<F, 1>(a.m[2], b[2], e[2], 1, a.z1, a.z2, k254, cz);
        const fe u1 = fe_from_table(load_fe256(a.z1 + a.num_vars));
        const fe s = fe_add<F>(fe_mul<F>(u1, cz[1]), cz[0]);                   // u1 CZ2 + CZ1, < 3M
        store_fe256(a.T + row, fe_to_integer<F>(fe_sub<F, 4>(m, s)));
    } else {
        fe d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) nifs_dot<F, 0>(a.m[k], b[k], e[k], 1, a.z1, a.z2, k254, d + k);
        nifs_epilogue<F, MODE>(a, row, d, nifs_u1<MODE>(a));
    }
}

// Long rows are cut into segments of NIFS_SEG entries per matrix, one 256-thread block each (a row of 3 x 10^4 entries is 30
// blocks, not one block walking 117 entries per thread): the block sums its share of the six dot products across the wave
// (shuffles) and the four waves (LDS) and writes them to part[segment]; k_nifs_rows_finish adds a row's segments and runs the
// epilogue.  seg_row[s]: the long row (index into long_rows) of segment s, seg_first[l]: its first segment.
static constexpr u32 NIFS_SEG = 1024;
template <int F>
__device__ __forceinline__ void nifs_wave_sum(fe &v) {
    for (int off = WAVE / 2; off > 0; off >>= 1) {
        fe o;
#pragma unroll
        for (int i = 0; i < 9; ++i) o.l[i] = (u32)__shfl_down((int)v.l[i], off, WAVE);
        REEF_SET_BOUND(o, 1.0);
        v = fe_canon<F>(fe_add<F>(v, o));
    }
}
template <int F, int MODE>
__global__ void __launch_bounds__(256) k_nifs_rows_long(NifsArgs a, const u32 *__restrict__ seg_row, const u32 *__restrict__ seg_first,
                                                        fe_limbs *__restrict__ part) {
    constexpr int TWO = MODE == NIFS_MODE_T, ND = TWO ? 6 : 3;
    __shared__ fe_limbs wsum[4][ND];
    const u32 l = seg_row[blockIdx.x], row = a.long_rows[l], seg = blockIdx.x - seg_first[l];
    const u32 lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const fe k254 = fe_from_table(a.k254);
    fe d[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const u32 b = a.m[k].rowptr[row], e = a.m[k].rowptr[row + 1];
        const u32 sb = min(e, b + seg * NIFS_SEG), se = min(e, sb + NIFS_SEG);
        nifs_dot<F, TWO>(a.m[k], sb + threadIdx.x, se, blockDim.x, a.z1, a.z2, k254, d + (TWO ? 2 * k : k));
    }
#pragma unroll
    for (int j = 0; j < ND; ++j) {
        nifs_wave_sum<F>(d[j]);
        if (lane == 0) wsum[wave][j] = fe_to_limbs(d[j]);
    }
    __syncthreads();
    if (threadIdx.x >= ND) return;
    fe v = fe_from_limbs(wsum[0][threadIdx.x], 1.0);
    for (int w = 1; w < (int)(blockDim.x / WAVE); ++w) v = fe_canon<F>(fe_add<F>(v, fe_from_limbs(wsum[w][threadIdx.x], 1.0)));
    part[(size_t)blockIdx.x * ND + threadIdx.x] = fe_to_limbs(v);
}
// one wave per long row: the segments' partial sums added up, then the row's epilogue
template <int F, int MODE>
__global__ void __launch_bounds__(64) k_nifs_rows_finish(NifsArgs a, const u32 *__restrict__ seg_first, const fe_limbs *__restrict__ part) {
    constexpr int ND = MODE == NIFS_MODE_T ? 6 : 3;
    const u32 l = blockIdx.x, row = a.long_rows[l];
    const u32 s0 = seg_first[l], s1 = seg_first[l + 1];
    fe d[6];
#pragma unroll
    for (int j = 0; j < ND; ++j) {
        d[j] = fe_zero();
        for (u32 s = s0 + threadIdx.x; s < s1; s += WAVE) d[j] = fe_canon<F>(fe_add<F>(d[j], fe_from_limbs(part[(size_t)s * ND + j], 1.0)));
        nifs_wave_sum<F>(d[j]);
    }
    if (threadIdx.x == 0) nifs_epilogue<F, MODE>(a, row, d, nifs_u1<MODE>(a));
}

}  // namespace reef
