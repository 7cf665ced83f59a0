// Vectors of scalar-field elements as the rows next to the MSM (N1-N6) hold them, and what every one of them shares:
// the kernels that convert between the caller's form and the resident table form, limb tables, wide accumulators,
// the lazily reduced 18-column products and the wave sums.
//
// Included by kernels_<curve>.hip after msm_kernels.inc (load_fe256 / store_fe256) and before any row's kernels.
#pragma once

namespace reef {

// the caller's form (canonical integers, or pasta Montgomery form when is_mont) -> resident table form (in place allowed)
template <int F>
__global__ void __launch_bounds__(256) k_fe_import(const fe256 *__restrict__ in, u64 n, int is_mont, fe256 *__restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    store_fe256(out + i, fe_to_table<F>(fe_from_caller<F>(load_fe256(in + i), is_mont)));
}
// resident -> the caller's form.  src_is_integer: the source holds canonical integers (the NIFS cross term T, the opening's a)
template <int F>
__global__ void __launch_bounds__(256) k_fe_export(const fe256 *__restrict__ in, u64 n, int src_is_integer, int to_mont, fe256 *__restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const fe256 v = load_fe256(in + i);
    fe256 o = v;                                                       // integers asked of an integer source
    if (!src_is_integer) o = fe_to_caller<F>(fe_from_table(v), to_mont);
    else if (to_mont) o = fe_to_abi<F>(fe_from_integer<F>(v));
    store_fe256(out + i, o);
}

struct fe_limbs { u32 l[9]; };   // internal form, unpacked canonical limbs: tables every lane of a wave reads at the same index (scalar loads)
__device__ __forceinline__ fe fe_from_limbs(const fe_limbs &t, double bound) {
    fe x;
#pragma unroll
    for (int i = 0; i < 9; ++i) x.l[i] = t.l[i];
    REEF_SET_BOUND(x, bound);
    (void)bound;
    return x;
}
__device__ __forceinline__ fe_limbs fe_to_limbs(const fe &canon) {
    fe_limbs o;
#pragma unroll
    for (int i = 0; i < 9; ++i) o.l[i] = canon.l[i];
    return o;
}

// Wide accumulators: 9 limbs of 64 bits in radix 2^29 absorb up to 2^34 normalised elements
// without a carry; fe_from_wide folds them back (9 reduction rounds give w/R', one product with
// R'^2 restores w).
struct fe_wide {
    u64 l[9];
};
__device__ __forceinline__ void wide_zero(fe_wide &w) {
#pragma unroll
    for (int i = 0; i < 9; ++i) w.l[i] = 0;
}
__device__ __forceinline__ void wide_carry(fe_wide &w) {   // keeps the value, brings limbs 0..7 below 2^29
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        w.l[i + 1] += w.l[i] >> LIMB_BITS;
        w.l[i] &= LIMB_MASK;
    }
}
template <int F> __device__ __forceinline__ fe fe_from_wide(const fe_wide &w) {
    u64 t[10];
#pragma unroll
    for (int i = 0; i < 9; ++i) t[i] = w.l[i];
    t[9] = 0;
    // limbs above 2^29 are carried first so that the columns stay far below 2^64
    u64 c = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const u64 v = t[i] + c;
        t[i] = v & LIMB_MASK;
        c = v >> LIMB_BITS;
    }
    // c (< 2^35) is the part above 2^261: fold it back as c * (2^261 mod M) = c * ONE.  With
    // c = c1*2^29 + c0 and the top limb of ONE landing on 2^261 again:
    //   c * ONE = (c0 + c1*ONE[8]) * ONE + c1 * (ONE[0..7] << 29)
    const u32 c0 = (u32)c & LIMB_MASK, c1 = (u32)(c >> LIMB_BITS);
    const u32 m0 = c0 + c1 * FC<F>::ONE[8];
#pragma unroll
    for (int i = 0; i < 9; ++i) t[i] += (u64)m0 * FC<F>::ONE[i];
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i + 1] += (u64)c1 * FC<F>::ONE[i];
    mont_bias(t);
#pragma unroll
    for (int i = 0; i < 9; ++i) mont_round<F>(t);
    fe x = mont_finish<F>(t);
    REEF_SET_BOUND(x, 2.0);
    return fe_mul<F>(x, fe_const<F>(FC<F>::C_R2, 1.0));
}

// The same for limb SUMS of reduced elements (fewer than 2^28 of them: limbs below 2^58, the value below 2^30 M): the quotient
// floor(value / 2^254) is small, so value - q M is one row of products and a conditional addition -- fe_canon with a 64-bit top
// limb -- where fe_from_wide pays nine reduction rounds and a product (~1.2 us of the dependent chain every round ends with).
// value - q M = (value mod 2^254) - q (M - 2^254) lies in (-2^156, 2^254): canonical after adding M to a negative one.
template <int F> __device__ __forceinline__ fe fe_from_limb_sums(const fe_wide &w) {
    u64 t[9], c = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const u64 v = w.l[i] + c;
        t[i] = v & LIMB_MASK;
        c = v >> LIMB_BITS;
    }
    t[8] = w.l[8] + c;
    const u64 q = t[8] >> 22;                                  // < 2^30
    fe r;
    i64 b = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const i64 v = (i64)t[i] - (i64)(q * FC<F>::MOD[i]) + b;
        r.l[i] = (u32)v & LIMB_MASK;
        b = v >> LIMB_BITS;                                    // arithmetic
    }
    const i64 top = (i64)t[8] - (i64)(q * FC<F>::MOD[8]) + b;
    const bool neg = top < 0;
    u32 cc = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const u32 v = r.l[i] + (neg ? FC<F>::MOD[i] : 0u) + cc;
        r.l[i] = v & LIMB_MASK;
        cc = v >> LIMB_BITS;
    }
    r.l[8] = (u32)(top + (neg ? (i64)FC<F>::MOD[8] : 0) + cc);
    REEF_SET_BOUND(r, 1.0);
    return r;
}

// 18-column accumulator of unreduced 9x9-limb products (lazy reduction): a product adds 9 terms of
// < 2^58 to a column, so four products fit between carries; the Montgomery reduction runs once per
// thread instead of once per product.
struct fe_wide18 { u64 c[18]; };
__device__ __forceinline__ void wide18_carry(fe_wide18 &w) {
#pragma unroll
    for (int i = 0; i < 17; ++i) {
        w.c[i + 1] += w.c[i] >> LIMB_BITS;
        w.c[i] &= LIMB_MASK;
    }
}
__device__ __forceinline__ void wide18_zero(fe_wide18 &w) {
#pragma unroll
    for (int k = 0; k < 18; ++k) w.c[k] = 0;
}
__device__ __forceinline__ void wide18_mac(fe_wide18 &w, const u32 (&a)[9], const u32 (&b)[9]) {   // limbs <= 2^29 + 7
#pragma unroll
    for (int i = 0; i < 9; ++i)
#pragma unroll
        for (int j = 0; j < 9; ++j) w.c[i + j] += (u64)a[i] * b[j];
}
// w / R' mod M, exact limbs, value below `bound` M: the bound the caller's w allows (w < 128 M^2, e.g. the Poseidon sums of
// up to five products with operands normalised so that sum (A/M)(B/M) < 128, gives a value < 2 M)
template <int F> __device__ __forceinline__ fe wide18_mont(fe_wide18 &w, double bound) {
    wide18_carry(w);
    u64 t[10];
#pragma unroll
    for (int i = 0; i < 9; ++i) t[i] = w.c[i] + MONT_BIAS;
    t[9] = 0;
#pragma unroll
    for (int r = 0; r < 9; ++r) {
        mont_round<F>(t);
        t[8] += w.c[9 + r];
    }
    fe x = mont_finish<F>(t);
    REEF_SET_BOUND(x, bound);
    (void)bound;
    return x;
}
// w < 34 * 128 * M^2 (e.g. <= 1024 products of a 256-bit value and a reduced one): value < 2 M
template <int F> __device__ __forceinline__ fe wide18_reduce(fe_wide18 &w) {
    return fe_mul<F>(wide18_mont<F>(w, 34.0), fe_one<F>());   // same residue, value < 2 M
}

// Sum over the 64 lanes of a wave, total in lane 63: six DPP additions (quad permutes, row shifts, row broadcasts) instead of six
// ds_bpermute round trips per value -- the nine 64-bit limb sums of a wave cost 2.1 us through shuffles, a fifth of a small round.
// Every lane of the wave must be active.
__device__ __forceinline__ u32 wave_sum63_u32(u32 v) {
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0xb1, 0xf, 0xf, false);    // quad_perm:[1,0,3,2]
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x4e, 0xf, 0xf, false);    // quad_perm:[2,3,0,1]
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xf, 0xf, false);   // row_shr:4
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xf, 0xf, false);   // row_shr:8: lane 15 of a row holds the row's sum
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xf, 0xf, false);   // row_bcast:15
    v += (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xf, 0xf, false);   // row_bcast:31
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum63(unsigned long long v) {   // v < 2^46 in every lane
    const u32 lo = wave_sum63_u32((u32)v & 0xfffffu), hi = wave_sum63_u32((u32)(v >> 20));
    return (unsigned long long)lo + ((unsigned long long)hi << 20);
}

}  // namespace reef
