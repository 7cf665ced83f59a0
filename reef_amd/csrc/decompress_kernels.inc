// Row a9, the way back: 32-byte point encodings -> affine points (include/reef_msm.h: reef_decompress), the inverse of
// affine_compress (ec.h).  Reef keeps a document commitment as PolyCommit.comm: Vec<CompressedCommitment>
// (src/backend/commitment.rs:60,187-197) and decompresses every row where it needs the point (:192-197; HyraxPC::prove_eval [R]).
//
// The decoding rule is pasta_curves' from_bytes [R] (oracle/pasta_oracle.py: Curve.decompress): 32 zero bytes are the identity;
// otherwise bit 255 is the parity of y and the low 255 bits are x, little-endian; x >= p is invalid; y^2 = x^3 + 5, a non-residue
// is invalid; y is the root whose canonical integer has that parity.  One thread per encoding, over the BASE field of curve C.
//
// The square root is the cost.  M - 1 = 2^32 T, and among random curve points t = (y^2)^T has order 2^30 or more for seven in
// eight: Tonelli-Shanks (keygen_kernels.inc: fe_sqrt) runs near its worst case, ~32^2/2 squarings after the 222-bit power, with
// loop lengths that depend on the data, so a wave pays the maximum over its lanes.  fe_sqrt_windowed does the same power and then
// takes the discrete logarithm of t in the 2^32 subgroup four bits at a time from tables (field_consts.h: SQ_TAB, SQ_TOP): 120
// squarings and 15 products whatever the input.  Both roots give the same bytes; which one ships: DESIGN.md 7j.
//
// Included by kernels_<curve>.hip after keygen_kernels.inc.  The part above the kernels is plain C++ as well (csrc/tools/sqrt_check.cpp).
#if defined(__HIPCC__)
#define REEF_DC __device__ __forceinline__
#else
#define REEF_DC inline
#endif
namespace reef {

static constexpr u32 SQ_TAB_WORDS = 128 * 9;

template <int F> REEF_DC bool fe_same(const fe &a, const fe &b) { return fe_is_zero<F>(fe_sub<F, 4>(a, b)); }   // a, b < 4
template <int F> REEF_DC u32 fe_parity(const fe &x) { return fe_to_integer<F>(x).w[0] & 1u; }                  // of the canonical integer
// x^((T - 1)/2), the 222-bit power both roots start from
template <int F> REEF_DC fe fe_pow_half_t(const fe &x) {
    fe acc = fe_one<F>();
    for (int i = 221; i >= 0; --i) {
        acc = fe_sqr<F>(acc);
        if ((FC<F>::TS_EXP[i >> 5] >> (i & 31)) & 1u) acc = fe_mul<F>(acc, x);
    }
    return acc;
}

// Square root without a data-dependent trip count: true and a root, or false for a non-residue (root is then meaningless).  x < 2.
// With w = x^((T-1)/2): y = x w has y^2 = x t, t = x^T = zeta^e in the 2^32 subgroup (zeta = TS_ROOT), and x is a square iff e is
// even; the root is y zeta^(-e/2).  e = sum_j e_j 16^j, lowest digit first: t^(2^(28 - 4j)) = (zeta^(2^28))^(e_j) once the digits
// below j are gone, recognised by its low limb (SQ_TOP); b = tab[16 j + e_j] = zeta^-(e_j 16^j / 2) goes into y, b^2 takes the digit
// out of t.  An odd e_0 leaves t outside the table's reach and y^2 != x at the end: that comparison is the residue test.
// tab: SQ_TAB of the field, SQ_TAB_WORDS words (a kernel's copy in LDS: the digits differ from lane to lane).
template <int F> REEF_DC bool fe_sqrt_windowed(const fe &x, const u32 *tab, fe &root) {
    const fe w = fe_pow_half_t<F>(x);
    fe y = fe_mul<F>(x, w), t = fe_mul<F>(y, w);
    for (int j = 0; j < 8; ++j) {
        fe v = t;
#pragma unroll 1
        for (int s = 0; s < 28 - 4 * j; ++s) v = fe_sqr<F>(v);
        const u32 low = fe_canon<F>(v).l[0];
        u32 k = 0;
#pragma unroll
        for (u32 i = 1; i < 16; ++i) k = low == FC<F>::SQ_TOP[i] ? i : k;
        fe b;
#pragma unroll
        for (int i = 0; i < 9; ++i) b.l[i] = tab[(16 * j + k) * 9 + i];
        REEF_SET_BOUND(b, 1.0);
        y = fe_mul<F>(y, b);
        if (j < 7) t = fe_mul<F>(t, fe_sqr<F>(b));
    }
    root = y;
    return fe_same<F>(fe_sqr<F>(y), x);
}

// the root that ships / the other one (W = false: Tonelli-Shanks, device code only)
template <int F, bool W> REEF_DC bool fe_sqrt_by(const fe &x, const u32 *tab, fe &root) {
    if constexpr (W) return fe_sqrt_windowed<F>(x, tab, root);
#if defined(__HIPCC__)
    else return fe_sqrt<F>(x, root);
#else
    else return false;
#endif
}
// the root of x whose canonical integer is even
template <int F, bool W> REEF_DC bool fe_sqrt_even(const fe &x, const u32 *tab, fe &root) {
    fe y;
    const bool ok = fe_sqrt_by<F, W>(x, tab, y);
    root = fe_parity<F>(y) ? fe_mul<F>(fe_neg<F, 2>(y), fe_one<F>()) : y;
    return ok;
}

// One encoding -> the ABI affine point; false (and (0, 0)) for an invalid one.
template <int C, bool W> REEF_DC bool point_decompress(const fe256 &enc, const u32 *tab, affine256 &out) {
    u32 any = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) { any |= enc.w[i]; out.x.w[i] = 0; out.y.w[i] = 0; }
    if (any == 0) return true;                                   // the identity
    fe256 xi = enc;
    const u32 sign = xi.w[7] >> 31;
    xi.w[7] &= 0x7fffffffu;
    const fe xs = fe_unpack(xi), xc = fe_canon<C>(xs);           // strict limbs, below 2^255 < 2 M: equal iff x < M
    u32 d = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) d |= xs.l[i] ^ xc.l[i];
    if (d) return false;
    const fe x = fe_from_integer<C>(xi), one = fe_one<C>();
    fe256 five_i = {};
    five_i.w[0] = 5;
    const fe y2 = fe_mul<C>(fe_add<C>(fe_mul<C>(fe_sqr<C>(x), x), fe_from_integer<C>(five_i)), one);   // x^3 + 5 < 2
    fe y;
    if (!fe_sqrt_even<C, W>(y2, tab, y)) return false;
    if (sign) y = fe_mul<C>(fe_neg<C, 2>(y), one);               // y = 0 has no odd form, and no point of these curves has y = 0
    affine a;
    a.x = x;
    a.y = y;
    out = affine_to_abi<C>(a);
    return true;
}

#if defined(__HIPCC__)
__device__ __forceinline__ void sq_tab_to_lds(const u32 *src, u32 *tab) {
    for (u32 i = threadIdx.x; i < SQ_TAB_WORDS; i += blockDim.x) tab[i] = src[i];
    __syncthreads();
}

// stats[0] += invalid encodings, stats[1] = min(their indices) (the host sets it to n).  One wave per workgroup: 2^13 encodings
// are 128 waves on 1024 SIMDs, and a wave alone on its SIMD runs the chain fastest.
template <int C, bool W>
__global__ void __launch_bounds__(64) k_decompress(const fe256 *__restrict__ in, u32 n, affine256 *__restrict__ out,
                                                   unsigned long long *__restrict__ stats) {
    __shared__ u32 tab[SQ_TAB_WORDS];
    if (W) sq_tab_to_lds(&FC<C>::SQ_TAB[0][0], tab);
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    affine256 p;
    if (!point_decompress<C, W>(load_fe256(in + i), tab, p)) {
        atomicAdd(stats, 1ull);
        atomicMin(stats + 1, (unsigned long long)i);
    }
    store_affine256(out + i, p);
}

// reef_test_field_op 8 (W = true) and 9: out = the even root of a, ABI form in and out; 32 bytes of 0xff for a non-residue
template <int F, bool W> __global__ void __launch_bounds__(64) k_test_sqrt(const fe256 *a, fe256 *out, u32 n) {
    __shared__ u32 tab[SQ_TAB_WORDS];
    if (W) sq_tab_to_lds(&FC<F>::SQ_TAB[0][0], tab);
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe y;
    fe256 r;
    if (fe_sqrt_even<F, W>(fe_from_abi<F>(load_fe256(a + i)), tab, y)) r = fe_to_abi<F>(y);
    else {
#pragma unroll
        for (int k = 0; k < 8; ++k) r.w[k] = 0xffffffffu;
    }
    store_fe256(out + i, r);
}
#endif

}  // namespace reef
