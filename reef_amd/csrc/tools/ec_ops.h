// The raw-limb forms of ec.h's routines that tools/ec_check.hip (gfx950, release flags) and tools/host_check.cpp (the host,
// REEF_BOUNDS) both expose, written once so that the two harnesses run the same compositions.  TEST HARNESS ONLY.
//
// Data forms: an XYZZ point is 36 words in xyzz_mem order (X, Y, ZZ, ZZZ, 9 limbs each), an affine operand the first 18 of 36
// (x, y), a packed table entry 16 words (affine256), a loop-form record the 32 words of affine_limbs.  Nothing is converted or
// normalised on the way in or out.
#pragma once
#include "../ec.h"

namespace reef {

REEF_HD fe raw_fe(const u32 *p, double bound) {
    fe x;
#pragma unroll
    for (int i = 0; i < 9; ++i) x.l[i] = p[i];
    REEF_SET_BOUND(x, bound);
    (void)bound;
    return x;
}
// bounds: the multiples of M the caller vouches for (X, Y, ZZ, ZZZ), read by the REEF_BOUNDS build alone
REEF_HD xyzz raw_xyzz(const u32 *p, const double *bounds) {
    xyzz r;
    r.x = raw_fe(p, bounds[0]); r.y = raw_fe(p + 9, bounds[1]); r.zz = raw_fe(p + 18, bounds[2]); r.zzz = raw_fe(p + 27, bounds[3]);
    return r;
}
REEF_HD affine raw_affine(const u32 *p, const double *bounds) {
    affine r;
    r.x = raw_fe(p, bounds[0]); r.y = raw_fe(p + 9, bounds[1]);
    return r;
}
REEF_HD void raw_store(u32 *p, const xyzz &v) {
#pragma unroll
    for (int i = 0; i < 9; ++i) { p[i] = v.x.l[i]; p[9 + i] = v.y.l[i]; p[18 + i] = v.zz.l[i]; p[27 + i] = v.zzz.l[i]; }
}
REEF_HD xyzz affine_as_xyzz(const affine &p) {          // an affine result in the 36-word form: (x, y, 0, 0)
    xyzz r;
    r.x = p.x; r.y = p.y; r.zz = fe_zero(); r.zzz = fe_zero();
    return r;
}

// Predicates: 0 fe_is_zero(word 0..8)   1 fe_is_literal_zero(words 0..8)   2 xyzz_is_inf(36 words)   3 affine_is_inf(18 words)
enum { EC_PRED_ZERO = 0, EC_PRED_LITERAL_ZERO = 1, EC_PRED_XYZZ_INF = 2, EC_PRED_AFFINE_INF = 3 };
template <int C> REEF_HD u32 ec_pred(int op, const u32 *in, const double *bounds) {
    switch (op) {
        case EC_PRED_ZERO: return fe_is_zero<C>(raw_fe(in, bounds[0])) ? 1u : 0u;
        case EC_PRED_LITERAL_ZERO: return fe_is_literal_zero(raw_fe(in, bounds[0])) ? 1u : 0u;
        case EC_PRED_XYZZ_INF: return xyzz_is_inf<C>(raw_xyzz(in, bounds)) ? 1u : 0u;
        default: return affine_is_inf(raw_affine(in, bounds)) ? 1u : 0u;
    }
}

// One-wave operations on a (XYZZ), b (XYZZ) or p (affine), flags bit 0 = a_known_empty, bit 1 = p_inf:
//   0 xyzz_dbl_affine(p)   1 xyzz_dbl(a)   2 xyzz_add(a, b)   3 xyzz_neg(a)   4 affine_neg(p)   5 xyzz_from_affine(p)
//   6 xyzz_madd_flags(a, a_known_empty, p, p_inf)
enum { EC_DBL_AFFINE = 0, EC_DBL = 1, EC_ADD = 2, EC_NEG = 3, EC_AFFINE_NEG = 4, EC_FROM_AFFINE = 5, EC_MADD_FLAGS = 6 };
template <int C> REEF_HD xyzz ec_one_wave(int op, const xyzz &a, const xyzz &b, const affine &p, u32 flags) {
    switch (op) {
        case EC_DBL_AFFINE: return xyzz_dbl_affine<C>(p);
        case EC_DBL: return xyzz_dbl<C>(a);
        case EC_ADD: return xyzz_add<C>(a, b);
        case EC_NEG: return xyzz_neg<C>(a);
        case EC_AFFINE_NEG: return affine_as_xyzz(affine_neg<C>(p));
        case EC_FROM_AFFINE: return xyzz_from_affine<C>(p);
        default: return xyzz_madd_flags<C>(a, (flags & 1u) != 0, p, (flags & 2u) != 0);
    }
}

// One entry of the bucket accumulation in its two forms (msm_kernels.inc: k_accum0), from the words each form loads.
// Loop form: the record's head and the y block its sign picked, its flag word as p_inf.
template <int C> REEF_HD xyzz ec_entry_limbs(const xyzz &acc, bool acc_empty, const limbs_entry &raw, bool neg) {
    bool pt_inf;
    const affine pt = affine_from_limbs(raw, neg, &pt_inf);
    return xyzz_madd_flags<C>(acc, acc_empty, pt, pt_inf);
}
// Packed form: unpacked, and negated when the digit is negative, per entry.
template <int C> REEF_HD xyzz ec_entry_packed(const xyzz &acc, bool acc_empty, const affine256 &raw, bool neg) {
    affine pt = affine_from_table(raw);
    pt.y = fe_select(neg && !affine_is_inf(pt), fe_neg<C, 2>(pt.y), pt.y);
    return xyzz_madd_flag<C>(acc, acc_empty, pt);
}
// the words load_limbs_entry (msm_kernels.inc) takes from a record, for the host
REEF_HD limbs_entry limbs_entry_of(const affine_limbs &r, bool neg) {
    limbs_entry e;
    for (int i = 0; i < 12; ++i) e.head[i] = r.w[i];
    for (int i = 0; i < 8; ++i) e.ysel[i] = r.w[(neg ? LIMBS_NEG_Y : LIMBS_Y) + i];
    return e;
}
REEF_HD affine256 raw_affine256(const u32 *p) {
    affine256 m;
    for (int i = 0; i < 8; ++i) { m.x.w[i] = p[i]; m.y.w[i] = p[8 + i]; }
    return m;
}

// Conversions, 36 words in and out (unused words of the result are zero):
//   0 xyzz_to_abi_jacobian -> 24 words   1 xyzz_from_abi_jacobian (24 words in)   2 xyzz_to_affine -> 18 raw words
//   3 affine_compress (18 words in) -> 8 words
enum { EC_TO_JACOBIAN = 0, EC_FROM_JACOBIAN = 1, EC_TO_AFFINE = 2, EC_COMPRESS = 3 };
template <int C> REEF_HD void ec_convert(int op, const u32 *in, const double *bounds, u32 *out) {
    for (int i = 0; i < 36; ++i) out[i] = 0;
    if (op == EC_TO_JACOBIAN) {
        const jacobian256 j = xyzz_to_abi_jacobian<C>(raw_xyzz(in, bounds));
        for (int i = 0; i < 8; ++i) { out[i] = j.x.w[i]; out[8 + i] = j.y.w[i]; out[16 + i] = j.z.w[i]; }
    } else if (op == EC_FROM_JACOBIAN) {
        jacobian256 j;
        for (int i = 0; i < 8; ++i) { j.x.w[i] = in[i]; j.y.w[i] = in[8 + i]; j.z.w[i] = in[16 + i]; }
        raw_store(out, xyzz_from_abi_jacobian<C>(j));
    } else if (op == EC_TO_AFFINE) {
        raw_store(out, affine_as_xyzz(xyzz_to_affine<C>(raw_xyzz(in, bounds))));
    } else {
        const fe256 c = affine_compress<C>(raw_affine(in, bounds));
        for (int i = 0; i < 8; ++i) out[i] = c.w[i];
    }
}

}  // namespace reef
