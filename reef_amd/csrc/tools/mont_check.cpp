// Host build of field.h's Montgomery products with bound tracking (REEF_BOUNDS), on raw 9 x 29-bit limbs: what
// tests/test_mont_reduction.py compares with Python integers.  Unlike host_check.cpp the operands are not taken
// from the ABI form, so limbs and values can sit exactly at the bounds each function states.  TEST HARNESS ONLY.
//   g++ -O2 -std=c++17 -DREEF_BOUNDS -shared -fPIC mont_check.cpp -o libreef_montcheck.so
#include <stddef.h>
#include <stdint.h>

#include "../field.h"

using namespace reef;

static fe load(const uint32_t *l, double bound) {
    fe x;
    for (int i = 0; i < 9; ++i) x.l[i] = l[i];
    x.bound = bound;
    return x;
}

// The reduction as the sum-check and Merkle kernels run it (fe_vec.h: wide18_mont): 18 product columns of a*b,
// carried to 29 bits, biased with mont_bias, nine rounds with the upper columns fed in one per round.
template <int F> static fe wide_reduce(const fe &a, const fe &b) {
    u64 w[18] = {0};
    for (int i = 0; i < 9; ++i)
        for (int j = 0; j < 9; ++j) w[i + j] += (u64)a.l[i] * b.l[j];
    for (int i = 0; i < 17; ++i) {
        w[i + 1] += w[i] >> LIMB_BITS;
        w[i] &= LIMB_MASK;
    }
    u64 t[10];
    for (int i = 0; i < 9; ++i) t[i] = w[i];
    t[9] = 0;
    mont_bias(t);
    for (int r = 0; r < 9; ++r) {
        mont_round<F>(t);
        t[8] += w[9 + r];
    }
    return mont_finish<F>(t);
}

template <int F, int K> static fe op_k(int op, const fe &a, const fe &b, const fe &c) {
    return op == 3 ? fe_mul_sub<F, K>(a, b, c) : fe_sqr_sub<F, K>(a, c);
}

template <int F> static fe op_f(int op, int k, const fe &a, const fe &b, const fe &c, const fe &d) {
    switch (op) {
        case 0: return fe_mul<F>(a, b);
        case 1: return fe_sqr<F>(a);
        case 2: return fe_mul2_add<F>(a, b, c, d);
        case 5: return wide_reduce<F>(a, b);
        default: break;
    }
    switch (k) {
        case 2: return op_k<F, 2>(op, a, b, c);
        case 4: return op_k<F, 4>(op, a, b, c);
        case 8: return op_k<F, 8>(op, a, b, c);
        case 16: return op_k<F, 16>(op, a, b, c);
        default: return op_k<F, 32>(op, a, b, c);
    }
}

// op 0 a*b, 1 a^2, 2 a*b + c*d, 3 a*b + K*M - c, 4 a^2 + K*M - c, 5 a*b through mont_bias + rounds (the wide form).
// Operands are n x 9 limbs; bounds[0..3] are the value bounds (in units of M) of a, b, c, d.
extern "C" void mc_op(int field, int op, int k, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d,
                      const double *bounds, uint32_t *out, size_t n) {
    for (size_t i = 0; i < n; ++i) {
        const fe x = load(a + 9 * i, bounds[0]), y = load(b + 9 * i, bounds[1]), z = load(c + 9 * i, bounds[2]),
                 w = load(d + 9 * i, bounds[3]);
        const fe r = field == 0 ? op_f<0>(op, k, x, y, z, w) : op_f<1>(op, k, x, y, z, w);
        for (int j = 0; j < 9; ++j) out[9 * i + j] = r.l[j];
    }
}
