// Host build of decompress_kernels.inc with bound tracking (REEF_BOUNDS): the fixed-trip-count square root and the decoding rule the
// kernels run, executed on the CPU so that `pytest -m "not gpu"` can compare them with the oracle (tests/test_decompress_host.py).
// TEST HARNESS ONLY -- the product (libreef_msm.so) never links this.
//   g++ -O2 -std=c++17 -DREEF_BOUNDS -shared -fPIC sqrt_check.cpp -o libreef_sqrtcheck.so
#include <stddef.h>

#include "../ec.h"
#include "../decompress_kernels.inc"

using namespace reef;

template <int F> static void root_of(const fe256 *a, fe256 *out) {
    fe y;
    if (fe_sqrt_even<F, true>(fe_from_abi<F>(*a), &FC<F>::SQ_TAB[0][0], y)) *out = fe_to_abi<F>(y);
    else
        for (int k = 0; k < 8; ++k) out->w[k] = 0xffffffffu;
}

extern "C" {
// out[i] = the even root of a[i] (ABI form), 32 bytes of 0xff for a non-residue: what reef_test_field_op(field, 8, ..) returns
void sqrtcheck_root(int field, const fe256 *a, fe256 *out, size_t n) {
    for (size_t i = 0; i < n; ++i) field == 0 ? root_of<0>(a + i, out + i) : root_of<1>(a + i, out + i);
}
// out[i] = the point of encoding in[i]; returns how many were invalid: what reef_decompress returns
size_t sqrtcheck_decompress(int curve, const fe256 *in, affine256 *out, size_t n) {
    size_t bad = 0;
    for (size_t i = 0; i < n; ++i)
        bad += !(curve == 0 ? point_decompress<0, true>(in[i], &FC<0>::SQ_TAB[0][0], out[i]) : point_decompress<1, true>(in[i], &FC<1>::SQ_TAB[0][0], out[i]));
    return bad;
}
}
