// Device build of field.h and fe_vec.h on raw limbs: the twin of mont_check.cpp, compiled with the release CXXFLAGS so that
// what it runs is what the product ships (on gfx950 the products are the v_mad_u64_u32 rows of field_mad_gfx950.h, not the
// host forms mont_check.cpp reaches).  tests/test_gpu_field_bounds.py compares every entry point with Python integers, with
// operands at the limb and value bounds each function states.  TEST HARNESS ONLY: not part of libreef_msm.so.
//
// Every entry point takes host arrays, returns 0 on success and the failing hipError_t otherwise.
#define REEF_CURVE 0
#include "../msm_kernels.inc"
#include "../fe_vec.h"

#include <stddef.h>

using namespace reef;

namespace {

__device__ __forceinline__ fe fc_load(const u32 *p) {
    fe x;
#pragma unroll
    for (int i = 0; i < 9; ++i) x.l[i] = p[i];
    return x;
}
__device__ __forceinline__ void fc_store(u32 *p, const fe &x) {
#pragma unroll
    for (int i = 0; i < 9; ++i) p[i] = x.l[i];
}
__device__ __forceinline__ fe256 fc_load256(const u32 *p) {   // the first 8 of 9 words
    fe256 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v.w[i] = p[i];
    return v;
}
__device__ __forceinline__ void fc_store256(u32 *p, const fe256 &v) {
#pragma unroll
    for (int i = 0; i < 8; ++i) p[i] = v.w[i];
    p[8] = 0;
}

template <int F> __device__ __forceinline__ fe wide_form(const fe &a, const fe &b) {   // the product as the row kernels form it
    fe_wide18 w;
    wide18_zero(w);
    wide18_mac(w, a.l, b.l);
    return wide18_mont<F>(w, 2.0);
}

template <int F, int K> __device__ fe op_k(int op, const fe &a, const fe &b, const fe &c) {
    switch (op) {
        case 3: return fe_mul_sub<F, K>(a, b, c);
        case 4: return fe_sqr_sub<F, K>(a, c);
        default: return fe_sub<F, K>(a, b);
    }
}

// Operands and results are 9 words each; the packed (fe256) operands and results use the first 8.
//   0 a*b   1 a^2   2 a*b + c*d   3 a*b + K*M - c   4 a^2 + K*M - c   5 a*b through wide18_mac + wide18_mont (mont_check.cpp's
//   numbering)   6 a + b   7 a + K*M - b   8 fe_norm_strict(a)   9 fe_canon(a)   10 fe_inv(a)   11 fe_unpack   12 fe_pack
//   13 fe_from_abi   14 fe_to_abi   15 fe_from_integer   16 fe_to_integer   17 fe_abi_to_integer
template <int F> __device__ void op_f(int op, int k, const u32 *pa, const u32 *pb, const u32 *pc, const u32 *pd, u32 *po) {
    const fe a = fc_load(pa), b = fc_load(pb), c = fc_load(pc), d = fc_load(pd);
    switch (op) {
        case 0: fc_store(po, fe_mul<F>(a, b)); return;
        case 1: fc_store(po, fe_sqr<F>(a)); return;
        case 2: fc_store(po, fe_mul2_add<F>(a, b, c, d)); return;
        case 5: fc_store(po, wide_form<F>(a, b)); return;
        case 6: fc_store(po, fe_add<F>(a, b)); return;
        case 8: fc_store(po, fe_norm_strict(a)); return;
        case 9: fc_store(po, fe_canon<F>(a)); return;
        case 10: fc_store(po, fe_inv<F>(a)); return;
        case 11: fc_store(po, fe_unpack(fc_load256(pa))); return;
        case 12: fc_store256(po, fe_pack(a)); return;
        case 13: fc_store(po, fe_from_abi<F>(fc_load256(pa))); return;
        case 14: fc_store256(po, fe_to_abi<F>(a)); return;
        case 15: fc_store(po, fe_from_integer<F>(fc_load256(pa))); return;
        case 16: fc_store256(po, fe_to_integer<F>(a)); return;
        case 17: fc_store256(po, fe_abi_to_integer<F>(fc_load256(pa))); return;
        default: break;
    }
    fe r;
    switch (k) {
        case 2: r = op_k<F, 2>(op, a, b, c); break;
        case 4: r = op_k<F, 4>(op, a, b, c); break;
        case 8: r = op_k<F, 8>(op, a, b, c); break;
        case 16: r = op_k<F, 16>(op, a, b, c); break;
        default: r = op_k<F, 32>(op, a, b, c); break;
    }
    fc_store(po, r);
}

template <int F>
__global__ void __launch_bounds__(256) k_fc_op(int op, int k, const u32 *a, const u32 *b, const u32 *c, const u32 *d, u32 *out, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    op_f<F>(op, k, a + 9 * i, b + 9 * i, c + 9 * i, d + 9 * i, out + 9 * i);
}

// 9 x u64 columns -> fe: op 0 fe_from_wide, op 1 fe_from_limb_sums
template <int F> __global__ void __launch_bounds__(256) k_fc_wide(int op, const u64 *cols, u32 *out, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe_wide w;
#pragma unroll
    for (int j = 0; j < 9; ++j) w.l[j] = cols[9 * i + j];
    fc_store(out + 9 * i, op == 0 ? fe_from_wide<F>(w) : fe_from_limb_sums<F>(w));
}

// Thread i sums the products a[i*m + p] * b[i*m + p], p < m, in the callers' cadence (a carry after every fourth product and
// one before the reduction), then reduces with wide18_mont(w, 2) (reduce = 0, the Merkle form) or wide18_reduce (reduce = 1).
template <int F> __global__ void __launch_bounds__(256) k_fc_wide18(int reduce, const u32 *a, const u32 *b, u64 m, u32 *out, u64 n) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe_wide18 w;
    wide18_zero(w);
    for (u64 p = 0; p < m; ++p) {
        const fe x = fc_load(a + 9 * (i * m + p)), y = fc_load(b + 9 * (i * m + p));
        wide18_mac(w, x.l, y.l);
        if ((p & 3) == 3) wide18_carry(w);
    }
    wide18_carry(w);
    fc_store(out + 9 * i, reduce ? wide18_reduce<F>(w) : wide18_mont<F>(w, 2.0));
}

// One value per lane of whole 64-lane waves; the total of wave j is lane 63's result.
__global__ void __launch_bounds__(256) k_fc_wave_sum(const u64 *v, u64 *out, u64 nwaves) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;   // the grid covers exactly nwaves * 64 lanes
    const unsigned long long s = wave_sum63(v[i]);
    if ((i & 63) == 63) out[i >> 6] = s;
    (void)nwaves;
}

struct DevBufs {
    void *p[8] = {};
    ~DevBufs() {
        for (void *q : p)
            if (q) (void)hipFree(q);
    }
};

#define FC_TRY(expr)                              \
    do {                                          \
        const hipError_t e_ = (expr);             \
        if (e_ != hipSuccess) return (int)e_;     \
    } while (0)

int finish_launch() {
    FC_TRY(hipGetLastError());
    FC_TRY(hipDeviceSynchronize());
    return 0;
}

unsigned blocks_for(size_t n, unsigned tpb) { return (unsigned)((n + tpb - 1) / tpb); }

}  // namespace

extern "C" {

// Operands are n x 9 words (a .. d; c and d may be null where op does not read them); out is n x 9 words.
int fc_op(int field, int op, int k, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *d, uint32_t *out, size_t n) {
    if (n == 0) return 0;
    const size_t bytes = 9 * sizeof(uint32_t) * n;
    DevBufs g;
    const uint32_t *host[4] = {a, b, c, d};
    for (int j = 0; j < 5; ++j) {
        FC_TRY(hipMalloc(&g.p[j], bytes));
        if (j < 4) FC_TRY(host[j] ? hipMemcpy(g.p[j], host[j], bytes, hipMemcpyHostToDevice) : hipMemset(g.p[j], 0, bytes));
    }
    const u32 *da = (const u32 *)g.p[0], *db = (const u32 *)g.p[1], *dc = (const u32 *)g.p[2], *dd = (const u32 *)g.p[3];
    u32 *dout = (u32 *)g.p[4];
    if (field == 0) k_fc_op<0><<<blocks_for(n, 256), 256>>>(op, k, da, db, dc, dd, dout, n);
    else k_fc_op<1><<<blocks_for(n, 256), 256>>>(op, k, da, db, dc, dd, dout, n);
    if (const int s = finish_launch()) return s;
    FC_TRY(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    return 0;
}

// cols: n x 9 u64; op 0 fe_from_wide, 1 fe_from_limb_sums; out n x 9 words
int fc_wide(int field, int op, const uint64_t *cols, uint32_t *out, size_t n) {
    if (n == 0) return 0;
    DevBufs g;
    FC_TRY(hipMalloc(&g.p[0], 9 * sizeof(uint64_t) * n));
    FC_TRY(hipMalloc(&g.p[1], 9 * sizeof(uint32_t) * n));
    FC_TRY(hipMemcpy(g.p[0], cols, 9 * sizeof(uint64_t) * n, hipMemcpyHostToDevice));
    if (field == 0) k_fc_wide<0><<<blocks_for(n, 256), 256>>>(op, (const u64 *)g.p[0], (u32 *)g.p[1], n);
    else k_fc_wide<1><<<blocks_for(n, 256), 256>>>(op, (const u64 *)g.p[0], (u32 *)g.p[1], n);
    if (const int s = finish_launch()) return s;
    FC_TRY(hipMemcpy(out, g.p[1], 9 * sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    return 0;
}

// a, b: n sums of m products each (n*m x 9 words); out: n x 9 words
int fc_wide18(int field, int reduce, const uint32_t *a, const uint32_t *b, size_t m, uint32_t *out, size_t n) {
    if (n == 0 || m == 0) return 0;
    const size_t in_bytes = 9 * sizeof(uint32_t) * n * m;
    DevBufs g;
    FC_TRY(hipMalloc(&g.p[0], in_bytes));
    FC_TRY(hipMalloc(&g.p[1], in_bytes));
    FC_TRY(hipMalloc(&g.p[2], 9 * sizeof(uint32_t) * n));
    FC_TRY(hipMemcpy(g.p[0], a, in_bytes, hipMemcpyHostToDevice));
    FC_TRY(hipMemcpy(g.p[1], b, in_bytes, hipMemcpyHostToDevice));
    if (field == 0) k_fc_wide18<0><<<blocks_for(n, 256), 256>>>(reduce, (const u32 *)g.p[0], (const u32 *)g.p[1], m, (u32 *)g.p[2], n);
    else k_fc_wide18<1><<<blocks_for(n, 256), 256>>>(reduce, (const u32 *)g.p[0], (const u32 *)g.p[1], m, (u32 *)g.p[2], n);
    if (const int s = finish_launch()) return s;
    FC_TRY(hipMemcpy(out, g.p[2], 9 * sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    return 0;
}

// v: nwaves x 64 lane values; out: nwaves totals (lane 63 of each wave)
int fc_wave_sum(const uint64_t *v, uint64_t *out, size_t nwaves) {
    if (nwaves == 0) return 0;
    DevBufs g;
    FC_TRY(hipMalloc(&g.p[0], 64 * sizeof(uint64_t) * nwaves));
    FC_TRY(hipMalloc(&g.p[1], sizeof(uint64_t) * nwaves));
    FC_TRY(hipMemcpy(g.p[0], v, 64 * sizeof(uint64_t) * nwaves, hipMemcpyHostToDevice));
    k_fc_wave_sum<<<(unsigned)nwaves, 64>>>((const u64 *)g.p[0], (u64 *)g.p[1], nwaves);
    if (const int s = finish_launch()) return s;
    FC_TRY(hipMemcpy(out, g.p[1], sizeof(uint64_t) * nwaves, hipMemcpyDeviceToHost));
    return 0;
}

// k_fe_import (dir 0: flag_a = is_mont) or k_fe_export (dir 1: flag_a = src_is_integer, flag_b = to_mont) on n packed elements
// (n x 8 words), with in == out on the device when in_place, in launches of 256 as the rows issue them
int fc_convert(int field, int dir, int flag_a, int flag_b, int in_place, const uint32_t *in, uint32_t *out, size_t n) {
    if (n == 0) return 0;
    const size_t bytes = sizeof(fe256) * n;
    DevBufs g;
    FC_TRY(hipMalloc(&g.p[0], bytes));
    FC_TRY(hipMemcpy(g.p[0], in, bytes, hipMemcpyHostToDevice));
    if (!in_place) FC_TRY(hipMalloc(&g.p[1], bytes));
    const fe256 *din = (const fe256 *)g.p[0];
    fe256 *dout = (fe256 *)(in_place ? g.p[0] : g.p[1]);
    const unsigned nb = blocks_for(n, 256);
    if (dir == 0) {
        if (field == 0) k_fe_import<0><<<nb, 256>>>(din, n, flag_a, dout);
        else k_fe_import<1><<<nb, 256>>>(din, n, flag_a, dout);
    } else {
        if (field == 0) k_fe_export<0><<<nb, 256>>>(din, n, flag_a, flag_b, dout);
        else k_fe_export<1><<<nb, 256>>>(din, n, flag_a, flag_b, dout);
    }
    if (const int s = finish_launch()) return s;
    FC_TRY(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
