// Device build of ec.h and ec_coop.h on raw limbs: the twin of the raw-limb entry points of host_check.cpp, compiled with the
// release CXXFLAGS so that what it runs is what the product ships.  tests/test_gpu_ec_bounds.py feeds it the grid of
// tests/ec_grid.py -- every representation the loose bounds of ec.h allow, every identity form, the exceptional cases in
// every lane layout -- and checks each raw result against Python integers.  TEST HARNESS ONLY: not part of libreef_msm.so.
//
// Data forms are those of tools/ec_ops.h.  Every entry point takes host arrays, returns 0 on success and the failing
// hipError_t otherwise.  The one-wave kernels run in blocks of 256 threads with a ragged last block whose idle lanes repeat
// lane n - 1, as the product's kernels do: there is no early return in front of a wave-wide test (REEF_ANY, __any).
#define REEF_CURVE 0
#include "../msm_kernels.inc"
#include "ec_ops.h"

#include <stddef.h>

using namespace reef;

namespace {

__device__ const double NO_BOUNDS[4] = {0.0, 0.0, 0.0, 0.0};   // read by REEF_BOUNDS builds alone

template <int C> __global__ void __launch_bounds__(256) k_ec_pred(int op, const u32 *in, u32 stride, u32 *out, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 j = i < n ? i : n - 1;
    const u32 r = ec_pred<C>(op, in + (size_t)stride * j, NO_BOUNDS);
    if (i < n) out[i] = r;
}

template <int C>
__global__ void __launch_bounds__(256) k_ec_one(int op, const u32 *a, const u32 *b, const u32 *flags, u32 *out, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 j = i < n ? i : n - 1;
    const xyzz r = ec_one_wave<C>(op, raw_xyzz(a + 36 * (size_t)j, NO_BOUNDS), raw_xyzz(b + 36 * (size_t)j, NO_BOUNDS),
                                  raw_affine(b + 36 * (size_t)j, NO_BOUNDS), flags[j]);
    if (i < n) raw_store(out + 36 * (size_t)i, r);
}

// packed table entries -> loop-form records, as the engine's table builder stores them
template <int C> __global__ void __launch_bounds__(256) k_ec_records(const affine256 *src, affine_limbs *dst, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const affine_limbs r = affine_limbs_from_table<C>(load_affine256(src + i));
    u32x4 *q = reinterpret_cast<u32x4 *>(dst + i);
#pragma unroll
    for (int k = 0; k < 8; ++k) q[k] = mk_u32x4(r.w[4 * k], r.w[4 * k + 1], r.w[4 * k + 2], r.w[4 * k + 3]);
}

// acc + (+/-) entry in both forms of k_accum0: pay = entry index | sign << 31 (the sorted entries' payload)
template <int C>
__global__ void __launch_bounds__(256) k_ec_entry(const affine256 *packed, const affine_limbs *records, const u32 *pay, const u32 *acc,
                                                 const u32 *empty, u32 *out_limbs, u32 *out_packed, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 j = i < n ? i : n - 1;
    const xyzz a = raw_xyzz(acc + 36 * (size_t)j, NO_BOUNDS);
    const bool neg = (pay[j] >> 31) != 0, a_empty = empty[j] != 0;
    const xyzz rl = ec_entry_limbs<C>(a, a_empty, load_accum_entry(records, pay[j]), neg);
    const xyzz rp = ec_entry_packed<C>(a, a_empty, load_accum_entry(packed, pay[j]), neg);
    if (i < n) {
        raw_store(out_limbs + 36 * (size_t)i, rl);
        raw_store(out_packed + 36 * (size_t)i, rp);
    }
}

// One thread per chain: the accumulator after every step, in the loop's form (acc_empty only before the first entry).
template <int C>
__global__ void __launch_bounds__(256) k_ec_chain(const affine_limbs *records, const u32 *pay, u32 len, u32 *out, u32 nchains) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 j = i < nchains ? i : nchains - 1;
    xyzz acc = xyzz_identity();
    bool acc_empty = true;
    for (u32 k = 0; k < len; ++k) {
        const u32 p = pay[(size_t)j * len + k];
        acc = ec_entry_limbs<C>(acc, acc_empty, load_accum_entry(records, p), (p >> 31) != 0);
        acc_empty = false;
        if (i < nchains) raw_store(out + 36 * ((size_t)i * len + k), acc);
    }
}

// The four-wave forms: one workgroup of 256 threads per 64 inputs, one addition site and one doubling site, the result taken
// from a different wave per block (every wave must hold it).  op 0: a + b, op 1: 2a.
template <int C> __global__ void __launch_bounds__(256) k_ec_coop(int op, const xyzz_mem *a, const xyzz_mem *b, u32 *out, u32 n) {
    __shared__ CoopLds L;
    const int lane = threadIdx.x & 63, role = threadIdx.x >> 6;
    const u32 i = blockIdx.x * 64u + lane;
    const u32 j = i < n ? i : n - 1;                      // every thread takes part in the barriers
    const xyzz x = load_xyzz_coop(a + j), y = load_xyzz_coop(b + j);
    xyzz r;
    if (op == 0) r = xyzz_add_coop<C>(x, y, L, role, lane);
    else r = xyzz_dbl_coop<C>(x, L, role, lane);
    if (role == (int)(blockIdx.x & 3u) && i < n) raw_store(out + 36 * (size_t)i, r);
}

template <int C> __global__ void __launch_bounds__(256) k_ec_convert(int op, const u32 *in, u32 *out, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;                                   // nothing wave-wide in the conversions
    ec_convert<C>(op, in + 36 * (size_t)i, NO_BOUNDS, out + 36 * (size_t)i);
}

struct DevBufs {
    void *p[10] = {};
    ~DevBufs() {
        for (void *q : p)
            if (q) (void)hipFree(q);
    }
};

#define EC_TRY(expr)                              \
    do {                                          \
        const hipError_t e_ = (expr);             \
        if (e_ != hipSuccess) return (int)e_;     \
    } while (0)

int finish_launch() {
    EC_TRY(hipGetLastError());
    EC_TRY(hipDeviceSynchronize());
    return 0;
}
int upload(DevBufs &g, int slot, const void *host, size_t bytes) {
    EC_TRY(hipMalloc(&g.p[slot], bytes));
    EC_TRY(hipMemcpy(g.p[slot], host, bytes, hipMemcpyHostToDevice));
    return 0;
}
int output(DevBufs &g, int slot, size_t bytes) {
    EC_TRY(hipMalloc(&g.p[slot], bytes));
    EC_TRY(hipMemset(g.p[slot], 0, bytes));
    return 0;
}

unsigned blocks_for(size_t n, unsigned per_block) { return (unsigned)((n + per_block - 1) / per_block); }
constexpr size_t W = sizeof(uint32_t), MAX_N = 1u << 24;

// pay[i] = entry index | sign << 31: every index must lie inside the table
bool payloads_in_range(const uint32_t *pay, size_t n, size_t entries) {
    for (size_t i = 0; i < n; ++i)
        if ((pay[i] & 0x7fffffffu) >= entries) return false;
    return true;
}

}  // namespace

extern "C" {

// in: n x stride words (stride >= 9, 36, 18 for ops 0/1, 2, 3 of ec_ops.h: ec_pred); out: n words, 1 = true
int ec_check_pred(int curve, int op, const uint32_t *in, size_t stride, uint32_t *out, size_t n) {
    if (n == 0) return 0;
    const size_t need = op == EC_PRED_XYZZ_INF ? 36 : op == EC_PRED_AFFINE_INF ? 18 : 9;
    if (op < 0 || op > 3 || stride < need || stride > 36 || n > MAX_N) return (int)hipErrorInvalidValue;
    DevBufs g;
    if (const int s = upload(g, 0, in, W * stride * n)) return s;
    if (const int s = output(g, 1, W * n)) return s;
    if (curve == 0) k_ec_pred<0><<<blocks_for(n, 256), 256>>>(op, (const u32 *)g.p[0], (u32)stride, (u32 *)g.p[1], (u32)n);
    else k_ec_pred<1><<<blocks_for(n, 256), 256>>>(op, (const u32 *)g.p[0], (u32)stride, (u32 *)g.p[1], (u32)n);
    if (const int s = finish_launch()) return s;
    EC_TRY(hipMemcpy(out, g.p[1], W * n, hipMemcpyDeviceToHost));
    return 0;
}

// a, b: n x 36 words (an affine operand is the first 18 words of b); flags: n words; out: n x 36 words (ec_ops.h: ec_one_wave)
int ec_check_one_wave(int curve, int op, const uint32_t *a, const uint32_t *b, const uint32_t *flags, uint32_t *out, size_t n) {
    if (n == 0) return 0;
    if (op < 0 || op > 6 || n > MAX_N) return (int)hipErrorInvalidValue;
    DevBufs g;
    if (const int s = upload(g, 0, a, 36 * W * n)) return s;
    if (const int s = upload(g, 1, b, 36 * W * n)) return s;
    if (const int s = upload(g, 2, flags, W * n)) return s;
    if (const int s = output(g, 3, 36 * W * n)) return s;
    const u32 *da = (const u32 *)g.p[0], *db = (const u32 *)g.p[1], *df = (const u32 *)g.p[2];
    if (curve == 0) k_ec_one<0><<<blocks_for(n, 256), 256>>>(op, da, db, df, (u32 *)g.p[3], (u32)n);
    else k_ec_one<1><<<blocks_for(n, 256), 256>>>(op, da, db, df, (u32 *)g.p[3], (u32)n);
    if (const int s = finish_launch()) return s;
    EC_TRY(hipMemcpy(out, g.p[3], 36 * W * n, hipMemcpyDeviceToHost));
    return 0;
}

// table: entries x 16 words (packed, canonical, internal form); pay, empty: n words; acc: n x 36 words.
// out_limbs, out_packed: n x 36 words (the sum through either form); records: entries x 32 words
int ec_check_entry(int curve, const uint32_t *table, size_t entries, const uint32_t *pay, const uint32_t *acc, const uint32_t *empty,
                   uint32_t *out_limbs, uint32_t *out_packed, uint32_t *records, size_t n) {
    if (n == 0 || entries == 0) return 0;
    if (n > MAX_N || entries > MAX_N || !payloads_in_range(pay, n, entries)) return (int)hipErrorInvalidValue;
    DevBufs g;
    if (const int s = upload(g, 0, table, 16 * W * entries)) return s;
    if (const int s = output(g, 1, 32 * W * entries)) return s;
    if (const int s = upload(g, 2, pay, W * n)) return s;
    if (const int s = upload(g, 3, acc, 36 * W * n)) return s;
    if (const int s = upload(g, 4, empty, W * n)) return s;
    if (const int s = output(g, 5, 36 * W * n)) return s;
    if (const int s = output(g, 6, 36 * W * n)) return s;
    const affine256 *dt = (const affine256 *)g.p[0];
    affine_limbs *dr = (affine_limbs *)g.p[1];
    const u32 *dp = (const u32 *)g.p[2], *dacc = (const u32 *)g.p[3], *de = (const u32 *)g.p[4];
    if (curve == 0) {
        k_ec_records<0><<<blocks_for(entries, 256), 256>>>(dt, dr, (u32)entries);
        k_ec_entry<0><<<blocks_for(n, 256), 256>>>(dt, dr, dp, dacc, de, (u32 *)g.p[5], (u32 *)g.p[6], (u32)n);
    } else {
        k_ec_records<1><<<blocks_for(entries, 256), 256>>>(dt, dr, (u32)entries);
        k_ec_entry<1><<<blocks_for(n, 256), 256>>>(dt, dr, dp, dacc, de, (u32 *)g.p[5], (u32 *)g.p[6], (u32)n);
    }
    if (const int s = finish_launch()) return s;
    EC_TRY(hipMemcpy(out_limbs, g.p[5], 36 * W * n, hipMemcpyDeviceToHost));
    EC_TRY(hipMemcpy(out_packed, g.p[6], 36 * W * n, hipMemcpyDeviceToHost));
    EC_TRY(hipMemcpy(records, g.p[1], 32 * W * entries, hipMemcpyDeviceToHost));
    return 0;
}

// pay: nchains x len payloads into the table; out: nchains x len x 36 words, the accumulator after every step
int ec_check_chain(int curve, const uint32_t *table, size_t entries, const uint32_t *pay, size_t len, uint32_t *out, size_t nchains) {
    if (nchains == 0 || len == 0 || entries == 0) return 0;
    if (nchains > 4096 || len > 65536 || entries > MAX_N || !payloads_in_range(pay, nchains * len, entries)) return (int)hipErrorInvalidValue;
    DevBufs g;
    if (const int s = upload(g, 0, table, 16 * W * entries)) return s;
    if (const int s = output(g, 1, 32 * W * entries)) return s;
    if (const int s = upload(g, 2, pay, W * nchains * len)) return s;
    if (const int s = output(g, 3, 36 * W * nchains * len)) return s;
    const affine256 *dt = (const affine256 *)g.p[0];
    affine_limbs *dr = (affine_limbs *)g.p[1];
    if (curve == 0) {
        k_ec_records<0><<<blocks_for(entries, 256), 256>>>(dt, dr, (u32)entries);
        k_ec_chain<0><<<blocks_for(nchains, 256), 256>>>(dr, (const u32 *)g.p[2], (u32)len, (u32 *)g.p[3], (u32)nchains);
    } else {
        k_ec_records<1><<<blocks_for(entries, 256), 256>>>(dt, dr, (u32)entries);
        k_ec_chain<1><<<blocks_for(nchains, 256), 256>>>(dr, (const u32 *)g.p[2], (u32)len, (u32 *)g.p[3], (u32)nchains);
    }
    if (const int s = finish_launch()) return s;
    EC_TRY(hipMemcpy(out, g.p[3], 36 * W * nchains * len, hipMemcpyDeviceToHost));
    return 0;
}

// op 0: xyzz_add_coop(a, b), op 1: xyzz_dbl_coop(a); a, b, out: n x 36 words
int ec_check_coop(int curve, int op, const uint32_t *a, const uint32_t *b, uint32_t *out, size_t n) {
    if (n == 0) return 0;
    if (op < 0 || op > 1 || n > MAX_N) return (int)hipErrorInvalidValue;
    DevBufs g;
    if (const int s = upload(g, 0, a, 36 * W * n)) return s;
    if (const int s = upload(g, 1, b, 36 * W * n)) return s;
    if (const int s = output(g, 2, 36 * W * n)) return s;
    const xyzz_mem *da = (const xyzz_mem *)g.p[0], *db = (const xyzz_mem *)g.p[1];
    if (curve == 0) k_ec_coop<0><<<blocks_for(n, 64), 256>>>(op, da, db, (u32 *)g.p[2], (u32)n);
    else k_ec_coop<1><<<blocks_for(n, 64), 256>>>(op, da, db, (u32 *)g.p[2], (u32)n);
    if (const int s = finish_launch()) return s;
    EC_TRY(hipMemcpy(out, g.p[2], 36 * W * n, hipMemcpyDeviceToHost));
    return 0;
}

// in, out: n x 36 words (ec_ops.h: ec_convert)
int ec_check_convert(int curve, int op, const uint32_t *in, uint32_t *out, size_t n) {
    if (n == 0) return 0;
    if (op < 0 || op > 3 || n > MAX_N) return (int)hipErrorInvalidValue;
    DevBufs g;
    if (const int s = upload(g, 0, in, 36 * W * n)) return s;
    if (const int s = output(g, 1, 36 * W * n)) return s;
    if (curve == 0) k_ec_convert<0><<<blocks_for(n, 256), 256>>>(op, (const u32 *)g.p[0], (u32 *)g.p[1], (u32)n);
    else k_ec_convert<1><<<blocks_for(n, 256), 256>>>(op, (const u32 *)g.p[0], (u32 *)g.p[1], (u32)n);
    if (const int s = finish_launch()) return s;
    EC_TRY(hipMemcpy(out, g.p[1], 36 * W * n, hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
