// HIP kernels of the Pasta MSM engine for gfx950 (wave64, 160 KiB LDS per CU).
// Included by kernels_pallas.hip / kernels_vesta.hip with REEF_CURVE = 0 / 1.
//
// Pipeline of one bucket-method MSM (K1), all on one HIP stream, no host round trip:
//   k_recode        scalars (32 B, coalesced) -> signed c-bit digits  dig[w][i]
//   k_count         LDS histogram (up to 32768 counters = 128 KiB) per (slice, group, part)
//   k_scan_*        exclusive scan -> bucket_start[], per-slice cursors
//   k_scatter       LDS cursors -> entries (key, payload) sorted by bucket, one 8-byte store each
//   k_accum0        every thread sums exactly L0 consecutive sorted entries (perfect load
//                   balance whatever the scalar distribution); complete bucket runs go
//                   straight to bucket_acc[], runs cut by a chunk edge become partials
//   k_accumN        wave-cooperative segmented reduction of the partial list (64 slots
//                   -> 2 slots per level) until everything is complete
//   k_reduce_rowcol sum_k k*B_k in two dimensions: the buckets of a group as a sqrt x sqrt matrix,
//                   one wave per row sum and per column sum
//   k_reduce_weighted  two weighted wave sums (suffix scan + tree) -> one point per bucket group
//   k_final         Horner over the bucket groups (c doublings each; none for a pre-shifted key),
//                   XYZZ -> Jacobian
// Batches (rows of reef_msm_rows, the L/R pair of reef_ipa_cross_terms) run through the same
// kernels with blockIdx.y / the key space extended by the batch index.
//
// Reference semantics: Group::vartime_multiscalar_mul of nova-snark's pasta provider
// (-> pasta_msm::pallas/vesta), reached from src/backend/framework.rs:668,695 and
// src/backend/commitment.rs:187,350,361,371,383,422,430 of eniac/Reef.
#include <type_traits>

#include "ec.h"
#include "ec_coop.h"
#include "glv_consts.h"
#include "msm_plan.h"     // the constants the launch plan and the kernels share: SCAN_*, SORT_SEG

namespace reef {

static constexpr u32 KEY_INVALID = 0xffffffffu;
static constexpr int WAVE = 64;

template <int C> struct Kern;  // host-side launch table, one per curve

// ------------------------------------------------------------------ helpers ----
// Everything except the bucket accumulation is a short or latency-bound kernel.  When several
// MSMs are in flight on different HIP streams those kernels share SIMDs with another MSM's
// k_accum0 (which saturates the integer pipe); raising their wave priority lets them run at
// close to their stand-alone latency while k_accum0 fills the remaining issue slots.
__device__ __forceinline__ void latency_critical() { __builtin_amdgcn_s_setprio(3); }

__device__ __forceinline__ u32 extract_bits(const fe256 &k, u32 off, u32 c) {
    const u32 limb = off >> 5, sh = off & 31u;
    u32 lo = 0, hi = 0;
#pragma unroll
    for (u32 l = 0; l < 8; ++l) {
        lo = (l == limb) ? k.w[l] : lo;
        hi = (l == limb + 1) ? k.w[l] : hi;
    }
    u64 v = (((u64)hi << 32) | lo) >> sh;
    return (u32)v & ((1u << c) - 1u);
}

__device__ __forceinline__ fe256 load_fe256(const fe256 *p) {
    const u32x4 *q = reinterpret_cast<const u32x4 *>(p);
    const u32x4 a = q[0], b = q[1];
    fe256 d;
    d.w[0] = a.x; d.w[1] = a.y; d.w[2] = a.z; d.w[3] = a.w;
    d.w[4] = b.x; d.w[5] = b.y; d.w[6] = b.z; d.w[7] = b.w;
    return d;
}
__device__ __forceinline__ void store_fe256(fe256 *p, const fe256 &s) {
    u32x4 *q = reinterpret_cast<u32x4 *>(p);
    q[0] = mk_u32x4(s.w[0], s.w[1], s.w[2], s.w[3]);
    q[1] = mk_u32x4(s.w[4], s.w[5], s.w[6], s.w[7]);
}
__device__ __forceinline__ affine256 load_affine256(const affine256 *p) {
    affine256 r;
    r.x = load_fe256(&p->x);
    r.y = load_fe256(&p->y);
    return r;
}
__device__ __forceinline__ void store_affine256(affine256 *p, const affine256 &s) {
    store_fe256(&p->x, s.x);
    store_fe256(&p->y, s.y);
}
__device__ __forceinline__ jacobian256 load_jacobian256(const jacobian256 *p) {
    jacobian256 r;
    r.x = load_fe256(&p->x); r.y = load_fe256(&p->y); r.z = load_fe256(&p->z);
    return r;
}
__device__ __forceinline__ void store_jacobian256(jacobian256 *p, const jacobian256 &s) {
    store_fe256(&p->x, s.x); store_fe256(&p->y, s.y); store_fe256(&p->z, s.z);
}
// key-table entry -> registers
__device__ __forceinline__ affine load_table_point(const affine256 *p) { return affine_from_table(load_affine256(p)); }
// loop-form key-table entry (ec.h: affine_limbs) -> the words one entry needs: x, the top limbs and the flag, and the y block
// the digit's sign picks by address
__device__ __forceinline__ limbs_entry load_limbs_entry(const affine_limbs *p, bool neg) {
    const u32x4 *q = reinterpret_cast<const u32x4 *>(p);
    const u32x4 *qy = q + (neg ? LIMBS_NEG_Y / 4 : LIMBS_Y / 4);
    const u32x4 a = q[0], b = q[1], c = q[2], d = qy[0], e = qy[1];
    limbs_entry r;
    r.head[0] = a.x; r.head[1] = a.y; r.head[2] = a.z; r.head[3] = a.w;
    r.head[4] = b.x; r.head[5] = b.y; r.head[6] = b.z; r.head[7] = b.w;
    r.head[8] = c.x; r.head[9] = c.y; r.head[10] = c.z; r.head[11] = c.w;
    r.ysel[0] = d.x; r.ysel[1] = d.y; r.ysel[2] = d.z; r.ysel[3] = d.w;
    r.ysel[4] = e.x; r.ysel[5] = e.y; r.ysel[6] = e.z; r.ysel[7] = e.w;
    return r;
}
// what k_accum0 keeps of a table entry between its load and its use, by the table's form
__device__ __forceinline__ affine256 load_accum_entry(const affine256 *tables, u32 pay) { return load_affine256(tables + (pay & 0x7fffffffu)); }
__device__ __forceinline__ limbs_entry load_accum_entry(const affine_limbs *tables, u32 pay) {
    return load_limbs_entry(tables + (pay & 0x7fffffffu), (pay >> 31) != 0);
}
__device__ __forceinline__ xyzz load_xyzz(const xyzz_mem *p) {
    const u32x4 *q = reinterpret_cast<const u32x4 *>(p);
    xyzz_mem m;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const u32x4 v = q[i];
        m.w[4 * i] = v.x; m.w[4 * i + 1] = v.y; m.w[4 * i + 2] = v.z; m.w[4 * i + 3] = v.w;
    }
    return xyzz_from_mem(m);
}
// The same for operands that go straight into the four-wave operations: every dword of the wide load results is moved
// into a register of its own first (coop_launder, ec_coop.h: compiler note).
__device__ __forceinline__ xyzz load_xyzz_coop(const xyzz_mem *p) {
    const u32x4 *q = reinterpret_cast<const u32x4 *>(p);
    xyzz_mem m;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const u32x4 v = q[i];
        m.w[4 * i] = coop_launder(v.x); m.w[4 * i + 1] = coop_launder(v.y); m.w[4 * i + 2] = coop_launder(v.z); m.w[4 * i + 3] = coop_launder(v.w);
    }
    return xyzz_from_mem(m);
}
__device__ __forceinline__ void store_xyzz(xyzz_mem *p, const xyzz &s) {
    const xyzz_mem m = xyzz_to_mem(s);
    u32x4 *q = reinterpret_cast<u32x4 *>(p);
#pragma unroll
    for (int i = 0; i < 9; ++i) q[i] = mk_u32x4(m.w[4 * i], m.w[4 * i + 1], m.w[4 * i + 2], m.w[4 * i + 3]);
}
__device__ __forceinline__ xyzz shfl_xyzz(const xyzz &a, int src_lane) {
    xyzz_mem m = xyzz_to_mem(a);
#pragma unroll
    for (int i = 0; i < 36; ++i) m.w[i] = __shfl(m.w[i], src_lane, WAVE);
    return xyzz_from_mem(m);
}

// ------------------------------------------------------------------ recode ----
// One thread per scalar.  Scalars arrive as Fq/Fp elements, Montgomery form when is_mont
// (the `is_mont` flag of pasta-msm's mult_pippenger_*), and are decoded with the *scalar*
// field of curve C (= field 1-C).  Signed digits d_w in [-(2^(c-1)-1), 2^(c-1)]:
//   dig[w*n + i] = |d_w| | (d_w < 0) << 31, 0 when the digit is zero.
template <int C>
__global__ void __launch_bounds__(256) k_recode(const fe256 *__restrict__ scalars, u32 n, int is_mont, u32 c, u32 W,
                                               u32 wrank, u32 wworld, u32 *__restrict__ dig) {
    latency_critical();
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe256 k = load_fe256(scalars + i);
    if (is_mont) k = fe_abi_to_integer<1 - C>(k);
    const u32 half = 1u << (c - 1);
    u32 carry = 0;
    for (u32 w = 0; w < W; ++w) {
        u32 raw = extract_bits(k, w * c, c) + carry;
        u32 mag, sign;
        if (raw > half) { mag = (1u << c) - raw; sign = 1u; carry = 1u; }
        else { mag = raw; sign = 0u; carry = 0u; }
        // window split across GPUs: this device keeps the windows w = wrank (mod wworld); the scalar is
        // recoded in full (carries cross window borders), the other digits are simply not emitted
        const bool mine = wworld <= 1 || (w % wworld) == wrank;
        dig[(size_t)w * n + i] = (mag && mine) ? (mag | (sign << 31)) : 0u;
    }
}

// Largest canonical scalar bit length in a batch (row-MSM window skipping).
template <int C>
__global__ void __launch_bounds__(256) k_max_bits(const fe256 *__restrict__ scalars, u32 n, int is_mont,
                                                 u32 *__restrict__ out_bits) {
    latency_critical();
    u32 best = 0;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        fe256 k = load_fe256(scalars + i);
        if (is_mont) k = fe_abi_to_integer<1 - C>(k);
        u32 bits = 0;
#pragma unroll
        for (int l = 0; l < 8; ++l)
            if (k.w[l]) bits = 32u * l + (32u - __clz(k.w[l]));
        best = max(best, bits);
    }
    for (int d = 32; d > 0; d >>= 1) best = max(best, (u32)__shfl_xor(best, d, WAVE));
    if ((threadIdx.x & 63) == 0 && best) atomicMax(out_bits, best);
}

// ------------------------------------------------------------ counting sort ----
// Sort key of digit (w, i):  key = group(w)*NB + |d| - 1 with group(w) = w % G; windows of
// one group share buckets because their bases are pre-shifted (table j = w / G).
// Grid (S slices of the scalar index, G groups, P parts of KB buckets).  The histogram of a
// part lives in LDS: up to 32768 counters (128 KiB) -- this is what the 160 KiB LDS buys.
struct SortShape {
    u32 n;       // scalars per MSM
    u32 B;       // MSMs in the batch (same bases); blockIdx.y = b*G + g, digits of MSM b at dig[w*B*n + b*n + i]
    u32 W, G;    // windows, bucket groups
    u32 NB;      // buckets per group
    u32 shift;   // histogram key = bucket >> shift (0: one-level sort; > 0: coarse pass of the two-level sort,
                 // NB/KB/NBT then count coarse keys, entries still carry the full bucket key)
    u32 KB;      // buckets per part (LDS counters)
    u32 per;     // scalars per slice
    u32 NBT;     // G*NB
    u32 row_len; // K2: scalars per row (0 = single MSM); keys get row*G*NB added
    u32 n_ctx;   // table stride
    u32 L0;      // entries per k_accum0 thread
};

static __global__ void __launch_bounds__(1024) k_count(const u32 *__restrict__ dig, SortShape sh, u32 *__restrict__ counts) {
    latency_critical();
    extern __shared__ u32 hist[];
    const u32 s = blockIdx.x, gy = blockIdx.y, p = blockIdx.z;
    const u32 b = gy / sh.G, g = gy - b * sh.G;
    for (u32 k = threadIdx.x; k < sh.KB; k += blockDim.x) hist[k] = 0;
    __syncthreads();
    const u32 lo = p * sh.KB;
    const u32 i0 = s * sh.per, i1 = min(sh.n, i0 + sh.per);
    for (u32 w = g; w < sh.W; w += sh.G) {
        const u32 *d = dig + ((size_t)w * sh.B + b) * sh.n;
        for (u32 i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
            const u32 mag = d[i] & 0x7fffffffu;
            const u32 rel = ((mag - 1u) >> sh.shift) - lo;  // mag = 0 (no entry) wraps far above KB
            if (rel < sh.KB) atomicAdd(&hist[rel], 1u);
        }
    }
    __syncthreads();
    u32 *out = counts + (size_t)s * sh.NBT + (size_t)gy * sh.NB + (size_t)p * sh.KB;
    for (u32 k = threadIdx.x; k < sh.KB; k += blockDim.x) out[k] = hist[k];
}

// k_recode and k_count as one launch, for a single MSM whose histogram fits one LDS part (one bucket group or coarse
// pass, <= 32768 keys): the thread that recodes a scalar also counts its digits.  One kernel boundary less on the chain
// a mid-size MSM waits for; the digit planes are still written (the scatter pass reads them).
template <int C>
__global__ void __launch_bounds__(1024) k_recode_count(const fe256 *__restrict__ scalars, int is_mont, u32 c, u32 wrank, u32 wworld, SortShape sh,
                                                      u32 *__restrict__ dig, u32 *__restrict__ counts) {
    latency_critical();
    extern __shared__ u32 hist[];
    const u32 s = blockIdx.x;
    for (u32 k = threadIdx.x; k < sh.KB; k += blockDim.x) hist[k] = 0;
    __syncthreads();
    const u32 i0 = s * sh.per, i1 = min(sh.n, i0 + sh.per);
    const u32 half = 1u << (c - 1);
    for (u32 i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
        fe256 k = load_fe256(scalars + i);
        if (is_mont) k = fe_abi_to_integer<1 - C>(k);
        u32 carry = 0;
        for (u32 w = 0; w < sh.W; ++w) {
            const u32 raw = extract_bits(k, w * c, c) + carry;
            u32 mag, sign;
            if (raw > half) { mag = (1u << c) - raw; sign = 1u; carry = 1u; }
            else { mag = raw; sign = 0u; carry = 0u; }
            const bool mine = wworld <= 1 || (w % wworld) == wrank;
            const bool live = mag && mine;
            dig[(size_t)w * sh.n + i] = live ? (mag | (sign << 31)) : 0u;
            if (live) {
                const u32 rel = (mag - 1u) >> sh.shift;
                if (rel < sh.KB) atomicAdd(&hist[rel], 1u);
            }
        }
    }
    __syncthreads();
    u32 *out = counts + (size_t)s * sh.NBT;
    for (u32 k = threadIdx.x; k < sh.KB; k += blockDim.x) out[k] = hist[k];
}

// totals[key] = sum over slices
static __global__ void __launch_bounds__(256) k_slice_totals(const u32 *__restrict__ counts, u32 S, u32 NBT,
                                                     u32 *__restrict__ totals) {
    latency_critical();
    const u32 key = blockIdx.x * blockDim.x + threadIdx.x;
    if (key >= NBT) return;
    u32 t = 0;
    for (u32 s = 0; s < S; ++s) t += counts[(size_t)s * NBT + key];
    totals[key] = t;
}

// Few keys, many slices (coarse pass of the two-level sort): one wave per key, lanes over the slices.
static __global__ void __launch_bounds__(256) k_slice_totals_w(const u32 *__restrict__ counts, u32 S, u32 NBT, u32 *__restrict__ totals) {
    latency_critical();
    const u32 key = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const u32 lane = threadIdx.x & 63;
    if (key >= NBT) return;
    u32 t = 0;
    for (u32 s = lane; s < S; s += 64) t += counts[(size_t)s * NBT + key];
    for (int d = 32; d > 0; d >>= 1) t += __shfl_down(t, d, 64);
    if (lane == 0) totals[key] = t;
}
static __global__ void __launch_bounds__(256) k_scan_finish_w(u32 *__restrict__ bucket_start, const u32 *__restrict__ tile_sums,
                                                      u32 *__restrict__ counts, u32 S, u32 NBT) {
    latency_critical();
    const u32 key = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const u32 lane = threadIdx.x & 63;
    if (key >= NBT) return;
    const u32 base = bucket_start[key] + tile_sums[key / SCAN_TILE];
    const u32 per = (S + 63) / 64, s0 = lane * per, s1 = min(S, s0 + per);   // consecutive slices per lane
    u32 mine = 0;
    for (u32 s = s0; s < s1; ++s) mine += counts[(size_t)s * NBT + key];
    u32 x = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const u32 y = __shfl_up(x, d, 64);
        if ((int)lane >= d) x += y;
    }
    u32 run = base + x - mine;
    for (u32 s = s0; s < s1; ++s) {
        u32 *p = counts + (size_t)s * NBT + key;
        const u32 t = *p;
        *p = run;
        run += t;
    }
    if (lane == 0) bucket_start[key] = base;   // every lane of this wave read the old value above (one wave per key)
}

// Three-phase exclusive scan of `in[0..len)` -> out[0..len], out[len] = total.

__device__ __forceinline__ u32 block_exclusive_scan(u32 v, u32 *lds, u32 &total) {
    const u32 lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    u32 x = v;
    for (int d = 1; d < 64; d <<= 1) {
        u32 y = __shfl_up(x, d, WAVE);
        if ((int)lane >= d) x += y;
    }
    if (lane == 63) lds[wid] = x;
    __syncthreads();
    if (wid == 0) {
        u32 s = lane < (blockDim.x >> 6) ? lds[lane] : 0;
        u32 xs = s;
        for (int d = 1; d < 64; d <<= 1) {
            u32 y = __shfl_up(xs, d, WAVE);
            if ((int)lane >= d) xs += y;
        }
        lds[64 + lane] = xs - s;  // exclusive wave offsets
        if (lane == 63) lds[128] = xs;
    }
    __syncthreads();
    total = lds[128];
    u32 r = x - v + lds[64 + wid];
    __syncthreads();
    return r;
}

static __global__ void __launch_bounds__(1024) k_scan_tiles(const u32 *__restrict__ in, u32 len, u32 *__restrict__ out,
                                                    u32 *__restrict__ tile_sums) {
    latency_critical();
    __shared__ u32 lds[192];
    const u32 base = blockIdx.x * SCAN_TILE + threadIdx.x * SCAN_ITEMS;
    u32 v[SCAN_ITEMS], sum = 0;
#pragma unroll
    for (u32 k = 0; k < SCAN_ITEMS; ++k) {
        v[k] = (base + k < len) ? in[base + k] : 0;
        sum += v[k];
    }
    u32 total;
    u32 ex = block_exclusive_scan(sum, lds, total);
#pragma unroll
    for (u32 k = 0; k < SCAN_ITEMS; ++k) {
        if (base + k < len) out[base + k] = ex;
        ex += v[k];
    }
    if (threadIdx.x == 0) tile_sums[blockIdx.x] = total;
}

// single block: exclusive scan of up to 1024 tile sums (len <= 4 Mi), writes grand total
static __global__ void __launch_bounds__(1024) k_scan_tile_sums(u32 *__restrict__ tile_sums, u32 ntiles,
                                                        u32 *__restrict__ grand_total) {
    latency_critical();
    __shared__ u32 lds[192];
    u32 v = threadIdx.x < ntiles ? tile_sums[threadIdx.x] : 0;
    u32 total;
    u32 ex = block_exclusive_scan(v, lds, total);
    if (threadIdx.x < ntiles) tile_sums[threadIdx.x] = ex;
    if (threadIdx.x == 0) *grand_total = total;
}

// bucket_start[key] += tile prefix; counts[s][key] -> running cursor base per slice
static __global__ void __launch_bounds__(256) k_scan_finish(u32 *__restrict__ bucket_start, const u32 *__restrict__ tile_sums,
                                                    u32 *__restrict__ counts, u32 S, u32 NBT) {
    latency_critical();
    const u32 key = blockIdx.x * blockDim.x + threadIdx.x;
    if (key >= NBT) return;
    u32 run = bucket_start[key] + tile_sums[key / SCAN_TILE];
    bucket_start[key] = run;
    for (u32 s = 0; s < S; ++s) {
        u32 *p = counts + (size_t)s * NBT + key;
        u32 t = *p;
        *p = run;
        run += t;
    }
}

// Small key spaces (mid-size MSMs, the coarse pass of the two-level sort): slice totals, the exclusive scan and the
// per-slice cursors in ONE workgroup -- the four-kernel scan above costs ~20 us of launches for 4096 keys.  Thread i
// owns the four keys 4i..4i+3 and reads them from every slice as one 16-byte load, all slices in flight together
// (NBT <= 4096, a multiple of 4; S <= SCAN_SMALL_SLICES, msm_plan.h).
static __global__ void __launch_bounds__(1024) k_scan_small(u32 *__restrict__ counts, u32 S, u32 NBT, u32 *__restrict__ bucket_start) {
    latency_critical();
    __shared__ u32 lds[192];
    const u32 k0 = threadIdx.x * 4u;
    const bool mine = k0 < NBT;
    u32x4 tot = mk_u32x4(0, 0, 0, 0);
    if (mine) {
#pragma unroll 8
        for (u32 s = 0; s < S; ++s) {                  // independent 16-byte loads, eight in flight
            const u32x4 c = *reinterpret_cast<const u32x4 *>(counts + (size_t)s * NBT + k0);
            tot.x += c.x; tot.y += c.y; tot.z += c.z; tot.w += c.w;
        }
    }
    u32 total;
    const u32 base = block_exclusive_scan(tot.x + tot.y + tot.z + tot.w, lds, total);
    if (mine) {
        u32x4 run = mk_u32x4(base, base + tot.x, base + tot.x + tot.y, base + tot.x + tot.y + tot.z);
        *reinterpret_cast<u32x4 *>(bucket_start + k0) = run;
#pragma unroll 8
        for (u32 s = 0; s < S; ++s) {                  // second read of the same lines (L2), the store carries the running cursor
            u32x4 *p = reinterpret_cast<u32x4 *>(counts + (size_t)s * NBT + k0);
            const u32x4 c = *p;
            *p = run;
            run.x += c.x; run.y += c.y; run.z += c.z; run.w += c.w;
        }
    }
    if (threadIdx.x == 0) bucket_start[NBT] = total;
}

// COMPACT (first level of the two-level sort only): an entry is ONE word -- the low `shift` key bits, the point index above them,
// the sign on top -- because its bin says the rest of the key; k_fine_scatter puts the 8-byte form back together.  Half the
// bytes of the level the second level reads twice.  Needs index bits + shift + 1 <= 32.
template <bool COMPACT>
static __global__ void __launch_bounds__(1024) k_scatter(const u32 *__restrict__ dig, SortShape sh,
                                                 const u32 *__restrict__ cursors, void *__restrict__ entries_) {
    latency_critical();
    extern __shared__ u32 cur[];
    const u32 s = blockIdx.x, gy = blockIdx.y, p = blockIdx.z;
    const u32 b = gy / sh.G, g = gy - b * sh.G;
    const u32 *in = cursors + (size_t)s * sh.NBT + gy * sh.NB + p * sh.KB;
    for (u32 k = threadIdx.x; k < sh.KB; k += blockDim.x) cur[k] = in[k];
    __syncthreads();
    const u32 lo = p * sh.KB;
    const u32 key_base = (gy * sh.NB) << sh.shift;     // first bucket key of this group
    const u32 i0 = s * sh.per, i1 = min(sh.n, i0 + sh.per);
    u32 j = 0;
    for (u32 w = g; w < sh.W; w += sh.G, ++j) {
        const u32 *d = dig + ((size_t)w * sh.B + b) * sh.n;
        for (u32 i = i0 + threadIdx.x; i < i1; i += blockDim.x) {
            const u32 v = __builtin_nontemporal_load(d + i);   // streamed once: leave the cache to the scattered writes
            const u32 bucket = (v & 0x7fffffffu) - 1u;
            const u32 rel = (bucket >> sh.shift) - lo;
            if (rel < sh.KB) {
                const u32 pos = atomicAdd(&cur[rel], 1u);
                if constexpr (COMPACT)
                    static_cast<u32 *>(entries_)[pos] = (bucket & ((1u << sh.shift) - 1u)) | ((j * sh.n_ctx + i) << sh.shift) | (v & 0x80000000u);
                else
                    static_cast<u32x2 *>(entries_)[pos] = mk_u32x2(key_base + bucket, (j * sh.n_ctx + i) | (v & 0x80000000u));
            }
        }
    }
}

// ---- second level of the two-level sort (large MSMs) ---------------------------------------
// The one-level scatter writes every 8-byte entry to its own place among 2^(c-1) buckets: a 32-byte
// HBM sector per entry (4x the payload) that also slows the accumulation of the MSMs it overlaps
// with.  Two levels keep every write inside a run that one workgroup fills within a short time, so
// the L2 merges them into full lines: level 1 (k_count/k_scatter with shift > 0) partitions the
// entries into coarse bins of FINE = 2^shift buckets; level 2 sorts each bin by the low key bits.
// A bin is cut into segments of <= SORT_SEG entries, one workgroup each (a giant bucket -- witness-like
// scalars -- simply becomes many segments).
__device__ __forceinline__ u32 ceil_div_u32(u32 a, u32 b) { return (a + b - 1u) / b; }

// seg_first[bin] = number of segments of all earlier bins (exclusive scan of ceil(count/SORT_SEG)); one workgroup.
static __global__ void __launch_bounds__(1024) k_seg_plan(const u32 *__restrict__ bin_start, u32 nbins, u32 *__restrict__ seg_first) {
    latency_critical();
    __shared__ u32 lds[192];
    __shared__ u32 carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (u32 base = 0; base < nbins; base += blockDim.x) {
        const u32 bin = base + threadIdx.x;
        const u32 v = bin < nbins ? ceil_div_u32(bin_start[bin + 1] - bin_start[bin], SORT_SEG) : 0u;
        u32 total;
        const u32 ex = block_exclusive_scan(v, lds, total);
        if (bin < nbins) seg_first[bin] = carry + ex;
        __syncthreads();
        if (threadIdx.x == 0) carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) seg_first[nbins] = carry;
}

// segment index -> (bin, first entry, one past the last entry); false when seg is beyond the plan
__device__ __forceinline__ bool seg_lookup(const u32 *__restrict__ bin_start, const u32 *__restrict__ seg_first, u32 nbins, u32 seg,
                                           u32 &bin, u32 &e0, u32 &e1) {
    if (seg >= seg_first[nbins]) return false;
    u32 lo = 0, hi = nbins;                    // last bin with seg_first[bin] <= seg (empty bins share a value: take the last)
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (seg_first[mid] <= seg) lo = mid; else hi = mid;
    }
    bin = lo;
    e0 = bin_start[bin] + (seg - seg_first[bin]) * SORT_SEG;
    e1 = min(e0 + SORT_SEG, bin_start[bin + 1]);
    return true;
}

// seg_counts[seg][f] = entries of the segment whose key has low bits f.  LDS: FINE counters.
template <bool COMPACT>
static __global__ void __launch_bounds__(1024) k_fine_count(const void *__restrict__ in_, const u32 *__restrict__ bin_start,
                                                    const u32 *__restrict__ seg_first, u32 nbins, u32 shift, u32 *__restrict__ seg_counts) {
    latency_critical();
    extern __shared__ u32 hist[];
    const u32 fine = 1u << shift;
    u32 bin, e0, e1;
    if (!seg_lookup(bin_start, seg_first, nbins, blockIdx.x, bin, e0, e1)) return;
    for (u32 k = threadIdx.x; k < fine; k += blockDim.x) hist[k] = 0;
    __syncthreads();
    for (u32 e = e0 + threadIdx.x; e < e1; e += 4 * blockDim.x) {      // four loads in flight
        u32 k[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            k[u] = 0xffffffffu;
            if (e + u * blockDim.x < e1) {
                if constexpr (COMPACT) k[u] = static_cast<const u32 *>(in_)[e + u * blockDim.x];
                else k[u] = static_cast<const u32x2 *>(in_)[e + u * blockDim.x].x;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (e + u * blockDim.x < e1) atomicAdd(&hist[k[u] & (fine - 1u)], 1u);
    }
    __syncthreads();
    for (u32 k = threadIdx.x; k < fine; k += blockDim.x) seg_counts[(size_t)blockIdx.x * fine + k] = hist[k];
}

// One workgroup per bin, one thread per low-bits value (FINE <= 1024): bucket_start of the bin's
// buckets, and seg_counts turned into the segments' write cursors.
static __global__ void __launch_bounds__(1024) k_fine_offsets(const u32 *__restrict__ bin_start, const u32 *__restrict__ seg_first, u32 nbins,
                                                      u32 shift, u32 *__restrict__ seg_counts, u32 *__restrict__ bucket_start) {
    latency_critical();
    __shared__ u32 lds[192];
    const u32 bin = blockIdx.x, f = threadIdx.x, fine = 1u << shift;
    const u32 s0 = seg_first[bin], s1 = seg_first[bin + 1];
    u32 tot = 0;
    for (u32 sg = s0; sg < s1; ++sg) tot += seg_counts[(size_t)sg * fine + f];
    u32 total;
    const u32 ex = block_exclusive_scan(tot, lds, total);
    u32 run = bin_start[bin] + ex;
    bucket_start[(size_t)bin * fine + f] = run;
    for (u32 sg = s0; sg < s1; ++sg) {
        u32 *p = seg_counts + (size_t)sg * fine + f;
        const u32 t = *p;
        *p = run;
        run += t;
    }
    if (bin == 0 && f == 0) bucket_start[(size_t)nbins * fine] = bin_start[nbins];
}

// WORD (round 4): the sorted entries are ONE word too -- the payload alone (table index * n + point index, sign on top).  The
// list is bucket-ordered and bucket_start[] says where every bucket begins, so k_accum0<.., WORD> finds its keys there: 67 MB
// less written here and 67 MB less read there per 2^20-point MSM.
template <bool COMPACT, bool WORD = false>
static __global__ void __launch_bounds__(1024) k_fine_scatter(const void *__restrict__ in_, const u32 *__restrict__ bin_start,
                                                      const u32 *__restrict__ seg_first, u32 nbins, u32 shift,
                                                      const u32 *__restrict__ seg_cursors, void *__restrict__ out_) {
    latency_critical();
    extern __shared__ u32 cur[];
    const u32 fine = 1u << shift;
    u32 bin, e0, e1;
    if (!seg_lookup(bin_start, seg_first, nbins, blockIdx.x, bin, e0, e1)) return;
    for (u32 k = threadIdx.x; k < fine; k += blockDim.x) cur[k] = seg_cursors[(size_t)blockIdx.x * fine + k];
    __syncthreads();
    for (u32 e = e0 + threadIdx.x; e < e1; e += 4 * blockDim.x) {      // four loads in flight
        u32x2 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            v[u] = mk_u32x2(0, 0);
            if (e + u * blockDim.x < e1) {
                if constexpr (COMPACT) {
                    const u32 w = static_cast<const u32 *>(in_)[e + u * blockDim.x];
                    v[u] = mk_u32x2((bin << shift) | (w & (fine - 1u)), ((w & 0x7fffffffu) >> shift) | (w & 0x80000000u));
                } else {
                    v[u] = static_cast<const u32x2 *>(in_)[e + u * blockDim.x];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (e + u * blockDim.x < e1) {
                const u32 pos = atomicAdd(&cur[v[u].x & (fine - 1u)], 1u);
                if constexpr (WORD) static_cast<u32 *>(out_)[pos] = v[u].y;
                else static_cast<u32x2 *>(out_)[pos] = v[u];
            }
    }
}

// K2 (batched row MSM with shared bases): one workgroup sorts a block of whole rows.
// key = (row*G + group)*NB + |d| - 1; the LDS histogram covers rows_per_block*G*NB keys,
// no other workgroup touches them, so counts are final (S = 1).
struct RowSortShape {
    u32 rows, row_len;  // scalars = rows*row_len
    u32 W, G, NB;
    u32 rows_per_block;
    u32 n_ctx, L0;
};

static __global__ void __launch_bounds__(1024) k_row_count(const u32 *__restrict__ dig, RowSortShape sh, u32 *__restrict__ counts) {
    latency_critical();
    extern __shared__ u32 hist[];
    const u32 r0 = blockIdx.x * sh.rows_per_block;
    const u32 nrows = min(sh.rows_per_block, sh.rows - r0);
    const u32 nkeys = nrows * sh.G * sh.NB;
    for (u32 k = threadIdx.x; k < nkeys; k += blockDim.x) hist[k] = 0;
    __syncthreads();
    const size_t n = (size_t)sh.rows * sh.row_len;
    const u32 cnt = nrows * sh.row_len;
    for (u32 w = 0; w < sh.W; ++w) {
        const u32 *d = dig + (size_t)w * n + (size_t)r0 * sh.row_len;
        const u32 g = w % sh.G;
        for (u32 e = threadIdx.x; e < cnt; e += blockDim.x) {
            const u32 mag = d[e] & 0x7fffffffu;
            if (mag) atomicAdd(&hist[((e / sh.row_len) * sh.G + g) * sh.NB + mag - 1u], 1u);
        }
    }
    __syncthreads();
    u32 *out = counts + (size_t)r0 * sh.G * sh.NB;
    for (u32 k = threadIdx.x; k < nkeys; k += blockDim.x) out[k] = hist[k];
}

static __global__ void __launch_bounds__(1024) k_row_scatter(const u32 *__restrict__ dig, RowSortShape sh,
                                                     const u32 *__restrict__ bucket_start, u32x2 *__restrict__ entries) {
    latency_critical();
    extern __shared__ u32 cur[];
    const u32 r0 = blockIdx.x * sh.rows_per_block;
    const u32 nrows = min(sh.rows_per_block, sh.rows - r0);
    const u32 nkeys = nrows * sh.G * sh.NB;
    const u32 key0 = r0 * sh.G * sh.NB;
    for (u32 k = threadIdx.x; k < nkeys; k += blockDim.x) cur[k] = bucket_start[key0 + k];
    __syncthreads();
    const size_t n = (size_t)sh.rows * sh.row_len;
    const u32 cnt = nrows * sh.row_len;
    for (u32 w = 0; w < sh.W; ++w) {
        const u32 *d = dig + (size_t)w * n + (size_t)r0 * sh.row_len;
        const u32 g = w % sh.G, j = w / sh.G;
        for (u32 e = threadIdx.x; e < cnt; e += blockDim.x) {
            const u32 v = d[e];
            const u32 mag = v & 0x7fffffffu;
            if (mag) {
                const u32 row = e / sh.row_len, col = e - row * sh.row_len;
                const u32 rel = (row * sh.G + g) * sh.NB + mag - 1u;
                const u32 pos = atomicAdd(&cur[rel], 1u);
                entries[pos] = mk_u32x2(key0 + rel, (j * sh.n_ctx + col) | (v & 0x80000000u));
            }
        }
    }
}

// ------------------------------------------------------- bucket accumulation ----
// (defined with k_merge_chunks below; k_accum0<C, true> runs it on its own registers)
template <int C, bool COOP>
__device__ __forceinline__ void merge_wave(u32 ka, u32 kb, xyzz v, xyzz bv, u32 wave_id, int lane, int role, CoopLds *L,
                                           xyzz_mem *__restrict__ bucket_acc, u32 *__restrict__ out_keys, xyzz_mem *__restrict__ out_vals);

// Output protocol shared by k_accum0 and k_accumN.  A chunk (L0 entries of one thread, or
// the 64 slots of one wave) owns two output slots A = 2*chunk, B = 2*chunk+1:
//   run closed on both sides            -> bucket_acc[key] (final, written exactly once)
//   run continues from the left only    -> slot A
//   run continues to the right only     -> slot B
//   run continues on both sides         -> slot A, and slot B = (key, identity) filler
// so that in the next level's list the slots of one bucket are always contiguous.

// FUSED (mid-size inputs, one wave per SIMD): the first merge level runs at the end of the same kernel on the slots still
// held on chip -- the leading-run sum waits in LDS (it is produced early in the chunk), the trailing-run sum is the
// accumulator the loop ends with -- and the kernel writes what k_merge_chunks<C, false> would have written (out_* are then
// the level-1 lists).  One launch, one kernel boundary and one round trip of the partial list less per MSM.
// WORD: entries are payloads only (k_fine_scatter<.., true>); the key of a position p is the bucket b with
// bucket_start[b] <= p < bucket_start[b + 1]: one binary search per chunk (the table is 256 KiB: L2) and one load per run.
// last bucket b <= hi_incl with bs[b] <= p (bs is non-decreasing, bs[0] = 0)
__device__ __forceinline__ u32 bucket_of(const u32 *__restrict__ bs, u32 nbt, u32 p) {
    u32 lo = 0, hi = nbt;
    while (hi - lo > 1) {
        const u32 mid = (lo + hi) >> 1;
        if (bs[mid] <= p) lo = mid; else hi = mid;
    }
    return lo;
}
// TABLE: affine256 -- the packed key tables: every entry is unpacked, and negated when its digit is negative, in the loop; or
// affine_limbs -- a pre-shifted key's loop-form tables (Key::limb_tables): the entry's operand is loaded as it stands, its sign
// picks the y block by address and the record's flag word says whether the point is the identity.  Same operands bit for bit.
template <int C, bool FUSED, bool WORD = false, typename TABLE = affine256>
__global__ void __launch_bounds__(256) k_accum0(const TABLE *__restrict__ tables, const void *__restrict__ entries_,
                                               const u32 *__restrict__ m_ptr, u32 L0,
                                               u32 nchunks, xyzz_mem *__restrict__ bucket_acc, u32 *__restrict__ out_keys,
                                               xyzz_mem *__restrict__ out_vals, u32 nbt = 0) {
    __shared__ xyzz_mem stash[FUSED ? 256 : 1];        // FUSED: slot A of every chunk of the workgroup (36 KiB)
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if constexpr (FUSED) {
        if (((t >> 6) << 6) >= nchunks) return;        // whole waves only: every lane of a live wave takes part in the merge
    } else {
        if (t >= nchunks) return;
    }
    const u32 M = *m_ptr;
    // The host sized the grid for the worst case (every digit non-zero).  With fewer entries
    // (zero digits are never sorted in) the same threads take shorter chunks: the chain of
    // dependent additions per thread is what a sparse or mid-size MSM waits for.
    while (L0 > 8 && (u64)(L0 >> 1) * nchunks >= M) L0 >>= 1;
    const u32 start = t * L0;
    u32 key_a = KEY_INVALID, key_b = KEY_INVALID;
    xyzz tail = xyzz_identity();                       // FUSED: slot B (the trailing run's sum)
    if (t < nchunks && start < M) {
        const u32 end = min(start + L0, M);
        const u32 cnt = end - start;
        const u32x2 *mine = static_cast<const u32x2 *>(entries_) + start;       // !WORD
        const u32 *mine1 = static_cast<const u32 *>(entries_) + start;          // WORD
        const u32 *bs = m_ptr - nbt;                                            // WORD: bucket_start[0 .. nbt]
        u32 cur_key, pay, boundary = 0;
        bool lo_open, ro_open = false;               // the chunk's first run began before it / (WORD) set when the last run is closed
        u32 prev_key = KEY_INVALID, next_key = KEY_INVALID;
        if constexpr (WORD) {
            cur_key = bucket_of(bs, nbt, start);
            boundary = bs[cur_key + 1];
            lo_open = bs[cur_key] < start;
            pay = mine1[0];
        } else {
            prev_key = start > 0 ? static_cast<const u32x2 *>(entries_)[start - 1].x : KEY_INVALID;
            next_key = end < M ? static_cast<const u32x2 *>(entries_)[end].x : KEY_INVALID;
            const u32x2 e0 = mine[0];
            cur_key = e0.x;
            pay = e0.y;
            lo_open = prev_key == cur_key;
        }
        auto raw = load_accum_entry(tables, pay);
        xyzz acc = xyzz_identity();
        bool acc_empty = true;
        bool first_run = true;
        for (u32 k = 0; k < cnt; ++k) {
            // prefetch the next entry while this one is being added.  The chunk's last entry fetches itself once more (one load
            // in L0, never used): with the loads under a branch the registers they land in were copied from the current entry's
            // first, every iteration, for the one in which nothing is loaded.
            const u32 kn = k + 1 < cnt ? k + 1 : k;
            u32 nkey = cur_key, npay;
            if constexpr (WORD) {
                npay = mine1[kn];
                if (k + 1 < cnt && start + k + 1 == boundary) {                // the next entry opens another bucket
                    nkey = cur_key + 1;
                    if (bs[nkey + 1] == boundary) nkey = bucket_of(bs, nbt, boundary);   // empty buckets in between (sparse digits)
                }
            } else {
                const u32x2 e = mine[kn];
                nkey = e.x;                                                    // (its own key again at the chunk's end)
                npay = e.y;
            }
            const auto nraw = load_accum_entry(tables, npay);
            if constexpr (std::is_same<TABLE, affine_limbs>::value) {
                bool pt_inf;
                const affine pt = affine_from_limbs(raw, (pay >> 31) != 0, &pt_inf);
                acc = xyzz_madd_flags<C>(acc, acc_empty, pt, pt_inf);
            } else {
                affine pt = affine_from_table(raw);
                pt.y = fe_select((pay >> 31) != 0 && !affine_is_inf(pt), fe_neg<C, 2>(pt.y), pt.y);
                acc = xyzz_madd_flag<C>(acc, acc_empty, pt);
            }
            acc_empty = false;
            const bool last = (k + 1 == cnt);
            if (last || nkey != cur_key) {
                const bool lo = first_run && lo_open;
                bool ro;
                if constexpr (WORD) ro = last && boundary > end;
                else ro = last && next_key == cur_key;
                if (!lo && !ro) {
                    store_xyzz(bucket_acc + cur_key, acc);
                } else if (lo) {
                    if constexpr (FUSED) store_xyzz(&stash[threadIdx.x], acc);
                    else store_xyzz(out_vals + 2 * (size_t)t, acc);
                    key_a = cur_key;
                    if (ro) {
                        if constexpr (!FUSED) store_xyzz(out_vals + 2 * (size_t)t + 1, xyzz_identity());
                        key_b = cur_key;
                    }
                } else {
                    if constexpr (FUSED) tail = acc;
                    else store_xyzz(out_vals + 2 * (size_t)t + 1, acc);
                    key_b = cur_key;
                }
                first_run = false;
                acc = xyzz_identity();
                acc_empty = true;
                if constexpr (WORD) { if (!last) boundary = bs[nkey + 1]; }
            }
            cur_key = nkey; pay = npay; raw = nraw;
        }
        (void)ro_open; (void)prev_key;
    }
    if constexpr (FUSED) {
        latency_critical();                            // from here on the wave is a tail: a chain of dependent additions
        xyzz v = xyzz_identity();
        if (key_a != KEY_INVALID) v = load_xyzz(&stash[threadIdx.x]);      // written by this very thread: no barrier needed
        merge_wave<C, false>(key_a, key_b, v, tail, t >> 6, (int)(threadIdx.x & 63), 0, nullptr, bucket_acc, out_keys, out_vals);
    } else {
        out_keys[2 * (size_t)t] = key_a;
        out_keys[2 * (size_t)t + 1] = key_b;
    }
}

// One slot per lane; segmented reduction over equal keys with wave shuffles; steps in which
// no lane of the wave has a partner are skipped, so sparse lists cost next to nothing.
template <int C>
__global__ void __launch_bounds__(256) k_accumN(const u32 *__restrict__ in_keys, const xyzz_mem *__restrict__ in_vals,
                                               u32 len, xyzz_mem *__restrict__ bucket_acc, u32 *__restrict__ out_keys,
                                               xyzz_mem *__restrict__ out_vals) {
    latency_critical();
    const u32 gid = blockIdx.x * blockDim.x + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const u32 wave_id = gid >> 6;
    const u32 wave_first = gid - lane;
    if (wave_first >= len) return;  // whole wave out of range (grid is sized in waves)
    const u32 key = gid < len ? in_keys[gid] : KEY_INVALID;
    const bool valid = key != KEY_INVALID;
    if (!__any(valid)) {
        if (lane == 0) { out_keys[2 * (size_t)wave_id] = KEY_INVALID; out_keys[2 * (size_t)wave_id + 1] = KEY_INVALID; }
        return;
    }
    xyzz v = xyzz_identity();
    if (valid) v = load_xyzz(in_vals + gid);
    for (int d = 1; d < 64; d <<= 1) {
        const u32 pk = __shfl_down(key, d, WAVE);
        const bool need = valid && (lane + d < 64) && pk == key;
        if (__any(need)) {
            xyzz o = shfl_xyzz(v, (lane + d) & 63);
            xyzz s = xyzz_add<C>(v, o);
            v = xyzz_select(need, s, v);
        }
    }
    const u32 key_up = __shfl_up(key, 1, WAVE);
    const bool is_head = valid && (lane == 0 || key_up != key);
    const u32 key63 = __shfl(key, 63, WAVE);
    const u32 prev_key = wave_first > 0 ? in_keys[wave_first - 1] : KEY_INVALID;
    const u32 next_key = wave_first + 64 < len ? in_keys[wave_first + 64] : KEY_INVALID;
    if (is_head) {
        const bool lo = (lane == 0) && prev_key == key;
        const bool ro = (key63 == key) && next_key == key;
        if (!lo && !ro) {
            store_xyzz(bucket_acc + key, v);
        } else if (lo) {
            store_xyzz(out_vals + 2 * (size_t)wave_id, v);
            if (ro) store_xyzz(out_vals + 2 * (size_t)wave_id + 1, xyzz_identity());
        } else {
            store_xyzz(out_vals + 2 * (size_t)wave_id + 1, v);
        }
    }
    if (lane == 0) {
        out_keys[2 * (size_t)wave_id] = (valid && prev_key == key) ? key : KEY_INVALID;
        out_keys[2 * (size_t)wave_id + 1] = (key63 != KEY_INVALID && next_key == key63) ? key63 : KEY_INVALID;
    }
}

// First level of the partial merge, one CHUNK per lane.  k_accum0 leaves two slots per chunk: A = its leading run
// if that run continues from the chunk on the left, B = its trailing run if that run continues to the right (for a
// chunk that is one run open on both sides the sum is in A and B only repeats the key).  k_accumN spends a lane per
// SLOT, so half its lanes hold such repeats; here a lane takes both slots of its chunk: a trailing run that starts
// inside chunk i (a "real" B) is handed to lane i + 1, where it meets the leading run A of the same bucket, and what
// remains is the plain segmented sum over the A's -- half the waves and one level less per run than before.
// Output: the same two-slot protocol per wave (64 chunks), consumed by k_accumN / k_accumN_coop.
// COOP: one workgroup (four waves sharing each addition) per 64 chunks; otherwise four independent waves per workgroup.
// The body of the first merge level for ONE wave of 64 chunks whose two slots (ka, v) / (kb, bv) are in registers: used by
// k_merge_chunks (slots loaded from the partial list) and by k_accum0<C, true> (slots still in the accumulation's registers).
// COOP: the four waves of the workgroup hold the same 64 chunks and share each addition (L, role).
template <int C, bool COOP>
__device__ __forceinline__ void merge_wave(u32 ka, u32 kb, xyzz v, xyzz bv, u32 wave_id, int lane, int role, CoopLds *L,
                                           xyzz_mem *__restrict__ bucket_acc, u32 *__restrict__ out_keys, xyzz_mem *__restrict__ out_vals) {
    const bool has_a = ka != KEY_INVALID;
    const bool interior = has_a && kb == ka;           // one run, open on both sides: the sum is in A
    const bool has_b = kb != KEY_INVALID && !interior; // a trailing run that starts inside this chunk
    if (!__any(has_a || has_b)) {
        if (lane == 0 && (!COOP || role == 0)) { out_keys[2 * (size_t)wave_id] = KEY_INVALID; out_keys[2 * (size_t)wave_id + 1] = KEY_INVALID; }
        return;
    }
    // a real B belongs to the bucket whose leading run sits in the next lane
    const int b_before = __shfl_up(has_b ? 1 : 0, 1, WAVE);   // every lane takes part in a shuffle: never inside a short-circuit
    const bool recv = lane > 0 && b_before != 0;
    for (int step = 0; step < 7; ++step) {              // step 0: A += B of the lane before; steps 1..6: segmented sum over equal keys
        const int d = step == 0 ? 63 : 1 << (step - 1);  // source lane = lane + d (mod 64)
        const u32 ka_d = __shfl(ka, (lane + d) & 63, WAVE);
        bool need;
        if (step == 0) need = recv;
        else need = has_a && lane + d < 64 && ka_d == ka;
        if (__any(need)) {
            const xyzz o = shfl_xyzz(step == 0 ? bv : v, (lane + d) & 63);
            xyzz sum;
            if constexpr (COOP) sum = xyzz_add_coop<C>(v, o, *L, role, lane);
            else sum = xyzz_add<C>(v, o);
            v = xyzz_select(need, sum, v);
        }
    }
    const u32 ka_up = __shfl_up(ka, 1, WAVE);
    const bool is_head = has_a && (lane == 0 || ka_up != ka);
    const u32 ka63 = __shfl(ka, 63, WAVE);
    const bool interior63 = __shfl(interior ? 1 : 0, 63, WAVE) != 0;
    const bool hasb63 = __shfl(has_b ? 1 : 0, 63, WAVE) != 0;
    const u32 kb63 = __shfl(kb, 63, WAVE);
    const u32 ka0 = __shfl(ka, 0, WAVE);
    if (COOP && role != 0) return;
    if (is_head) {
        const bool lo = lane == 0;                      // a leading run in lane 0 continues from the wave before
        const bool ro = interior63 && ka63 == ka;       // the segment runs through the last chunk and beyond
        if (!lo && !ro) {
            store_xyzz(bucket_acc + ka, v);
        } else if (lo) {
            store_xyzz(out_vals + 2 * (size_t)wave_id, v);
            if (ro) store_xyzz(out_vals + 2 * (size_t)wave_id + 1, xyzz_identity());
        } else {
            store_xyzz(out_vals + 2 * (size_t)wave_id + 1, v);
        }
    }
    if (lane == 63 && has_b) store_xyzz(out_vals + 2 * (size_t)wave_id + 1, bv);   // a run that starts in the last chunk
    if (lane == 0) {
        out_keys[2 * (size_t)wave_id] = ka0;            // valid exactly when lane 0 holds a leading run
        out_keys[2 * (size_t)wave_id + 1] = interior63 ? ka63 : (hasb63 ? kb63 : KEY_INVALID);
    }
}

template <int C, bool COOP>
__global__ void __launch_bounds__(256) k_merge_chunks(const u32 *__restrict__ in_keys, const xyzz_mem *__restrict__ in_vals, u32 nchunks,
                                                     xyzz_mem *__restrict__ bucket_acc, u32 *__restrict__ out_keys, xyzz_mem *__restrict__ out_vals) {
    latency_critical();
    __shared__ CoopLds L;
    const int lane = threadIdx.x & 63, role = threadIdx.x >> 6;
    const u32 wave_id = COOP ? blockIdx.x : blockIdx.x * 4u + (u32)role;
    const u32 first = wave_id * 64u;
    if (first >= nchunks) return;                      // COOP: the whole workgroup leaves together
    const u32 t = first + lane;
    const bool in_range = t < nchunks;
    const u32 ka = in_range ? in_keys[2 * (size_t)t] : KEY_INVALID;
    const u32 kb = in_range ? in_keys[2 * (size_t)t + 1] : KEY_INVALID;
    const bool has_a = ka != KEY_INVALID;
    const bool has_b = kb != KEY_INVALID && !(has_a && kb == ka);
    xyzz v = xyzz_identity(), bv = xyzz_identity();
    if (has_a) v = load_xyzz_coop(in_vals + 2 * (size_t)t);
    if (has_b) bv = load_xyzz_coop(in_vals + 2 * (size_t)t + 1);
    merge_wave<C, COOP>(ka, kb, v, bv, wave_id, lane, role, &L, bucket_acc, out_keys, out_vals);
}

// ------------------------------------------------------------ bucket reduce ----
// ---- two-dimensional bucket reduction --------------------------------------------------
// sum_k (k+1)*B_k over the NB = 2^(c1+c2) buckets of a group, with k = i*2^c2 + j:
//      = 2^c2 * sum_i i*Row_i  +  sum_j j*Col_j  +  sum_i Row_i,
//   Row_i = sum_j B_{i,j} (2^c1 plain sums),  Col_j = sum_i B_{i,j} (2^c2 plain sums).
// Same two additions per bucket as a running sum, but the dependent chain is two short
// weighted sums over 2^(c/2) elements instead of one over 2^c: the tail of an MSM is a
// latency chain of ~5 us group operations, so depth is what matters.
// k_reduce_rowcol: LPS lanes per row or column sum, 64 / LPS sums per wave.  Grid: ceil(groups * (rows + cols) * LPS / 64) waves.
// LPS = 64 is one wave per sum, the shortest chain a lone wave offers (REEF_MSM_COOP=0).  LPS = 32 / 16 are the THROUGHPUT forms
// run_core takes for a large bucket matrix while the device is shared: a lane first sums its count / LPS strided elements, the lane
// tree then has log2(LPS) levels inside the sum's lane group -- fewer steps with idle lanes, and none of the exchange the four-wave
// form pays per addition.  The chain is longer (9 / 12 / 19 dependent additions at count = 256), which only a caller who waits for
// this one MSM sees.  As in k_reduce_rowcol_coop the additions go through ONE call site in a step loop (instruction cache).
template <int C, int LPS>
__global__ void __launch_bounds__(256) k_reduce_rowcol(const xyzz_mem *__restrict__ bucket_acc,
                                                      const u32 *__restrict__ bucket_start, u32 c1, u32 c2, u32 groups,
                                                      xyzz_mem *__restrict__ rowcol) {
    static_assert(LPS == 64 || LPS == 32 || LPS == 16, "lanes per sum");
    latency_critical();
    constexpr u32 SPW = 64 / LPS;                      // sums per wave
    const u32 rows = 1u << c1, cols = 1u << c2, per_group = rows + cols, sums = groups * per_group;
    const u32 wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int lane = threadIdx.x & 63, l = lane & (LPS - 1);      // l: the lane's place in its sum's group
    if (wave * SPW >= sums) return;                    // the whole wave leaves together
    const u32 sum = wave * SPW + (u32)lane / LPS;
    const bool valid = sum < sums;                     // the last wave may hold fewer than SPW sums
    const u32 g = sum / per_group, idx = sum - g * per_group;
    const bool is_row = idx < rows;
    const u32 key0 = g << (c1 + c2);
    const u32 count = valid ? (is_row ? cols : rows) : 0u;        // elements of this lane's sum (rows and columns may share a wave)
    const u32 first = is_row ? key0 + (idx << c2) : key0 + (idx - rows);
    const u32 stride = is_row ? 1u : cols;
    xyzz acc = xyzz_identity();
    bool live = false;
    const u32 nload = (max(rows, cols) + LPS - 1) / LPS;          // the longer of the two chains, the same for every wave
    u32 levels = 0;
    while ((1u << levels) < LPS) ++levels;
    for (u32 step = 0; step < nload + levels; ++step) {            // nload rounds of bucket loads, then the levels of the lane tree
        xyzz o = xyzz_identity();
        bool take;
        if (step < nload) {
            const u32 e = step * LPS + (u32)l;
            const u32 key = first + e * stride;
            take = e < count && bucket_start[key + 1] != bucket_start[key];
            if (take) o = load_xyzz(bucket_acc + key);
        } else {
            const int d = (LPS / 2) >> (step - nload);
            const bool o_live = __shfl(live ? 1 : 0, (lane + d) & 63, WAVE) != 0;
            take = l < d && o_live;                    // l < d: lane + d is a lane of the same sum
            if (__any(take)) o = shfl_xyzz(acc, (lane + d) & 63);
        }
        if (__any(take)) {
            if (__any(take && live)) {
                const xyzz s = xyzz_add<C>(acc, o);
                acc = xyzz_select(take, live ? s : o, acc);
            } else {
                acc = xyzz_select(take, o, acc);
            }
            live = live || take;
        }
    }
    if (valid && l == 0) store_xyzz(rowcol + (size_t)g * per_group + idx, acc);
}

// Weighted sum  X = sum_e e*in[e]  and plain total  T = sum_e in[e]  of `count` (power of two)
// elements, computed by one wave: lane l owns s = count/64 consecutive elements (running sums),
// a suffix scan over the lanes gives sum_l l*r_l as the sum of the suffixes.
template <int C>
__device__ __forceinline__ void wave_weighted_sum(const xyzz_mem *__restrict__ in, u32 count, int lane, xyzz &X, xyzz &T) {
    const u32 s = count >= 64 ? count / 64 : 1;        // elements per lane
    const u32 lanes = count >= 64 ? 64 : count;        // lanes with work
    const bool has = (u32)lane < lanes;
    xyzz r = xyzz_identity(), a = xyzz_identity();
    if (__any(has)) {
        const u32 e0 = (u32)lane * s;
        if (has) r = load_xyzz(in + e0 + s - 1);
        a = (s > 1) ? r : xyzz_identity();
        for (int t = (int)s - 2; t >= 0; --t) {
            xyzz b = xyzz_identity();
            if (has) b = load_xyzz(in + e0 + t);
            r = xyzz_add<C>(r, b);
            if (t >= 1) a = xyzz_add<C>(a, r);
        }
    }
    // suffix sums of r over the lanes
    xyzz U = r;
    for (int d = 1; d < 64; d <<= 1) {
        if ((u32)d >= lanes) break;
        const xyzz o = shfl_xyzz(U, (lane + d) & 63);
        const xyzz sum = xyzz_add<C>(U, o);
        U = xyzz_select(lane + d < 64, sum, U);
    }
    T = U;                                             // lane 0 holds the total
    // V_l = a_l + s * U_l (l >= 1);  X = sum_l V_l
    xyzz sU = U;
    for (u32 k = 1; k < s; k <<= 1) sU = xyzz_dbl<C>(sU);
    xyzz V = a;
    if (lanes > 1) {
        const xyzz va = xyzz_add<C>(a, sU);
        V = xyzz_select(lane >= 1, va, a);
    }
    for (int d = 32; d > 0; d >>= 1) {
        if ((u32)d >= lanes) continue;
        const xyzz o = shfl_xyzz(V, (lane + d) & 63);
        const xyzz sum = xyzz_add<C>(V, o);
        V = xyzz_select(lane < d, sum, V);
    }
    X = V;                                             // lane 0 holds the weighted sum
}

// One block of 128 threads per group: wave 0 takes the rows, wave 1 the columns.  With a pre-shifted key
// (one group per result) the group sum is the result and is written as the ABI Jacobian point directly.
template <int C>
__global__ void __launch_bounds__(128) k_reduce_weighted(const xyzz_mem *__restrict__ rowcol, u32 c1, u32 c2,
                                                        xyzz_mem *__restrict__ group_sums, jacobian256 *__restrict__ direct_out) {
    latency_critical();
    __shared__ xyzz_mem lds_x;
    const u32 rows = 1u << c1, cols = 1u << c2, per_group = rows + cols;
    const u32 g = blockIdx.x;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const xyzz_mem *base = rowcol + (size_t)g * per_group;
    xyzz X, T;
    if (wid == 0) wave_weighted_sum<C>(base, rows, lane, X, T);
    else wave_weighted_sum<C>(base + rows, cols, lane, X, T);
    if (wid == 1 && lane == 0) lds_x = xyzz_to_mem(X);
    __syncthreads();
    if (threadIdx.x == 0) {
        xyzz acc = X;                                  // sum_i i*Row_i
        for (u32 k = 0; k < c2; ++k) acc = xyzz_dbl<C>(acc);
        acc = xyzz_add<C>(acc, xyzz_from_mem(lds_x));  // + sum_j j*Col_j
        acc = xyzz_add<C>(acc, T);                     // + sum of all buckets (bucket value = k + 1)
        if (direct_out) store_jacobian256(direct_out + g, xyzz_to_abi_jacobian<C>(acc));   // one group per result: this is the result
        else store_xyzz(group_sums + g, acc);
    }
}

// ---- the same tail with every group operation spread over the four waves of a workgroup (ec_coop.h) ----
// One WORKGROUP of 256 threads stands where one wave stood: its four waves hold the same 64 slots and share
// the field products of each addition / doubling through LDS, which cuts the latency of a dependent group
// operation from ~5.6 us to ~2 us.  Everything else (keys, shuffles, the output protocol) is unchanged and
// runs replicated; wave 0 does the stores.
template <int C>
__global__ void __launch_bounds__(256) k_accumN_coop(const u32 *__restrict__ in_keys, const xyzz_mem *__restrict__ in_vals,
                                                    u32 len, xyzz_mem *__restrict__ bucket_acc, u32 *__restrict__ out_keys,
                                                    xyzz_mem *__restrict__ out_vals) {
    latency_critical();
    __shared__ CoopLds L;
    const int lane = threadIdx.x & 63, role = threadIdx.x >> 6;
    const u32 wave_id = blockIdx.x;
    const u32 wave_first = wave_id * 64u, gid = wave_first + lane;
    if (wave_first >= len) return;
    const u32 key = gid < len ? in_keys[gid] : KEY_INVALID;
    const bool valid = key != KEY_INVALID;
    if (!__any(valid)) {
        if (threadIdx.x == 0) { out_keys[2 * (size_t)wave_id] = KEY_INVALID; out_keys[2 * (size_t)wave_id + 1] = KEY_INVALID; }
        return;
    }
    xyzz v = xyzz_identity();
    if (valid) v = load_xyzz_coop(in_vals + gid);
    for (int d = 1; d < 64; d <<= 1) {
        const u32 pk = __shfl_down(key, d, WAVE);
        const bool need = valid && (lane + d < 64) && pk == key;
        if (__any(need)) {
            const xyzz o = shfl_xyzz(v, (lane + d) & 63);
            const xyzz s = xyzz_add_coop<C>(v, o, L, role, lane);
            v = xyzz_select(need, s, v);
        }
    }
    const u32 key_up = __shfl_up(key, 1, WAVE);
    const bool is_head = valid && (lane == 0 || key_up != key);
    const u32 key63 = __shfl(key, 63, WAVE);
    const u32 prev_key = wave_first > 0 ? in_keys[wave_first - 1] : KEY_INVALID;
    const u32 next_key = wave_first + 64 < len ? in_keys[wave_first + 64] : KEY_INVALID;
    if (role != 0) return;
    if (is_head) {
        const bool lo = (lane == 0) && prev_key == key;
        const bool ro = (key63 == key) && next_key == key;
        if (!lo && !ro) {
            store_xyzz(bucket_acc + key, v);
        } else if (lo) {
            store_xyzz(out_vals + 2 * (size_t)wave_id, v);
            if (ro) store_xyzz(out_vals + 2 * (size_t)wave_id + 1, xyzz_identity());
        } else {
            store_xyzz(out_vals + 2 * (size_t)wave_id + 1, v);
        }
    }
    if (lane == 0) {
        out_keys[2 * (size_t)wave_id] = (valid && prev_key == key) ? key : KEY_INVALID;
        out_keys[2 * (size_t)wave_id + 1] = (key63 != KEY_INVALID && next_key == key63) ? key63 : KEY_INVALID;
    }
}

// One workgroup per row sum / column sum (k_reduce_rowcol: one wave each).  The additions of the kernel all go
// through ONE call site (a step loop): an inlined addition is ~35 KB of code, and a kernel with one site per use ran
// out of the instruction cache (the one-wave k_reduce_weighted is 580 KB).
template <int C>
__global__ void __launch_bounds__(256) k_reduce_rowcol_coop(const xyzz_mem *__restrict__ bucket_acc,
                                                           const u32 *__restrict__ bucket_start, u32 c1, u32 c2, u32 groups,
                                                           xyzz_mem *__restrict__ rowcol) {
    latency_critical();
    __shared__ CoopLds L;
    const u32 rows = 1u << c1, cols = 1u << c2, per_group = rows + cols;
    const u32 wave = blockIdx.x;
    const int lane = threadIdx.x & 63, role = threadIdx.x >> 6;
    if (wave >= groups * per_group) return;
    const u32 g = wave / per_group, idx = wave - g * per_group;
    const bool is_row = idx < rows;
    const u32 key0 = g << (c1 + c2);
    const u32 count = is_row ? cols : rows;
    const u32 first = is_row ? key0 + (idx << c2) : key0 + (idx - rows);
    const u32 stride = is_row ? 1u : cols;
    xyzz acc = xyzz_identity();
    bool live = false;
    const u32 nload = (count + 63u) / 64u;
    for (u32 step = 0; step < nload + 6u; ++step) {     // nload rounds of bucket loads, then the six levels of the lane tree
        xyzz o = xyzz_identity();
        bool take;
        if (step < nload) {
            const u32 e = step * 64u + lane;
            const u32 key = first + e * stride;
            take = e < count && bucket_start[key + 1] != bucket_start[key];
            if (take) o = load_xyzz_coop(bucket_acc + key);
        } else {
            const int d = 32 >> (step - nload);
            const bool o_live = __shfl(live ? 1 : 0, (lane + d) & 63, WAVE) != 0;
            take = lane < d && o_live;
            if (__any(take)) o = shfl_xyzz(acc, (lane + d) & 63);
        }
        if (__any(take)) {
            if (__any(take && live)) {
                const xyzz sum = xyzz_add_coop<C>(acc, o, L, role, lane);
                acc = xyzz_select(take, live ? sum : o, acc);
            } else {
                acc = xyzz_select(take, o, acc);
            }
            live = live || take;
        }
    }
    if (threadIdx.x == 0) store_xyzz(rowcol + (size_t)g * per_group + idx, acc);
}

// wave_weighted_sum with the four waves of the workgroup sharing every group operation: X = sum_e e*in[e] and
// T = sum_e in[e] over `count` (a power of two) elements, lane l owning s = count/64 consecutive ones.  Written as a
// step machine over two accumulators so that the kernel holds ONE addition site and ONE doubling site:
//   R: running sum of the lane's elements, then suffix sums over the lanes (lane 0 = T), then s * suffix sum
//   A: sum of the lane's inner running sums, then a_l + s*U_l, then the lane tree (lane 0 = X)
template <int C>
__device__ __forceinline__ void coop_weighted_sum(const xyzz_mem *__restrict__ in, u32 count, int lane, int role, CoopLds &L, xyzz &X, xyzz &T) {
    const u32 s = count >= 64 ? count / 64 : 1;        // elements per lane
    const u32 lanes = count >= 64 ? 64 : count;        // lanes with work
    const bool has = (u32)lane < lanes;
    const u32 e0 = (u32)lane * s;
    xyzz R = xyzz_identity(), A = xyzz_identity();
    if (has) R = load_xyzz_coop(in + e0 + s - 1);
    if (s > 1) A = R;
    enum { RUN_R, RUN_A, SCAN, SHIFT, JOIN, TREE, DONE };
    int phase = s > 1 ? RUN_R : SCAN;
    int t = (int)s - 2;                                // RUN_*: element index
    int d = 1;                                         // SCAN / TREE: lane distance
    u32 k = 1;                                         // SHIFT: doublings done (as a power of two)
    T = xyzz_identity();
    for (;;) {
        if (phase == SCAN && (u32)d >= lanes) { T = R; phase = s > 1 ? SHIFT : JOIN; }          // lane 0 of R is the total
        if (phase == SHIFT && k >= s) phase = JOIN;
        if (phase == JOIN && lanes <= 1) phase = TREE, d = 32;
        if (phase == JOIN && s == 1) {                 // A is still empty: the join is a copy, not an addition
            A = xyzz_select(lane >= 1, R, A);
            phase = TREE, d = 32;
        }
        if (phase == TREE) { while (d > 0 && (u32)d >= lanes) d >>= 1; if (d == 0) phase = DONE; }
        if (phase == DONE) break;
        xyzz x, y;
        bool keep = true;                              // lanes that take the result
        bool into_r = true;
        if (phase == SHIFT) {                          // R = 2*R
            x = R; y = R;
        } else if (phase == RUN_R) {                   // R += in[e0 + t]
            x = R; y = xyzz_identity();
            if (has) y = load_xyzz_coop(in + e0 + t);
        } else if (phase == RUN_A) {                   // A += R
            x = A; y = R; into_r = false;
        } else if (phase == SCAN) {                    // R += R of lane + d
            x = R; y = shfl_xyzz(R, (lane + d) & 63); keep = lane + d < 64;
        } else if (phase == JOIN) {                    // A += s * (suffix sum), lanes >= 1
            x = A; y = R; keep = lane >= 1; into_r = false;
        } else {                                       // TREE: A += A of lane + d
            x = A; y = shfl_xyzz(A, (lane + d) & 63); keep = lane < d; into_r = false;
        }
        xyzz res;                                      // the kernel's two group operation sites
        if (phase == SHIFT) res = xyzz_dbl_coop<C>(x, L, role, lane);
        else res = xyzz_add_coop<C>(x, y, L, role, lane);
        if (into_r) R = xyzz_select(keep, res, R);
        else A = xyzz_select(keep, res, A);
        if (phase == SHIFT) { k <<= 1; continue; }
        if (phase == RUN_R) { phase = t >= 1 ? RUN_A : SCAN; if (t == 0) --t; }
        else if (phase == RUN_A) { --t; phase = RUN_R; }
        else if (phase == SCAN) d <<= 1;
        else if (phase == JOIN) { phase = TREE; d = 32; }
        else d >>= 1;
        if (phase == RUN_R && t < 0) phase = SCAN;
    }
    X = A;                                             // lane 0 holds the weighted sum
}

// Grid (groups, 2): blockIdx.y = 0 the rows, 1 the columns of a group; wsum[g][2*y] = X, wsum[g][2*y + 1] = T.
template <int C>
__global__ void __launch_bounds__(256) k_reduce_weighted_coop(const xyzz_mem *__restrict__ rowcol, u32 c1, u32 c2, xyzz_mem *__restrict__ wsum) {
    latency_critical();
    __shared__ CoopLds L;
    const u32 rows = 1u << c1, cols = 1u << c2, per_group = rows + cols;
    const u32 g = blockIdx.x, y = blockIdx.y;
    const int lane = threadIdx.x & 63, role = threadIdx.x >> 6;
    const xyzz_mem *base = rowcol + (size_t)g * per_group + (y ? rows : 0u);
    xyzz X, T;
    coop_weighted_sum<C>(base, y ? cols : rows, lane, role, L, X, T);
    if (threadIdx.x == 0) {
        store_xyzz(wsum + 4 * (size_t)g + 2 * y, X);
        store_xyzz(wsum + 4 * (size_t)g + 2 * y + 1, T);
    }
}

// 2^c2 * Xrows + Xcols + Trows per group; with a pre-shifted key (one group per result) this is the result.
template <int C>
__global__ void __launch_bounds__(256) k_reduce_combine_coop(const xyzz_mem *__restrict__ wsum, u32 c2, xyzz_mem *__restrict__ group_sums,
                                                            jacobian256 *__restrict__ direct_out) {
    latency_critical();
    __shared__ CoopLds L;
    const u32 g = blockIdx.x;
    const int lane = threadIdx.x & 63, role = threadIdx.x >> 6;
    xyzz acc = load_xyzz_coop(wsum + 4 * (size_t)g);                              // sum_i i*Row_i   (every lane the same point)
    for (u32 k = 0; k < c2 + 2; ++k) {                                        // c2 doublings, then + sum_j j*Col_j, + sum of all buckets
        xyzz other = acc;
        if (k >= c2) other = load_xyzz_coop(wsum + 4 * (size_t)g + (k == c2 ? 2u : 1u));
        if (k < c2) acc = xyzz_dbl_coop<C>(acc, L, role, lane);
        else acc = xyzz_add_coop<C>(acc, other, L, role, lane);
    }
    if (threadIdx.x == 0) {
        if (direct_out) store_jacobian256(direct_out + g, xyzz_to_abi_jacobian<C>(acc));
        else store_xyzz(group_sums + g, acc);
    }
}

// ---- small MSMs over a resident key: nibble tables, no sort, no buckets -------------------------------------------
// Reef's 1- and 2-term Pedersen commitments (CE::commit with a blind, src/backend/commitment.rs:349-351,360-361,422,430)
// and the <= 2^10-point MSMs of cap_prove (commitment.rs:261-268) are too small for the bucket pipeline (a dozen
// launches, ~0.25 ms).  For a resident key of at most SMALL_N_MAX points every nibble multiple of every point is
// tabulated once,  S[(w*15 + d - 1)*n + i] = d * 16^w * P_i  (w < 64, d = 1..15; affine, key-table form; 60 KiB per
// point), and an MSM is the plain sum of the <= 64n table entries its scalars select -- no doubling at all.  One
// workgroup of four waves per SMALL_PER_BLOCK entries (each lane a few entries, then the lane tree, every addition
// shared by the four waves: ec_coop.h), a second small launch when there is more than one workgroup.
static constexpr u32 SMALL_N_MAX = 1024, SMALL_WINDOWS = 64, SMALL_DIGITS = 15, SMALL_PER_BLOCK = 512;

// S for `n` points, in two launches (k_xyzz_normalize follows): k_shift_chain leaves base[w*n + i] = 16^w * P_i (one
// thread per point, a chain of 252 doublings), k_small_fill the 15 multiples of every base (one thread per (w, i), a chain
// of 14 additions) -- 1.2 ms for any n <= 1024 where one thread per point doing both took 7 ms.  Once per key.
template <int C>
__global__ void __launch_bounds__(64) k_small_fill(const xyzz_mem *__restrict__ base, u32 n, xyzz_mem *__restrict__ out) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * SMALL_WINDOWS) return;
    const u32 w = t / n, i = t - w * n;
    const xyzz b = load_xyzz(base + t);
    xyzz m = b;
    for (u32 d = 1; d <= SMALL_DIGITS; ++d) {
        store_xyzz(out + ((size_t)(w * SMALL_DIGITS + d - 1)) * n + i, m);
        if (d < SMALL_DIGITS) m = d == 1 ? xyzz_dbl<C>(b) : xyzz_add<C>(m, b);
    }
}

struct SmallSeg {            // one table with its scalars: the key, or the blinding generator h with the blind
    const affine256 *tab;
    const fe256 *scalars;
    u32 n_tab;               // points the table was built for (stride)
    u32 n;                   // scalars used (<= n_tab)
};

// partial[blockIdx.x] (or, for a single workgroup with `direct`, the result) = sum of the workgroup's entries.
// Entry e < 64*(seg0.n + seg1.n): window w = e / ntot, point i = e % ntot (i >= seg0.n: segment 1).
template <int C>
__global__ void __launch_bounds__(256) k_small_msm(SmallSeg s0, SmallSeg s1, int is_mont, xyzz_mem *__restrict__ partial, jacobian256 *__restrict__ direct) {
    latency_critical();
    __shared__ CoopLds L;
    const int lane = threadIdx.x & 63, role = threadIdx.x >> 6;
    const u32 ntot = s0.n + s1.n, total = SMALL_WINDOWS * ntot;
    const u32 e0 = blockIdx.x * SMALL_PER_BLOCK;
    xyzz acc = xyzz_identity();
    bool live = false;
    // SMALL_PER_BLOCK / 64 rounds of entries, then the six levels of the lane tree: one addition site
    for (u32 step = 0; step < SMALL_PER_BLOCK / 64 + 6; ++step) {
        xyzz o = xyzz_identity();
        bool take = false;
        if (step < SMALL_PER_BLOCK / 64) {
            const u32 e = e0 + step * 64u + lane;
            if (e < total) {
                const u32 w = e / ntot, i = e - w * ntot;
                const SmallSeg &sg = i < s0.n ? s0 : s1;
                const u32 j = i < s0.n ? i : i - s0.n;
                fe256 k = load_fe256(sg.scalars + j);
                if (is_mont) k = fe_abi_to_integer<1 - C>(k);
                const u32 d = (k.w[w >> 3] >> ((w & 7u) * 4u)) & 15u;
                if (d) {
                    const affine pt = load_table_point(sg.tab + ((size_t)(w * SMALL_DIGITS + d - 1)) * sg.n_tab + j);
                    take = !affine_is_inf(pt);
                    if (take) o = xyzz_from_affine<C>(pt);
                }
            }
        } else {
            const int dd = 32 >> (step - SMALL_PER_BLOCK / 64);
            const bool o_live = __shfl(live ? 1 : 0, (lane + dd) & 63, WAVE) != 0;
            take = lane < dd && o_live;
            if (__any(take)) o = shfl_xyzz(acc, (lane + dd) & 63);
        }
        if (__any(take)) {
            if (__any(take && live)) {
                const xyzz sum = xyzz_add_coop<C>(acc, o, L, role, lane);
                acc = xyzz_select(take, live ? sum : o, acc);
            } else {
                acc = xyzz_select(take, o, acc);
            }
            live = live || take;
        }
    }
    if (threadIdx.x == 0) {
        if (direct) store_jacobian256(direct, xyzz_to_abi_jacobian<C>(acc));
        else store_xyzz(partial + blockIdx.x, acc);
    }
}

// out = sum of `cnt` partial sums (one workgroup; cnt <= 64 * 8).
template <int C>
__global__ void __launch_bounds__(256) k_small_final(const xyzz_mem *__restrict__ partial_, u32 cnt, jacobian256 *__restrict__ out_) {
    latency_critical();
    __shared__ CoopLds L;
    const int lane = threadIdx.x & 63, role = threadIdx.x >> 6;
    const xyzz_mem *partial = partial_ + (size_t)blockIdx.x * cnt;   // a grid of g workgroups: g independent sums of cnt partial sums each
    jacobian256 *out = out_ + blockIdx.x;
    xyzz acc = xyzz_identity();
    const u32 rounds = (cnt + 63u) / 64u;
    for (u32 step = 0; step < rounds + 6; ++step) {
        xyzz o = xyzz_identity();
        bool take = true;
        if (step < rounds) {
            const u32 e = step * 64u + lane;
            if (e < cnt) o = load_xyzz_coop(partial + e);
        } else {
            const int dd = 32 >> (step - rounds);
            take = lane < dd;
            o = shfl_xyzz(acc, (lane + dd) & 63);
        }
        const xyzz sum = xyzz_add_coop<C>(acc, o, L, role, lane);       // identities fall out of the addition
        acc = xyzz_select(take, sum, acc);
    }
    if (threadIdx.x == 0) store_jacobian256(out, xyzz_to_abi_jacobian<C>(acc));
}

// ---- MSMs over a resident key of a few 10^4 points: byte tables, no sort, no buckets -------------------------------------
// What Reef's prover issues all day is MSMs of 2^14..2^17 points over keys that never change (prove_step, the IPAs:
// src/backend/framework.rs:668-695), and on this chip they are latency chains: the bucket pipeline spends 0.32 ms on 2^15
// points, most of it in ~45 dependent group operations of merge and bucket reduction (DESIGN.md 6).  288 GB of HBM buy a
// shorter chain: for every point every signed byte multiple is tabulated once,
//      W[(w*128 + d - 1)*n + i] = d * 256^w * P_i     (w < 32, d = 1..128; affine, key-table form: 256 KiB per point)
// and an MSM is the plain sum of the <= 32 n entries its signed-byte digits select (negative digits negate y): no doubling,
// no sort, no bucket reduction -- 16 mixed additions per thread, one wave tree, two small reduction launches.
static constexpr u32 WIDE_WINDOWS = 32, WIDE_DIGITS = 128;
static constexpr int WIDE_LEVEL_K = 16;        // additions per thread of the table build (k_wide_level): amortises the workgroup's inversion

// scalars -> 32 signed byte digits each, dig[w*n + i] in [-128, 128] (a raw byte above 128 becomes raw - 256 with a carry;
// canonical scalars are below 2^255, so the top digit absorbs its carry).
template <int C>
__global__ void __launch_bounds__(256) k_wide_recode(const fe256 *__restrict__ scalars, u32 n, int is_mont, short *__restrict__ dig) {
    latency_critical();
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe256 k = load_fe256(scalars + i);
    if (is_mont) k = fe_abi_to_integer<1 - C>(k);
    u32 carry = 0;
#pragma unroll
    for (u32 w = 0; w < WIDE_WINDOWS; ++w) {
        const u32 raw = ((k.w[w >> 2] >> (8u * (w & 3u))) & 0xffu) + carry;
        int d = (int)raw;
        carry = 0;
        if (raw > 128u) { d = (int)raw - 256; carry = 1; }
        dig[(size_t)w * n + i] = (short)d;
    }
}

// partial[workgroup] = sum of the table entries selected by entries e in [workgroup*256*per, ...): e = w*n + i, `per`
// consecutive entries per thread (digits and points of the next entry are fetched while the current addition runs); the 256
// lane sums then go through LDS and are added up by the four waves together (ec_coop.h): 3 + 6 shared additions.
// DUAL: two sums in one pass, for the cross terms of an IPA round (reef_ipa_cross_terms): point i feeds the first sum when it
// lies in the upper half of its block of n_k points (L = <a_lo, G_hi>) and the second otherwise (R = <a_hi, G_lo>);
// partial[workgroup] and partial[gridDim.x + workgroup].
template <int C, bool DUAL>
__global__ void __launch_bounds__(256) k_wide_accum(const affine256 *__restrict__ tab, u32 n_tab, const short *__restrict__ dig, u32 n, u32 per, u32 n_k,
                                                    xyzz_mem *__restrict__ partial) {
    __shared__ CoopLds L;
    __shared__ xyzz_mem stash[256];                                    // 36 KiB + the slots of ec_coop.h: two workgroups per CU
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    const u64 total = (u64)WIDE_WINDOWS * n;
    const u64 e0 = (u64)t * per;
    xyzz acc = xyzz_identity(), acc2 = xyzz_identity();
    affine nxt;
    bool nxt_second = false;
    auto fetch = [&](u64 e, affine &pt, bool &second) -> bool {
        if (e >= total) return false;
        const u32 w = (u32)(e / n), i = (u32)(e - (u64)w * n);
        const int d = dig[e];
        if (d == 0) return false;
        const u32 mag = d < 0 ? (u32)(-d) : (u32)d;
        pt = load_table_point(tab + ((size_t)w * WIDE_DIGITS + mag - 1) * n_tab + i);
        if (d < 0) pt = affine_neg<C>(pt);
        if constexpr (DUAL) second = (i & (n_k - 1u)) < (n_k >> 1);
        return true;
    };
    bool have = fetch(e0, nxt, nxt_second);
    for (u32 k = 0; k < per; ++k) {
        const affine cur = nxt;
        const bool use = have, second = nxt_second;
        if (k + 1 < per) have = fetch(e0 + k + 1, nxt, nxt_second);
        if (use) {
            if constexpr (DUAL) {                                      // one addition site: pick the sum, add, put it back
                const xyzz sum = xyzz_madd<C>(xyzz_select(second, acc2, acc), cur);
                acc = xyzz_select(second, acc, sum);
                acc2 = xyzz_select(second, sum, acc2);
            } else {
                acc = xyzz_madd<C>(acc, cur);
            }
        }
    }
    latency_critical();
    const int lane = threadIdx.x & 63, role = threadIdx.x >> 6;
    for (int which = 0; which < (DUAL ? 2 : 1); ++which) {
        if (which) __syncthreads();                                    // the first sum has been read
        stash[threadIdx.x] = xyzz_to_mem(which ? acc2 : acc);
        __syncthreads();
        const xyzz_mem *src = stash;
        acc = load_xyzz_coop(src + lane);                              // from here on the four waves hold the same 64 sums
        for (int step = 1; step < 4 + 6; ++step) {
            xyzz o;
            bool take = true;
            if (step < 4) {
                o = load_xyzz_coop(src + step * 64 + lane);
            } else {
                const int dd = 32 >> (step - 4);
                take = lane < dd;
                o = shfl_xyzz(acc, (lane + dd) & 63);
            }
            const xyzz sum = xyzz_add_coop<C>(acc, o, L, role, lane);
            acc = xyzz_select(take, sum, acc);
        }
        if (threadIdx.x == 0) store_xyzz(partial + (size_t)which * gridDim.x + blockIdx.x, acc);
    }
}

// out[g] = sum of in[64 g .. 64 g + 64) (cnt entries in all): one four-wave workgroup per 64 partial sums.
template <int C>
__global__ void __launch_bounds__(256) k_wide_reduce(const xyzz_mem *__restrict__ in, u32 cnt, xyzz_mem *__restrict__ out) {
    latency_critical();
    __shared__ CoopLds L;
    const int lane = threadIdx.x & 63, role = threadIdx.x >> 6;
    const u32 e = blockIdx.x * 64u + (u32)lane;
    xyzz acc = xyzz_identity();
    if (e < cnt) acc = load_xyzz_coop(in + e);
    for (int dd = 32; dd >= 1; dd >>= 1) {
        const xyzz o = shfl_xyzz(acc, (lane + dd) & 63);
        const xyzz sum = xyzz_add_coop<C>(acc, o, L, role, lane);
        acc = xyzz_select(lane < dd, sum, acc);
    }
    if (threadIdx.x == 0) store_xyzz(out + blockIdx.x, acc);
}

// out[r] += blinds[r] * H for many rows from H's nibble table: the blinding terms of HyraxPC::commit (commitment.rs:187)
// without 255 doublings per row.  BLIND_LANES lanes share a row: each adds the table entries of its four nibbles, a
// butterfly over the lanes sums them -- a chain of 4 + 4 + 1 dependent additions where one lane per row had 64 (0.28 ms
// behind every commitment of 1024 rows, profiles/r03_rows_timing.txt).
static constexpr u32 BLIND_LANES = 16;
template <int C>
__global__ void __launch_bounds__(64) k_add_blind_tab(jacobian256 *__restrict__ out, const fe256 *__restrict__ blinds, const affine256 *__restrict__ htab,
                                                     int is_mont, u32 nres) {
    latency_critical();
    constexpr u32 PER = SMALL_WINDOWS / BLIND_LANES;           // nibbles per lane: half a 32-bit word
    static_assert(PER == 4, "a lane's nibbles sit in one word of the scalar");
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 r = t / BLIND_LANES, sub = t % BLIND_LANES;
    const bool live = r < nres;
    fe256 k = load_fe256(blinds + (live ? r : 0u));
    if (is_mont) k = fe_abi_to_integer<1 - C>(k);
    u32 word = k.w[0];
#pragma unroll
    for (u32 j = 1; j < 8; ++j) word = (sub >> 1) == j ? k.w[j] : word;
    word = live ? (word >> ((sub & 1u) * 16u)) & 0xFFFFu : 0u;
    xyzz acc = xyzz_identity();
#pragma unroll 1
    for (u32 j = 0; j < PER; ++j) {
        const u32 d = (word >> (4u * j)) & 15u, w = sub * PER + j;
        if (__any(d != 0)) {
            affine pt;
            pt.x = fe_zero(); pt.y = fe_zero();
            if (d) pt = load_table_point(htab + (w * SMALL_DIGITS + d - 1));
            acc = xyzz_madd<C>(acc, pt);                   // the identity (0, 0) adds nothing
        }
    }
#pragma unroll 1
    for (u32 off = BLIND_LANES / 2; off >= 1; off >>= 1)
        acc = xyzz_add<C>(acc, shfl_xyzz(acc, (int)((threadIdx.x & 63u) ^ off)));
    if (live && sub == 0)
        store_jacobian256(out + r, xyzz_to_abi_jacobian<C>(xyzz_add<C>(xyzz_from_abi_jacobian<C>(load_jacobian256(out + r)), acc)));
}

// The nibble table of a DEVICE-resident blinding generator, kept current without a host round trip: one wave compares h
// (ABI form, 64 B) with the copy the table was built for and returns when they agree (the usual case: h is fixed for the
// life of a commitment key, commitment.rs:146-149); otherwise it rebuilds the 960 entries in place -- lane 0 the chain of
// 16^w * h, every lane the 15 multiples of its window, normalised five at a time per inversion -- and records the new h.
// `scratch` holds 64 + 960 XYZZ points.  ~1 ms when h changed, a few microseconds of stream time when it did not.
template <int C>
__global__ void __launch_bounds__(64) k_h_refresh(const affine256 *__restrict__ h_abi, affine256 *__restrict__ cached, u32 *__restrict__ valid,
                                                  xyzz_mem *__restrict__ scratch, affine256 *__restrict__ tab) {
    const u32 lane = threadIdx.x;
    const u32 *a = reinterpret_cast<const u32 *>(h_abi);
    u32 *b = reinterpret_cast<u32 *>(cached);
    const u32 mine = lane < 16 ? a[lane] : 0u;
    const bool differs = lane < 16 && mine != b[lane];
    if (!__any(differs) && *valid != 0) return;
    xyzz_mem *base = scratch, *mult = scratch + SMALL_WINDOWS;
    if (lane == 0) {
        xyzz p = xyzz_from_affine<C>(affine_from_abi<C>(load_affine256(h_abi)));
        for (u32 w = 0; w < SMALL_WINDOWS; ++w) {
            if (w)
                for (u32 s = 0; s < 4; ++s) p = xyzz_dbl<C>(p);
            store_xyzz(base + w, p);
        }
    }
    __syncthreads();
    {
        const xyzz bw = load_xyzz(base + lane);
        xyzz m = bw;
        for (u32 d = 1; d <= SMALL_DIGITS; ++d) {
            store_xyzz(mult + lane * SMALL_DIGITS + d - 1, m);
            if (d < SMALL_DIGITS) m = d == 1 ? xyzz_dbl<C>(bw) : xyzz_add<C>(m, bw);
        }
    }
    constexpr int PER = 5;
    static_assert(SMALL_DIGITS % PER == 0, "the digits of a window are normalised PER at a time");
    for (u32 g = 0; g < SMALL_DIGITS / PER; ++g) {
        const xyzz_mem *in = mult + lane * SMALL_DIGITS + g * PER;
        fe zp[PER], pre[PER];
        fe acc = fe_one<C>();
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const xyzz p = load_xyzz(in + k);
            const fe prod = fe_mul<C>(p.zz, p.zzz);
            zp[k] = fe_select(fe_is_zero<C>(prod), fe_one<C>(), prod);
            pre[k] = acc;
            acc = fe_mul<C>(acc, zp[k]);
        }
        fe inv = fe_inv<C>(acc);
#pragma unroll
        for (int k = PER - 1; k >= 0; --k) {
            const fe ti = fe_mul<C>(inv, pre[k]);
            inv = fe_mul<C>(inv, zp[k]);
            const affine q = xyzz_to_affine_with_inv<C>(load_xyzz(in + k), ti);
            store_affine256(tab + lane * SMALL_DIGITS + g * PER + k, affine_to_table<C>(q));
        }
    }
    __syncthreads();
    if (lane < 16) b[lane] = mine;
    if (lane == 0) *valid = 1u;
}

// Horner over the G group sums of each result: acc = 2^c * acc + S_g.  One thread per
// result (rows of a batched MSM run in parallel).  Writes ABI Jacobian (x, y, z), 96 B.
template <int C>
__global__ void __launch_bounds__(64) k_final(const xyzz_mem *__restrict__ group_sums, u32 G, u32 c, u32 nres,
                                             jacobian256 *__restrict__ out) {
    latency_critical();
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nres) return;
    xyzz acc = load_xyzz(group_sums + (size_t)r * G + (G - 1));
    for (int g = (int)G - 2; g >= 0; --g) {
        for (u32 k = 0; k < c; ++k) acc = xyzz_dbl<C>(acc);
        acc = xyzz_add<C>(acc, load_xyzz(group_sums + (size_t)r * G + g));
    }
    store_jacobian256(out + r, xyzz_to_abi_jacobian<C>(acc));
}

// ------------------------------------------------- batch normalisation (K4) ----
// ABI Jacobian -> ABI affine (and optionally the 32-byte compressed form).  Each thread owns
// NORM_PER consecutive points and shares one field inversion among them (Montgomery's trick).
static constexpr int NORM_PER = 8;

// ---- one field inversion per workgroup ---------------------------------------------------------
// Every lane hands in a non-zero `a` and gets 1/a back.  Products are scanned inside each wave with
// shuffles (prefix and suffix), the wave totals meet in LDS, wave 0 inverts their product -- the
// other waves wait at the barrier and leave the SIMDs to other workgroups -- and every lane rebuilds
// its own inverse from the pieces: 14 products per lane plus one inversion per workgroup instead of
// one inversion (~290 products) per lane.  blockDim.x: a multiple of 64, at most 1024.
__device__ __forceinline__ fe shfl_fe(const fe &a, int src_lane) {
    fe r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = __shfl(a.l[i], src_lane, WAVE);
    REEF_SET_BOUND(r, REEF_GET_BOUND(a));
    return r;
}
struct BatchInvShared {
    u32 tot[16][9];
    u32 inv[16][9];
};
template <int C>
__device__ __forceinline__ fe block_batch_inverse(const fe &a, BatchInvShared &sh) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    fe x = a, s = a;                                   // inclusive prefix / suffix products within the wave
    for (int d = 1; d < 64; d <<= 1) {
        const fe up = shfl_fe(x, (lane - d) & 63), dn = shfl_fe(s, (lane + d) & 63);
        const fe xu = fe_mul<C>(x, up), sd = fe_mul<C>(s, dn);
        x = fe_select(lane >= d, xu, x);
        s = fe_select(lane + d < 64, sd, s);
    }
    const fe one = fe_one<C>();
    fe e = shfl_fe(x, (lane - 1) & 63), t = shfl_fe(s, (lane + 1) & 63);   // exclusive
    e = fe_select(lane == 0, one, e);
    t = fe_select(lane == 63, one, t);
    if (lane == 63) {
#pragma unroll
        for (int i = 0; i < 9; ++i) sh.tot[wid][i] = x.l[i];
    }
    __syncthreads();
    if (wid == 0) {                                    // lanes 0..nw-1 hold the wave totals; the same scans again
        fe w = one;
        if (lane < nw) {
#pragma unroll
            for (int i = 0; i < 9; ++i) w.l[i] = sh.tot[lane][i];
        }
        fe px = w, sx = w;
        for (int d = 1; d < 16; d <<= 1) {
            const fe up = shfl_fe(px, (lane - d) & 63), dn = shfl_fe(sx, (lane + d) & 63);
            const fe xu = fe_mul<C>(px, up), sd = fe_mul<C>(sx, dn);
            px = fe_select(lane >= d, xu, px);
            sx = fe_select(lane + d < 64, sd, sx);     // lanes >= nw hold one: they do not disturb the products
        }
        const fe total = shfl_fe(px, 15);              // product of all wave totals (lanes nw..15 contribute one)
        const fe inv_total = fe_inv<C>(total);
        fe pe = shfl_fe(px, (lane - 1) & 63), se = shfl_fe(sx, (lane + 1) & 63);
        pe = fe_select(lane == 0, one, pe);
        const fe winv = fe_mul<C>(inv_total, fe_mul<C>(pe, se));   // inverse of this lane's wave total
        if (lane < nw) {
#pragma unroll
            for (int i = 0; i < 9; ++i) sh.inv[lane][i] = winv.l[i];
        }
    }
    __syncthreads();
    fe winv;
#pragma unroll
    for (int i = 0; i < 9; ++i) winv.l[i] = sh.inv[wid][i];
    REEF_SET_BOUND(winv, 2.0);
    return fe_mul<C>(winv, fe_mul<C>(e, t));
}


template <int C>
__global__ void __launch_bounds__(256) k_normalize(const jacobian256 *__restrict__ in, u32 n, affine256 *__restrict__ out_aff,
                                                  fe256 *__restrict__ out_comp) {
    __shared__ BatchInvShared inv_sh;
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    const u64 i0 = (u64)t * NORM_PER;                  // threads past the end take part in the shared inversion with a one
    fe z[NORM_PER], pre[NORM_PER];
    fe acc = fe_one<C>();
#pragma unroll
    for (int k = 0; k < NORM_PER; ++k) {
        z[k] = fe_one<C>();
        if (i0 + k < n) {
            const fe zk = fe_from_abi<C>(load_fe256(&in[i0 + k].z));
            z[k] = fe_select(fe_is_zero<C>(zk), z[k], zk);  // identity handled below
        }
        pre[k] = acc;
        acc = fe_mul<C>(acc, z[k]);
    }
    fe inv = block_batch_inverse<C>(acc, inv_sh);
#pragma unroll
    for (int k = NORM_PER - 1; k >= 0; --k) {
        const fe zi = fe_mul<C>(inv, pre[k]);
        inv = fe_mul<C>(inv, z[k]);
        if (i0 + k < n) {
            const jacobian256 j = load_jacobian256(in + i0 + k);
            const fe zz = fe_from_abi<C>(j.z);
            const bool inf = fe_is_zero<C>(zz);
            const fe zi2 = fe_sqr<C>(zi);
            affine a;
            a.x = fe_select(inf, fe_zero(), fe_mul<C>(fe_from_abi<C>(j.x), zi2));
            a.y = fe_select(inf, fe_zero(), fe_mul<C>(fe_from_abi<C>(j.y), fe_mul<C>(zi2, zi)));
            if (out_aff) store_affine256(out_aff + i0 + k, affine_to_abi<C>(a));
            if (out_comp) store_fe256(out_comp + i0 + k, affine_compress<C>(a));
        }
    }
}

// One doubling level of the byte tables (k_wide_accum): W[m + j] = W[m] + W[j] for j = 1..m, every window, every point,
// in place and in affine form: 32*m*n independent additions share inversions by Montgomery's trick (8 per thread, one
// inversion per workgroup).  Seven levels (m = 1 .. 64) turn the 32 window bases of every point into its 4096 table entries;
// the additions of a level cannot collide (multiples below 256 of a point of prime order), so the only special case is a
// denominator of zero: the point at infinity as a key point ((0, 0) stays (0, 0)).  j = m is the doubling.
template <int C>
__global__ void __launch_bounds__(256) k_wide_level(affine256 *__restrict__ tab, u32 n, u32 m, const int *__restrict__ abort_flag) {
    if (abort_flag && *(const volatile int *)abort_flag) return;      // the key is being dropped or re-keyed: the levels still queued do nothing
    __shared__ BatchInvShared inv_sh;
    constexpr int K = WIDE_LEVEL_K;
    const u64 total = (u64)WIDE_WINDOWS * m * n;
    const u64 T = (u64)gridDim.x * blockDim.x;
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    auto locate = [&](u64 a, size_t &ip, size_t &iq, size_t &io, bool &dbl) {
        const u32 i = (u32)(a % n);
        const u64 r = a / n;
        const u32 j = (u32)(r % m) + 1u, w = (u32)(r / m);
        const size_t row = (size_t)w * WIDE_DIGITS;
        ip = (row + m - 1) * n + i;
        iq = (row + j - 1) * n + i;
        io = (row + m + j - 1) * n + i;
        dbl = j == m;
    };
    fe den[K], pre[K];
    fe acc = fe_one<C>();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        den[k] = fe_one<C>();
        const u64 a = t + (u64)k * T;
        if (a < total) {
            size_t ip, iq, io;
            bool dbl;
            locate(a, ip, iq, io, dbl);
            const affine P = load_table_point(tab + ip), Q = load_table_point(tab + iq);
            const fe d = dbl ? fe_dbl<C>(P.y) : fe_sub<C, 2>(Q.x, P.x);                          // < 4
            den[k] = fe_select(fe_is_zero<C>(d), den[k], d);
        }
        pre[k] = acc;
        acc = fe_mul<C>(acc, den[k]);
    }
    fe inv = block_batch_inverse<C>(acc, inv_sh);
#pragma unroll
    for (int k = K - 1; k >= 0; --k) {
        const fe di = fe_mul<C>(inv, pre[k]);
        inv = fe_mul<C>(inv, den[k]);
        const u64 a = t + (u64)k * T;
        if (a < total) {
            size_t ip, iq, io;
            bool dbl;
            locate(a, ip, iq, io, dbl);
            const affine P = load_table_point(tab + ip), Q = load_table_point(tab + iq);
            const fe d = dbl ? fe_dbl<C>(P.y) : fe_sub<C, 2>(Q.x, P.x);
            const bool inf = fe_is_zero<C>(d);                          // infinity in, infinity out
            fe num;
            if (dbl) { const fe xx = fe_sqr<C>(P.x); num = fe_add<C>(fe_dbl<C>(xx), xx); }     // 3 x^2 < 6
            else num = fe_sub<C, 2>(Q.y, P.y);                                                  // < 3
            const fe lam = fe_mul<C>(num, di);                                                  // < 2
            const fe x3 = fe_sub<C, 2>(fe_sub<C, 2>(fe_sqr<C>(lam), P.x), Q.x);                 // < 6
            const fe y3 = fe_sub<C, 2>(fe_mul<C>(lam, fe_sub<C, 8>(P.x, x3)), P.y);             // < 4
            affine r;
            r.x = fe_select(inf, fe_zero(), x3);
            r.y = fe_select(inf, fe_zero(), y3);
            store_affine256(tab + io, affine_to_table<C>(r));
        }
    }
}

// ------------------------------------------------ resident-key precompute ----
// XYZZ -> affine for `n` points; NORM_PER points per thread share one inversion.  Output in
// key-table form (internal Montgomery, canonical) or ABI form.
template <int C, bool ABI_OUT>
__global__ void __launch_bounds__(256) k_xyzz_normalize(const xyzz_mem *__restrict__ in, u32 n, affine256 *__restrict__ out) {
    __shared__ BatchInvShared inv_sh;
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    const u64 i0 = (u64)t * NORM_PER;                  // threads past the end take part in the shared inversion with a one
    fe zp[NORM_PER], pre[NORM_PER];
    fe acc = fe_one<C>();
#pragma unroll
    for (int k = 0; k < NORM_PER; ++k) {
        zp[k] = fe_one<C>();
        if (i0 + k < n) {
            const xyzz p = load_xyzz(in + i0 + k);
            const fe prod = fe_mul<C>(p.zz, p.zzz);
            zp[k] = fe_select(fe_is_zero<C>(prod), zp[k], prod);
        }
        pre[k] = acc;
        acc = fe_mul<C>(acc, zp[k]);
    }
    fe inv = block_batch_inverse<C>(acc, inv_sh);
#pragma unroll
    for (int k = NORM_PER - 1; k >= 0; --k) {
        const fe ti = fe_mul<C>(inv, pre[k]);
        inv = fe_mul<C>(inv, zp[k]);
        if (i0 + k < n) {
            const affine a = xyzz_to_affine_with_inv<C>(load_xyzz(in + i0 + k), ti);
            store_affine256(out + i0 + k, ABI_OUT ? affine_to_abi<C>(a) : affine_to_table<C>(a));
        }
    }
}

// ABI points -> key-table form (one Montgomery product per coordinate, once per key).
template <int C>
__global__ void __launch_bounds__(256) k_import_key(const affine256 *__restrict__ src, u32 n, affine256 *__restrict__ dst) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    store_affine256(dst + i, affine_to_table<C>(affine_from_abi<C>(load_affine256(src + i))));
}

// dst[i] = the loop form of the packed table entry src[i] (ec.h: affine_limbs), for all the tables of a pre-shifted key at
// once: what k_accum0 would otherwise work out again for every entry of every MSM on the key.  Runs once per key.
template <int C>
__global__ void __launch_bounds__(256) k_limb_tables(const affine256 *__restrict__ src, u32 count, affine_limbs *__restrict__ dst) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const affine_limbs r = affine_limbs_from_table<C>(load_affine256(src + i));
    u32x4 *q = reinterpret_cast<u32x4 *>(dst + i);
#pragma unroll
    for (int k = 0; k < 8; ++k) q[k] = mk_u32x4(r.w[4 * k], r.w[4 * k + 1], r.w[4 * k + 2], r.w[4 * k + 3]);
}

// tmp[j*n + i] = 2^(shift*(j + 1 - first)) * src[i] for j < count (XYZZ; with `first` tmp[i] is src[i] itself): the
// pre-shifted tables of a key in ONE dependent chain per point, followed by ONE k_xyzz_normalize over all of them -- a
// table at a time (shift, normalise, shift, ...) was 2 x (T - 1) launches that each waited for a Fermat inversion.
// Runs once per key (commitment keys are fixed for the life of a PublicParams, src/backend/framework.rs:45,134).
template <int C>
__global__ void __launch_bounds__(64) k_shift_chain(const affine256 *__restrict__ src, u32 n, u32 shift, u32 count, int first,
                                                    xyzz_mem *__restrict__ tmp) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    xyzz p = xyzz_from_affine<C>(load_table_point(src + i));
    for (u32 j = 0; j < count; ++j) {
        if (!(first && j == 0))
            for (u32 s = 0; s < shift; ++s) p = xyzz_dbl<C>(p);
        store_xyzz(tmp + (size_t)j * n + i, p);
    }
}

// ---- K2 for tiny scalars: block tables instead of buckets -----------------------------------
// HyraxPC::commit (src/backend/commitment.rs:187) commits every row of the document matrix to the
// same row generators, and the entries are document symbols (< |alphabet| + 3, framework.rs:978-1011).
// With `bits`-bit symbols the generators are taken k at a time (2^(bits*k) <= 512) and every sum
//   T[block][combo] = sum_{t<k} sym_t * G_{block*k + t},   combo = sym_0 | sym_1 << bits | ...
// is tabulated once per key (affine, key-table form).  A row is then the plain sum of row_len/k table
// entries: no digits, no sort, no bucket reduction -- the entries (key = row, payload = table index)
// are written in row order and go straight into k_accum0 / k_accumN with the rows as "buckets".

// Phase 1: small multiples of every generator.  part 0: lo*G for lo < 2^lb; part 1: hi*(2^lb G) for
// hi < 2^hb.  One thread per (generator, part), running sums (XYZZ).
template <int C>
__global__ void __launch_bounds__(256) k_sym_multiples(const affine256 *__restrict__ gens, u32 n, u32 lb, u32 hb, xyzz_mem *__restrict__ lo_out,
                                                      xyzz_mem *__restrict__ hi_out) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 j = t >> 1, part = t & 1u;
    if (j >= n || (part == 1 && hb == 0)) return;
    const affine g = load_table_point(gens + j);
    const u32 count = 1u << (part ? hb : lb);
    xyzz_mem *out = (part ? hi_out : lo_out) + (size_t)j * count;
    xyzz step = xyzz_from_affine<C>(g);
    if (part)
        for (u32 s = 0; s < lb; ++s) step = xyzz_dbl<C>(step);
    xyzz acc = xyzz_identity();
    store_xyzz(out, acc);
    for (u32 v = 1; v < count; ++v) {
        acc = part ? xyzz_add<C>(acc, step) : xyzz_madd<C>(acc, g);
        store_xyzz(out + v, acc);
    }
}

// Phase 2: table[block][combo] (XYZZ) from the multiples; generators past row_len count as identity.
template <int C>
__global__ void __launch_bounds__(256) k_sym_blocks(const xyzz_mem *__restrict__ lo_in, const xyzz_mem *__restrict__ hi_in, u32 n, u32 bits, u32 lb,
                                                   u32 k, u32 blocks, xyzz_mem *__restrict__ table) {
    const u32 combos = 1u << (bits * k);
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (u64)blocks * combos) return;
    const u32 block = (u32)(t / combos), combo = (u32)(t % combos);
    const u32 hb = bits - lb;
    xyzz acc = xyzz_identity();
    bool have = false;                                 // the first term is copied, not added to the identity
    for (u32 q = 0; q < k; ++q) {
        const u32 j = block * k + q;
        const u32 sym = (combo >> (bits * q)) & ((1u << bits) - 1u);
        if (j >= n || sym == 0) continue;
        const u32 lo = sym & ((1u << lb) - 1u), hi = sym >> lb;
        if (lo) {
            const xyzz x = load_xyzz(lo_in + ((size_t)j << lb) + lo);
            acc = have ? xyzz_add<C>(acc, x) : x;
            have = true;
        }
        if (hi) {
            const xyzz x = load_xyzz(hi_in + ((size_t)j << hb) + hi);
            acc = have ? xyzz_add<C>(acc, x) : x;
            have = true;
        }
    }
    store_xyzz(table + t, acc);
}

// Field-element scalars (known to be < 2^bits) -> one byte each.
template <int C>
__global__ void __launch_bounds__(256) k_row_symbols(const fe256 *__restrict__ scalars, u64 n, int is_mont, unsigned char *__restrict__ sym) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    fe256 v = load_fe256(scalars + i);
    if (is_mont) v = fe_abi_to_integer<1 - C>(v);
    sym[i] = (unsigned char)v.w[0];
}

// entries[row*blocks + block] = (row, block*combos + combo); bucket_start[row] = row*blocks.
static __global__ void __launch_bounds__(256) k_sym_entries(const unsigned char *__restrict__ sym, u32 rows, u32 row_len, u32 bits, u32 k, u32 blocks,
                                                    u32x2 *__restrict__ entries, u32 *__restrict__ bucket_start) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= rows) bucket_start[t] = (u32)t * blocks;
    if (t >= (u64)rows * blocks) return;
    const u32 row = (u32)(t / blocks), block = (u32)(t % blocks);
    const unsigned char *p = sym + (size_t)row * row_len;
    const u32 mask = (1u << bits) - 1u;
    u32 combo = 0;
    for (u32 q = 0; q < k; ++q) {
        const u32 j = block * k + q;
        if (j < row_len) combo |= ((u32)p[j] & mask) << (bits * q);
    }
    entries[t] = mk_u32x2(row, (block << (bits * k)) + combo);
}

// Symbols wider than a byte (T = uint16_t, uint32_t; P = ceil(bits / 8) byte planes).  A symbol is sum_p byte_p * 256^p, so its
// term is the sum of P entries of byte-multiple tables over the plane generators 256^p * G_j.  The table holds the full planes
// first, 256 multiples per generator, and then the top plane with 2^top_bits (top_bits = bits - 8(P - 1)):
//   index(p, j, v) = (p*row_len + j)*256 + v               for p < P - 1
//   index(P-1, j, v) = (P - 1)*row_len*256 + (j << top_bits) + v
// One symbol per thread; its P entries are consecutive (generator-major), so a thread's store is one 8P-byte run and a wave's
// stores are contiguous.  entries[(row*row_len + j)*P + p] = (row, index(p, j, byte_p)); bucket_start[row] = row*P*row_len.
template <typename T>
static __global__ void __launch_bounds__(256) k_sym_entries_wide(const T *__restrict__ sym, u32 rows, u32 row_len, u32 bits, u32 P,
                                                                 u32x2 *__restrict__ entries, u32 *__restrict__ bucket_start) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t <= rows) bucket_start[t] = (u32)t * P * row_len;
    if (t >= (u64)rows * row_len) return;
    const u32 row = (u32)(t / row_len), j = (u32)(t % row_len);
    const u32 s = (u32)sym[t] & (bits >= 32 ? ~0u : (1u << bits) - 1u);
    const u32 top_bits = bits - 8 * (P - 1);
    u32x2 *e = entries + t * P;
    for (u32 p = 0; p + 1 < P; ++p) e[p] = mk_u32x2(row, ((p * row_len + j) << 8) + ((s >> (8 * p)) & 0xffu));
    e[P - 1] = mk_u32x2(row, (((P - 1) * row_len) << 8) + (j << top_bits) + (s >> (8 * (P - 1))));
}

// Deterministic test key: B_i = (k0 + i*d)*G, G = (-1, 2) (the discrete logs are known, so
// any MSM over these bases can be checked in O(n) field operations).  Thread t produces
// `per` consecutive points (XYZZ, normalised afterwards by k_xyzz_normalize).
template <int C>
__global__ void __launch_bounds__(256) k_gen_bases_ap(u64 k0, u64 d, u32 n, u32 per, xyzz_mem *__restrict__ tmp) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    const u64 i0 = (u64)t * per;
    if (i0 >= n) return;
    affine g;
    g.x = fe_canon<C>(fe_neg<C, 2>(fe_one<C>()));   // -1
    g.y = fe_canon<C>(fe_dbl<C>(fe_one<C>()));      //  2
    const unsigned __int128 ks = (unsigned __int128)k0 + (unsigned __int128)i0 * d;
    u32 kw[8] = {(u32)ks, (u32)(ks >> 32), (u32)(ks >> 64), (u32)(ks >> 96), 0, 0, 0, 0};
    u32 dw[8] = {(u32)d, (u32)(d >> 32), 0, 0, 0, 0, 0, 0};
    xyzz cur = xyzz_scalar_mul<C>(g, kw, 127);
    const xyzz step = xyzz_scalar_mul<C>(g, dw, 63);
    for (u32 k = 0; k < per && i0 + k < n; ++k) {
        store_xyzz(tmp + i0 + k, cur);
        cur = xyzz_add<C>(cur, step);
    }
}

// Seeded scalars, identical stream to oracle/pasta_ref.c::pasta_ref_gen_scalars
// (SplitMix64, 4 draws per scalar; kind 0 uniform, 1 witness-like, 2 small).
__device__ __forceinline__ u64 splitmix_at(u64 seed, u64 idx) {
    u64 z = seed + (idx + 1) * 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
template <int C>
__global__ void __launch_bounds__(256) k_gen_scalars(u64 seed, int kind, u64 small_bound, u32 n, int to_mont,
                                                    fe256 *__restrict__ out) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 w[4];
    for (int j = 0; j < 4; ++j) w[j] = splitmix_at(seed, 4ull * i + j);
    fe256 v;
#pragma unroll
    for (int j = 0; j < 8; ++j) v.w[j] = 0;
    if (kind == 2) {
        u64 x = small_bound ? w[0] % small_bound : 0;
        v.w[0] = (u32)x; v.w[1] = (u32)(x >> 32);
    } else {
        int cls = 2;
        if (kind == 1) {
            u32 sel = (u32)(w[3] >> 56) % 10u;
            cls = sel < 7 ? 0 : (sel < 9 ? 1 : 2);
        }
        if (cls == 0) v.w[0] = (u32)(w[0] & 1);
        else if (cls == 1) v.w[0] = (u32)(w[0] & 0xffff);
        else {
            for (int j = 0; j < 4; ++j) { v.w[2 * j] = (u32)w[j]; v.w[2 * j + 1] = (u32)(w[j] >> 32); }
            v.w[7] &= 0x7fffffffu;
            fe x = fe_unpack(v);  // < 2^255 < 2M
            REEF_SET_BOUND(x, 2.0);
            v = fe_pack(fe_canon<1 - C>(x));
        }
    }
    if (to_mont) v = fe_to_abi<1 - C>(fe_from_integer<1 - C>(v));
    store_fe256(out + i, v);
}

// ----------------------------------------------------------- fold (K3) --------
// out_i = w1*L_i + w2*R_i for i < half (L = gens[0..half), R = gens[half..2*half)), the
// generator fold of the IPA rounds (nova-snark ipa_pc via CompressedSNARK::prove,
// src/backend/framework.rs:695).  All lanes share (w1, w2), so the joint double-and-add
// (Shamir) runs without divergence; k_xyzz_normalize then writes the affine generators.
template <int C>
__global__ void __launch_bounds__(256) k_fold(const affine256 *__restrict__ gens, u32 half, fe256 w1, fe256 w2,
                                             xyzz_mem *__restrict__ tmp) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= half) return;
    int top = -1;
    for (int l = 7; l >= 0; --l) {
        u32 x = w1.w[l] | w2.w[l];
        if (x) { top = 32 * l + (31 - (int)__clz(x)); break; }
    }
    const affine L = affine_from_abi<C>(load_affine256(gens + i));
    const affine R = affine_from_abi<C>(load_affine256(gens + half + i));
    xyzz a = xyzz_identity();
    for (int b = top; b >= 0; --b) {
        a = xyzz_dbl<C>(a);
        if ((w1.w[b >> 5] >> (b & 31)) & 1u) a = xyzz_madd<C>(a, L);
        if ((w2.w[b >> 5] >> (b & 31)) & 1u) a = xyzz_madd<C>(a, R);
    }
    store_xyzz(tmp + i, a);
}

// The same fold with the curve endomorphism (phi(x, y) = (beta*x, y) = lambda*(x, y)): w1 = a1 + a2*lambda and
// w2 = b1 + b2*lambda with 128-bit parts (glv_host.h), so
//   w1*L + w2*R = a1*L + a2*phi(L) + b1*R + b2*phi(R)
// is a joint double-and-add over 128 bits instead of 255.  Every lane first tabulates the 15 non-empty sums
// of its four points (signs of the parts folded into the points), then each bit costs one doubling and at
// most one addition from the table; the four scalars are wave-uniform, so there is no divergence.
struct GlvScalars {
    u32 k[4][5];     // |a1|, |a2|, |b1|, |b2|
    u32 neg[4];
    u32 top;         // highest set bit over the four magnitudes (-1: all zero)
};
template <int C>
__global__ void __launch_bounds__(256) k_fold_glv(const affine256 *__restrict__ gens, u32 half, GlvScalars sc, xyzz_mem *__restrict__ table,
                                                 xyzz_mem *__restrict__ tmp) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= half) return;
    const fe beta = fe_const<C>(GLV<C>::BETA, 1.0);
    affine pt[4];
    pt[0] = affine_from_abi<C>(load_affine256(gens + i));
    pt[2] = affine_from_abi<C>(load_affine256(gens + half + i));
    pt[1] = pt[0];
    pt[3] = pt[2];
    pt[1].x = fe_canon<C>(fe_mul<C>(pt[0].x, beta));   // phi keeps (0, 0), the affine identity
    pt[3].x = fe_canon<C>(fe_mul<C>(pt[2].x, beta));
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (sc.neg[j]) pt[j].y = fe_select(affine_is_inf(pt[j]), pt[j].y, fe_canon<C>(fe_neg<C, 2>(pt[j].y)));
    // table[m][i] = sum of pt[j] over the set bits j of m, m = 1..15 (entry 0 unused)
    for (u32 m = 1; m < 16; ++m) {
        const u32 low = m & (m - 1u);                  // m without its lowest set bit
        const int j = __ffs((int)m) - 1;
        xyzz v;
        if (low == 0) v = xyzz_from_affine<C>(pt[j]);
        else v = xyzz_madd<C>(load_xyzz(table + (size_t)low * half + i), pt[j]);
        store_xyzz(table + (size_t)m * half + i, v);
    }
    xyzz a = xyzz_identity();
    for (int b = (int)sc.top; b >= 0; --b) {
        a = xyzz_dbl<C>(a);
        u32 m = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) m |= ((sc.k[j][b >> 5] >> (b & 31)) & 1u) << j;
        if (m) a = xyzz_add<C>(a, load_xyzz(table + (size_t)m * half + i));
    }
    store_xyzz(tmp + i, a);
}

// The same fold with every group operation spread over the four waves of a workgroup (ec_coop.h): 64 outputs per workgroup.
// A fold of at most 2^16 outputs is ONE wave per SIMD at best, i.e. a chain of ~128 dependent doublings and ~120 additions at
// one-wave latency (3.7 / 7.2 us: 1.3 ms whatever the size); shared over four waves the operations take 3.0 / 3.7 us.  One
// addition site and one doubling site (an inlined operation is ~35 KB of code): the eleven composite table entries and the
// bits of the chain go through the same loop.  Wave 0 does the stores; the table is read back by all four (workgroup-scope
// coherence: a barrier after each store).
template <int C>
__global__ void __launch_bounds__(256) k_fold_glv_coop(const affine256 *__restrict__ gens, u32 half, GlvScalars sc, xyzz_mem *table,
                                                      xyzz_mem *__restrict__ tmp) {
    latency_critical();
    __shared__ CoopLds L;
    const int lane = threadIdx.x & 63, role = threadIdx.x >> 6;
    const u32 i0 = blockIdx.x * 64u + lane;
    const bool live = i0 < half;
    const u32 i = live ? i0 : half - 1u;                      // idle lanes repeat the last output and store nothing
    {
        const fe beta = fe_const<C>(GLV<C>::BETA, 1.0);
        affine pt[4];
        pt[0] = affine_from_abi<C>(load_affine256(gens + i));
        pt[2] = affine_from_abi<C>(load_affine256(gens + half + i));
        pt[1] = pt[0];
        pt[3] = pt[2];
        pt[1].x = fe_canon<C>(fe_mul<C>(pt[0].x, beta));
        pt[3].x = fe_canon<C>(fe_mul<C>(pt[2].x, beta));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (sc.neg[j]) pt[j].y = fe_select(affine_is_inf(pt[j]), pt[j].y, fe_canon<C>(fe_neg<C, 2>(pt[j].y)));
            if (role == 0 && live) store_xyzz(table + (size_t)(1u << j) * half + i, xyzz_from_affine<C>(pt[j]));
        }
    }
    __syncthreads();
    xyzz a = xyzz_identity(), ahead = xyzz_identity();      // ahead: the table entry of the NEXT bit, requested a step early
    auto entry_of = [&](int b) {
        u32 sel = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) sel |= ((sc.k[j][b >> 5] >> (b & 31)) & 1u) << j;
        return sel;
    };
    const int steps = 11 + (int)sc.top + 1;
    u32 m = 2;
    for (int step = 0; step < steps; ++step) {
        xyzz x, y;
        bool add;
        if (step < 11) {                                      // table[m] = table[m without its lowest bit] + table[lowest bit], m = 3, 5, 6, 7, 9, ..
            do { ++m; } while ((m & (m - 1u)) == 0);
            const u32 low = m & (m - 1u);
            x = load_xyzz_coop(table + (size_t)low * half + i);
            y = load_xyzz_coop(table + (size_t)(m ^ low) * half + i);
            add = true;
        } else {
            const int b = (int)sc.top - (step - 11);
            add = entry_of(b) != 0;
            y = ahead;
            if (b > 0) {
                const u32 nxt = entry_of(b - 1);
                if (nxt) ahead = load_xyzz_coop(table + (size_t)nxt * half + i);
            }
            a = xyzz_dbl_coop<C>(a, L, role, lane);
            x = a;
        }
        if (add) {                                            // uniform over the workgroup
            const xyzz sum = xyzz_add_coop<C>(x, y, L, role, lane);
            if (step < 11) {
                if (role == 0 && live) store_xyzz(table + (size_t)m * half + i, sum);
                __syncthreads();
            } else a = sum;
        }
        if (step == 10) {                                     // the table is complete: the entry of the top bit
            const u32 nxt = entry_of((int)sc.top);
            if (nxt) ahead = load_xyzz_coop(table + (size_t)nxt * half + i);
        }
    }
    if (role == 0 && live) store_xyzz(tmp + i, a);
}

// ---- deep fold (K3, deep): the generators k folds away in one bucket pass -----------------------------------------
// After k folds G^(k)_j = sum_{t < T} s_t * G_{t*n_k + j} (T = 2^k, n_k = n/T, s_t the products k_ipa_coef forms): n_k outputs that all
// use the SAME T scalars.  The host forms the s_t, splits them with the endomorphism (s_t = a_t + b_t*lambda, 128-bit parts) and recodes
// the parts into signed 3-bit digits in [-4, 4]; dig[(h*DEEP_WMAX + w)*T + t] is digit w of half h (0: a_t, 1: b_t) with the sign
// of the part folded in.  One lane per (output j, window w): a wave holds 64 consecutive j of ONE window, so the digit of every term is
// wave-uniform (a scalar load, a scalar branch), and the four signed buckets of the window live in registers.  phi(P) = (beta*x, y) is
// applied on load for the second half.  One mixed-addition site: the bucket is moved out, added to and moved back.
// k_deep_accum leaves part[(s*W + w)*cnt + j]: the sum of window w over the t of chunk s; k_deep_reduce sums the chunks (only when
// there is more than one: few outputs of many terms); k_deep_horner_coop combines the windows per output, 3 doublings and one
// addition per window, every group operation shared over the four waves of a workgroup (ec_coop.h) as in k_fold_glv_coop.
static constexpr u32 DEEP_C = 3, DEEP_WMAX = 88;       // 88 windows of 3 bits: a 256-bit magnitude and its carry
template <int C>
__global__ void __launch_bounds__(64) k_deep_accum(const affine256 *__restrict__ tab0, u32 n_k, u32 j0, u32 cnt, u32 T, u32 t_per, u32 H,
                                                  const signed char *__restrict__ dig, xyzz_mem *__restrict__ part) {
    const u32 jl = blockIdx.x * 64u + threadIdx.x;
    const u32 w = blockIdx.y, s = blockIdx.z, W = gridDim.y;
    if (jl >= cnt) return;
    const u32 t0 = s * t_per, t1 = min(T, t0 + t_per);
    const fe beta = fe_const<C>(GLV<C>::BETA, 1.0);
    xyzz b1 = xyzz_identity(), b2 = b1, b3 = b1, b4 = b1;
    for (u32 t = t0; t < t1; ++t) {
        const int d0 = dig[(size_t)w * T + t];
        const int d1 = H > 1 ? (int)dig[((size_t)DEEP_WMAX + w) * T + t] : 0;
        if ((d0 | d1) == 0) continue;                               // wave-uniform
        affine p = load_table_point(tab0 + (size_t)t * n_k + j0 + jl);
        const bool inf = affine_is_inf(p);
        const fe yneg = fe_select(inf, p.y, fe_canon<C>(fe_neg<C, 2>(p.y)));
        const fe ypos = p.y;
#pragma unroll 1
        for (u32 h = 0; h < 2; ++h) {
            const int d = h ? d1 : d0;
            if (h) p.x = fe_canon<C>(fe_mul<C>(p.x, beta));        // phi keeps (0, 0), the affine identity
            if (d == 0) continue;
            p.y = d < 0 ? yneg : ypos;
            const int m = d < 0 ? -d : d;
            xyzz cur;
            switch (m) {
                case 1: cur = b1; break;
                case 2: cur = b2; break;
                case 3: cur = b3; break;
                default: cur = b4; break;
            }
            cur = xyzz_madd<C>(cur, p);
            switch (m) {
                case 1: b1 = cur; break;
                case 2: b2 = cur; break;
                case 3: b3 = cur; break;
                default: b4 = cur; break;
            }
        }
    }
    // b1 + 2 b2 + 3 b3 + 4 b4 by running sums
    xyzz run = b4, acc = b4;
#pragma unroll 1
    for (int m = 3; m >= 1; --m) {
        const xyzz bm = m == 3 ? b3 : m == 2 ? b2 : b1;
        run = xyzz_add<C>(run, bm);
        acc = xyzz_add<C>(acc, run);
    }
    store_xyzz(part + ((size_t)s * W + w) * cnt + jl, acc);
}
// part[e] += part[s*stride + e] for s = 1 .. S-1 (e < stride = W*cnt)
template <int C>
__global__ void __launch_bounds__(64) k_deep_reduce(xyzz_mem *__restrict__ part, u32 stride, u32 S) {
    const u32 e = blockIdx.x * 64u + threadIdx.x;
    if (e >= stride) return;
    xyzz acc = load_xyzz(part + e);
    for (u32 s = 1; s < S; ++s) acc = xyzz_add<C>(acc, load_xyzz(part + (size_t)s * stride + e));
    store_xyzz(part + e, acc);
}
// out[j] = sum_w 8^w * part[w*cnt + j]: 64 outputs per workgroup of four waves
template <int C>
__global__ void __launch_bounds__(256) k_deep_horner_coop(const xyzz_mem *__restrict__ part, u32 cnt, u32 W, xyzz_mem *__restrict__ out) {
    latency_critical();
    __shared__ CoopLds L;
    const int lane = threadIdx.x & 63, role = threadIdx.x >> 6;
    const u32 i0 = blockIdx.x * 64u + lane;
    const bool live = i0 < cnt;
    const u32 i = live ? i0 : cnt - 1u;                       // idle lanes repeat the last output and store nothing
    xyzz a = load_xyzz_coop(part + (size_t)(W - 1u) * cnt + i);
    for (int w = (int)W - 2; w >= 0; --w) {
        const xyzz y = load_xyzz_coop(part + (size_t)w * cnt + i);   // requested ahead of the doublings
#pragma unroll 1
        for (u32 d = 0; d < DEEP_C; ++d) a = xyzz_dbl_coop<C>(a, L, role, lane);   // one doubling site
        a = xyzz_add_coop<C>(a, y, L, role, lane);
    }
    if (role == 0 && live) store_xyzz(out + i, a);
}

// ---- IPA rounds without generator folding ----------------------------------------------
// After k folds G'_i = w1*G_i + w2*G_{i+half} the generators are
//   G^(k)_i = sum_t coef(t) * G_{i + t*n_k},  n_k = n/2^k,  coef(t) = prod_m (bit_{k-1-m}(t) ? w2_m : w1_m),
// so the cross terms of round k,  L = <a_lo, G^(k)_hi>  and  R = <a_hi, G^(k)_lo>, are MSMs over the
// ORIGINAL (resident, pre-shifted) generators with scalars a[.] * coef(.) -- no 255-step scalar
// multiplication per generator, no re-keying.  k_ipa_coef builds the 2^k coefficients,
// k_ipa_expand the two length-n scalar vectors (canonical integers; half of each is zero and
// costs nothing downstream).
struct IpaChallenges {   // by-value kernel argument: the fold challenges so far (canonical integers)
    fe256 w1[31], w2[31];
};
template <int C>
__global__ void __launch_bounds__(256) k_ipa_coef(IpaChallenges ch, u32 k, fe256 *__restrict__ coef) {
    constexpr int F = 1 - C;
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (1u << k)) return;
    fe acc = fe_one<F>();
    for (u32 m = 0; m < k; ++m) {
        const bool hi = (t >> (k - 1 - m)) & 1u;
        acc = fe_mul<F>(acc, fe_from_integer<F>(hi ? ch.w2[m] : ch.w1[m]));
    }
    store_fe256(coef + t, fe_to_table<F>(acc));
}
template <int C>
__global__ void __launch_bounds__(256) k_ipa_expand(const fe256 *__restrict__ a, u32 n_k, const fe256 *__restrict__ coef, u32 n,
                                                   int is_mont, fe256 *__restrict__ s_l, fe256 *__restrict__ s_r) {
    constexpr int F = 1 - C;
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const u32 half = n_k >> 1;
    const u32 i = j & (n_k - 1u), t = j / n_k;
    const bool upper = i >= half;                       // upper half of its block: belongs to L (with a_lo)
    const fe256 raw = load_fe256(a + (upper ? i - half : i + half));
    const fe x = is_mont ? fe_from_abi<F>(raw) : fe_from_integer<F>(raw);
    const fe v = fe_mul<F>(x, fe_from_table(load_fe256(coef + t)));
    fe one = fe_zero();
    one.l[0] = 1;
    REEF_SET_BOUND(one, 1.0);
    const fe256 out = fe_pack(fe_canon<F>(fe_mul<F>(v, one)));
    fe256 zero;
#pragma unroll
    for (int w = 0; w < 8; ++w) zero.w[w] = 0;
    store_fe256(s_l + j, upper ? out : zero);
    store_fe256(s_r + j, upper ? zero : out);
}

// Both cross terms in one scalar vector (byte-table path: k_wide_accum<C, true> tells them apart by the position of the point
// in its block): s[j] = a[i -/+ half] * coef(t), the non-zero one of (s_l[j], s_r[j]) of k_ipa_expand.
template <int C>
__global__ void __launch_bounds__(256) k_ipa_expand_merged(const fe256 *__restrict__ a, u32 n_k, const fe256 *__restrict__ coef, u32 n, int is_mont,
                                                          fe256 *__restrict__ s) {
    constexpr int F = 1 - C;
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const u32 half = n_k >> 1;
    const u32 i = j & (n_k - 1u), t = j / n_k;
    const fe256 raw = load_fe256(a + (i >= half ? i - half : i + half));
    const fe x = is_mont ? fe_from_abi<F>(raw) : fe_from_integer<F>(raw);
    const fe v = fe_mul<F>(x, fe_from_table(load_fe256(coef + t)));
    fe one = fe_zero();
    one.l[0] = 1;
    REEF_SET_BOUND(one, 1.0);
    store_fe256(s + j, fe_pack(fe_canon<F>(fe_mul<F>(v, one))));
}

// Scalars of a commitment over folded generators (v_msm_folded): s[i] = v[j - off] * coef(t) for i = j + t*n_k with
// off <= j < off + len, zero elsewhere; canonical integers.
template <int C>
__global__ void __launch_bounds__(256) k_fold_expand(const fe256 *__restrict__ v, u32 len, u32 off, u32 n_k, const fe256 *__restrict__ coef, u32 n,
                                                    int is_mont, fe256 *__restrict__ s) {
    constexpr int F = 1 - C;
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 t = i / n_k, j = i - t * n_k;
    fe256 out;
#pragma unroll
    for (int w = 0; w < 8; ++w) out.w[w] = 0;
    if (j >= off && j - off < len) {
        const fe256 raw = load_fe256(v + (j - off));
        const fe x = is_mont ? fe_from_abi<F>(raw) : fe_from_integer<F>(raw);
        const fe val = fe_mul<F>(x, fe_from_table(load_fe256(coef + t)));
        fe one = fe_zero();
        one.l[0] = 1;
        REEF_SET_BOUND(one, 1.0);
        out = fe_pack(fe_canon<F>(fe_mul<F>(val, one)));
    }
    store_fe256(s + i, out);
}

// Sum of `cnt` ABI Jacobian points -> one ABI Jacobian point (multi-GPU combine of per-rank
// partial MSM results after the RCCL all-gather; cnt <= 65536).
template <int C>
__global__ void __launch_bounds__(64) k_sum_points(const jacobian256 *__restrict__ in, u32 cnt, jacobian256 *__restrict__ out) {
    latency_critical();
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    xyzz acc = xyzz_identity();
    for (u32 i = 0; i < cnt; ++i) acc = xyzz_add<C>(acc, xyzz_from_abi_jacobian<C>(load_jacobian256(in + i)));
    store_jacobian256(out, xyzz_to_abi_jacobian<C>(acc));
}

// ------------------------------------------------------- unit-test kernels ----
// Operands and results in ABI form (Montgomery R = 2^256, canonical).
// op: 0 mul, 1 add, 2 sub, 3 inv, 4 to_mont, 5 from_mont, 6 neg, 7 sqr
template <int F>
__global__ void k_test_field(int op, const fe256 *a, const fe256 *b, fe256 *out, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const fe256 xa = load_fe256(a + i), xb = load_fe256(b + i);
    fe256 r;
    if (op == 4) r = fe_to_abi<F>(fe_from_integer<F>(xa));
    else if (op == 5) r = fe_abi_to_integer<F>(xa);
    else {
        const fe x = fe_from_abi<F>(xa), y = fe_from_abi<F>(xb);
        fe z;
        switch (op) {
            case 0: z = fe_mul<F>(x, y); break;
            case 1: z = fe_add<F>(x, y); break;
            case 2: z = fe_sub<F, 2>(x, y); break;
            case 3: z = fe_inv<F>(x); break;
            case 6: z = fe_neg<F, 2>(x); break;
            default: z = fe_sqr<F>(x); break;
        }
        r = fe_to_abi<F>(z);
    }
    store_fe256(out + i, r);
}

// op: 0 madd(P_xyzz, Q_affine), 1 add(P, Q), 2 dbl(P), 3 scalar-mul k*P (k from kbuf)
template <int C>
__global__ void k_test_ec(int op, const affine256 *pa, const affine256 *qa, const fe256 *kbuf, jacobian256 *out, u32 n) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const affine p = affine_from_abi<C>(load_affine256(pa + i)), q = affine_from_abi<C>(load_affine256(qa + i));
    xyzz r;
    if (op == 0) r = xyzz_madd<C>(xyzz_from_affine<C>(p), q);
    else if (op == 1) {
        // push both operands off Z = 1 first so the general formulas are exercised
        xyzz a = xyzz_dbl<C>(xyzz_from_affine<C>(p));
        a = xyzz_madd<C>(a, affine_neg<C>(p));
        xyzz b = xyzz_dbl<C>(xyzz_from_affine<C>(q));
        b = xyzz_madd<C>(b, affine_neg<C>(q));
        r = xyzz_add<C>(a, b);
    } else if (op == 2) r = xyzz_dbl<C>(xyzz_from_affine<C>(p));
    else if (op == 9) {                                   // the one-wave forms of probes 7 / 8
        r = xyzz_from_affine<C>(p);
        const xyzz b = xyzz_dbl<C>(xyzz_from_affine<C>(q));
        for (int k = 0; k < 128; ++k) r = xyzz_add<C>(r, b);                          // P + 256*Q
    } else if (op == 10) {
        r = xyzz_from_affine<C>(p);
        for (int k = 0; k < 64; ++k) r = xyzz_dbl<C>(r);
    } else {
        const fe256 k = load_fe256(kbuf + i);
        r = xyzz_scalar_mul<C>(p, k.w, 255);
    }
    store_jacobian256(out + i, xyzz_to_abi_jacobian<C>(r));
}

// The four-wave forms (ec_coop.h): op 4 general add, 5 double, 6 a chain (P + Q, doubled twice, + P) that reuses the
// LDS slots back to back.  One workgroup of 256 threads per 64 inputs; operands pushed off Z = 1 like op 1.
template <int C>
__global__ void __launch_bounds__(256) k_test_ec_coop(int op, const affine256 *pa, const affine256 *qa, jacobian256 *out, u32 n) {
    __shared__ CoopLds L;
    const int lane = threadIdx.x & 63, role = threadIdx.x >> 6;
    const u32 i = blockIdx.x * 64u + lane;
    const u32 j = i < n ? i : n - 1;                      // every thread takes part in the barriers
    const affine p = affine_from_abi<C>(load_affine256(pa + j)), q = affine_from_abi<C>(load_affine256(qa + j));
    xyzz a = xyzz_dbl<C>(xyzz_from_affine<C>(p));
    a = xyzz_madd<C>(a, affine_neg<C>(p));
    xyzz b = xyzz_dbl<C>(xyzz_from_affine<C>(q));
    b = xyzz_madd<C>(b, affine_neg<C>(q));
    xyzz r;
    if (op == 4) r = xyzz_add_coop<C>(a, b, L, role, lane);
    else if (op == 5) r = xyzz_dbl_coop<C>(a, L, role, lane);
    else if (op == 7) {                                   // latency probes: one call site, executed many times
        r = a;
        for (int k = 0; k < 256; ++k) r = xyzz_add_coop<C>(r, b, L, role, lane);     // P + 256*Q
    } else if (op == 8) {
        r = a;
        for (int k = 0; k < 64; ++k) r = xyzz_dbl_coop<C>(r, L, role, lane);         // 2^64 * P
    } else if (op == 11) {
        r = xyzz_add_coop<C>(a, b, L, role, lane);
        r = xyzz_dbl_coop<C>(r, L, role, lane);
    } else if (op == 12) {
        r = xyzz_add_coop<C>(a, b, L, role, lane);
        r = xyzz_add_coop<C>(r, a, L, role, lane);
    } else if (op == 13) {
        r = xyzz_add_coop<C>(a, b, L, role, lane);
        r = xyzz_dbl_coop<C>(r, L, role, lane);
        r = xyzz_dbl_coop<C>(r, L, role, lane);
    } else if (op == 16) {
        const xyzz r1 = xyzz_dbl_coop<C>(a, L, role, lane);
        asm volatile("" ::: "memory");
        r = xyzz_dbl_coop<C>(r1, L, role, lane);
    } else if (op == 17) {
        r = a;
        for (int k = 0; k < 2; ++k) r = xyzz_dbl_coop<C>(r, L, role, lane);
    } else if (op == 18) {
        r = a;
#pragma unroll 1
        for (int k = 0; k < 2; ++k) r = xyzz_dbl_coop<C>(r, L, role, lane);
    } else if (op == 20) {                                // doubling, then an addition that falls into its own shared doubling (P + P)
        const xyzz r1 = xyzz_dbl_coop<C>(a, L, role, lane);
        r = xyzz_add_coop<C>(r1, r1, L, role, lane);
    } else if (op == 21) {                                // Z = 1 operands (table entries of the generator fold)
        r = xyzz_add_coop<C>(xyzz_from_affine<C>(p), xyzz_from_affine<C>(q), L, role, lane);
    } else if (op == 22) {                                // a step machine (one addition site, one doubling site): T = P + Q, then 7*T by doubling and adding
        xyzz t = xyzz_identity(), acc = xyzz_identity();
        for (int k = -1; k < 3; ++k) {
            xyzz x, y;
            if (k < 0) { x = xyzz_from_affine<C>(p); y = xyzz_from_affine<C>(q); }
            else { acc = xyzz_dbl_coop<C>(acc, L, role, lane); x = acc; y = t; }
            const xyzz s = xyzz_add_coop<C>(x, y, L, role, lane);
            if (k < 0) t = s; else acc = s;
        }
        r = acc;
    } else if (op == 14) {
        r = xyzz_dbl_coop<C>(a, L, role, lane);
        r = xyzz_add_coop<C>(r, b, L, role, lane);
    } else if (op == 15) {
        r = xyzz_dbl_coop<C>(a, L, role, lane);
        r = xyzz_dbl_coop<C>(r, L, role, lane);
        r = xyzz_add_coop<C>(r, b, L, role, lane);
    } else {
        r = xyzz_add_coop<C>(a, b, L, role, lane);
        r = xyzz_dbl_coop<C>(r, L, role, lane);
        r = xyzz_dbl_coop<C>(r, L, role, lane);
        r = xyzz_add_coop<C>(r, a, L, role, lane);
    }
    if (role == (int)(blockIdx.x & 3u) && i < n) store_jacobian256(out + i, xyzz_to_abi_jacobian<C>(r));   // every wave must hold the result: take a different one per block
}

template <int C>
__global__ void __launch_bounds__(256) k_test_dd(int op, const affine256 *pa, jacobian256 *out, u32 n) {
    __shared__ CoopLds L;
    const int lane = threadIdx.x & 63, role = threadIdx.x >> 6;
    const u32 i = blockIdx.x * 64u + lane;
    const u32 j = i < n ? i : n - 1;
    const affine p = affine_from_abi<C>(load_affine256(pa + j));
    xyzz a = xyzz_dbl<C>(xyzz_from_affine<C>(p));
    a = xyzz_madd<C>(a, affine_neg<C>(p));
    xyzz r = xyzz_dbl_coop<C>(a, L, role, lane);
    r = xyzz_dbl_coop<C>(r, L, role, lane);
    if (role == (int)(blockIdx.x & 3u) && i < n) store_jacobian256(out + i, xyzz_to_abi_jacobian<C>(r));
}

// Throughput probe: `iters` x 2 dependent Montgomery products per thread.
template <int F>
__global__ void __launch_bounds__(256) k_bench_fmul(fe256 *io, u32 iters) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    fe x = fe_from_abi<F>(load_fe256(io + 2 * i));
    fe y = fe_from_abi<F>(load_fe256(io + 2 * i + 1));
    for (u32 k = 0; k < iters; ++k) {
        x = fe_mul<F>(x, y);
        y = fe_mul<F>(y, x);
    }
    store_fe256(io + 2 * i, fe_to_abi<F>(x));
    store_fe256(io + 2 * i + 1, fe_to_abi<F>(y));
}

}  // namespace reef
