// Row N2 of SURVEY.md 8f: the host sum-check of Reef's nlookup witness generation as vector
// kernels over the scalar field (Pallas scalars = Fq = the CirC modulus, r1cs_helper.rs:37-38).
//
// Reference functions (src/backend/r1cs_helper.rs), called once per folding step from
// wit_nlookup_gadget (src/backend/r1cs.rs:2177-2393, loop :2343-2376):
//   linear_mle_product   :441-506  -> k_sc_coeffs (the three sums, :455-476)
//                                     k_sc_fold   (both tables, :491-503); the Poseidon challenge
//                                     between the two (:478-489) stays on the host
//   gen_eq_table         :508-544  -> k_sc_eq_factors + k_sc_eq_table + k_sc_eq_points
//   prover_mle_partial_eval(for_t, no hole) / verifier_mle_eval :551-641
//                                  -> nothing to compute: after the last round the folded table
//                                     holds T~(r) in entry 0
// On the host these are O(N) rug::Integer multiplications with rem_floor per step over tables
// of 2^21..2^26 entries.  Here a table entry is 32 B in HBM (internal Montgomery form), a
// round streams both tables once: this path is HBM-bound, unlike the MSM.
//
// Included by kernels_<curve>.hip after fe_vec.h; F = scalar field of the curve.

namespace reef {

// (xsq, sum t1 e1, con) as 27 limb sums -> the three coefficients (xsq, x, con) as canonical integers
template <int F> __device__ __forceinline__ void sc_coeffs_from_limb_sums(const unsigned long long *tot, fe256 *out3) {
    fe v[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        fe_wide w;
#pragma unroll
        for (int i = 0; i < 9; ++i) w.l[i] = tot[9 * k + i];
        v[k] = fe_from_limb_sums<F>(w);   // < 2
    }
    const fe x = fe_sub<F, 2>(fe_sub<F, 2>(v[1], v[2]), v[0]);   // x = sum t1*e1 - con - xsq
    store_fe256(out3 + 0, fe_to_integer<F>(v[0]));
    store_fe256(out3 + 1, fe_to_integer<F>(x));
    store_fe256(out3 + 2, fe_to_integer<F>(v[2]));
}

// A round in ONE launch: every block adds its 27 limb sums to `gacc` (device-scope atomics; the returned values are
// consumed, so the additions have been performed before the block takes its ticket), and the block that draws the last
// ticket turns the totals into the coefficients, writes them where the host reads them (pinned memory) and leaves gacc and
// the ticket counter at zero for the next round.  Saves the second launch and the copy of every round: ~15 us of the
// ~55 us a small round takes (21 of the 26 rounds of a 2^26-entry step are small).  gacc[27] is the ticket counter.
// The word after the three coefficients (pinned host memory) takes the call's sequence number once they are written: the
// host polls it instead of going through hipStreamSynchronize (12 -> 6.6 us per launch-and-wait, reef_amd/_lib/sync_probe).
// What the host polls is written through to system scope (sc0 sc1) and waited for, flag last: a system-scope FENCE also writes the
// XCD's L2 back -- the freshly folded table -- which nobody outside the device reads (2-3 us of a ~10 us round).
__device__ __forceinline__ void sc_post_fe256(fe256 *p, const fe256 &s) {
    typedef u32 v4 __attribute__((ext_vector_type(4)));
    const v4 lo = {s.w[0], s.w[1], s.w[2], s.w[3]}, hi = {s.w[4], s.w[5], s.w[6], s.w[7]};
    asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\tglobal_store_dwordx4 %0, %2, off offset:16 sc0 sc1" : : "v"(p), "v"(lo), "v"(hi) : "memory");
}
__device__ __forceinline__ void sc_signal_host(fe256 *out3, u32 seq) {   // by a lane of the wave that posted: its stores are acknowledged first
    asm volatile("s_waitcnt vmcnt(0)\n\tglobal_store_dword %0, %1, off sc0 sc1" : : "v"(out3 + 3), "v"(seq) : "memory");
}
// The last step of a one-launch round, by the whole block: the three limb groups are folded back by three waves at once (a lone
// thread took ~6 us for them, a quarter of a small round), lanes 0..2 of the first wave combine and post, lane 0 signals.
template <int F>
__device__ __forceinline__ void sc_finish_parallel(const unsigned long long *tot /* shared, 27 */, fe256 *__restrict__ out3, u32 seq) {
    __shared__ u32 conv[3][9];
    __syncthreads();
    if ((threadIdx.x & 63) == 0 && threadIdx.x < 192) {
        const u32 k = threadIdx.x >> 6;
        fe_wide w;
#pragma unroll
        for (int i = 0; i < 9; ++i) w.l[i] = tot[9 * k + i];
        const fe x = fe_from_limb_sums<F>(w);   // < 2
#pragma unroll
        for (int i = 0; i < 9; ++i) conv[k][i] = x.l[i];
    }
    __syncthreads();
    if (threadIdx.x < 64) {                                   // one wave: its s_waitcnt covers the stores of lanes 0..2
        if (threadIdx.x < 3) {                                // xsq, x, con: one lane each
            fe v[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
#pragma unroll
                for (int i = 0; i < 9; ++i) v[k].l[i] = conv[k][i];
                REEF_SET_BOUND(v[k], 2.0);
            }
            const fe x = fe_sub<F, 2>(fe_sub<F, 2>(v[1], v[2]), v[0]);
            const fe pick = threadIdx.x == 0 ? v[0] : threadIdx.x == 1 ? x : v[2];
            sc_post_fe256(out3 + threadIdx.x, fe_to_integer<F>(pick));
        }
        if (threadIdx.x == 0) sc_signal_host(out3, seq);
    }
}
// How the last block of a multi-block one-launch round learns that every other block's additions to `gacc` have been performed
// (REEF_SC_FENCE, read once per step; tests/test_gpu_sumcheck.py runs the stress test under all three):
//   SC_ORDER_RETURNS (0; rounds 4-5 shipped it, since round 6 the documented opt-in REEF_SC_FENCE=0) -- no fence.  The argument, in terms of what the ISA does, not of the HIP memory model
//     (which gives relaxed atomics on different addresses no order):
//       (1) the 27 additions and the ticket are `global_atomic_add_x2 ... sc1` WITH RETURN (glc): device-scope read-modify-writes on
//           gfx942/gfx950 are not performed in the issuing XCD's L2 -- the eight L2s are not coherent with each other -- but forwarded to the
//           memory side (the data fabric's atomic unit in front of the Infinity Cache), the one place every XCD's sc1 accesses meet;
//       (2) a returning atomic's value comes back through the vector memory return path and is counted by vmcnt: after
//           `s_waitcnt vmcnt(0)` in wave 0 (threads 0..26 issue the additions, thread 0 the ticket -- the same wave) every addition
//           of this block HAS been performed at the memory side; the `memory` clobber keeps the compiler from moving the ticket up;
//       (3) the ticket is issued after that wait, so in the memory side's order it follows the block's additions; the block that
//           draws ticket nblocks - 1 therefore follows all additions of all blocks, and it reads the totals with atomicExch --
//           again a device-scope RMW performed at the memory side, never served from its XCD's L2.
//     No plain load or store takes part in the hand-over, so there is nothing for a cache to hold stale.
//   SC_ORDER_THREADFENCE (1) -- round 4's first form: __threadfence() before the ticket (release at agent scope: s_waitcnt + buffer_wbl2
//     sc1, which also writes back the table the block has just folded: 2-4 us per block).
//   SC_ORDER_RELEASE_TICKET (2, THE DEFAULT since round 6) -- the form the HIP memory model blesses (ADVICE r4, r5): the ticket is an acq_rel RMW at
//     agent scope, the additions relaxed; the compiler emits the same write-back for the release half.
// Why 2 ships although 0 never failed a stress run (2.4 x 10^7 rounds): bit-exactness is the path's first bar, and 0 rests on where gfx950 performs
// sc1 atomics -- hardware behaviour the memory model does not promise, which a firmware or part change would void silently.  What the principle
// costs (tools/fence_cost.sh, profiles/r06_fence_cost.txt, medians of five alternating replays on one box): cfg3's sum-check step 0.514 -> 0.538 ms
// (+24 us, +4.7 %), cfg4's 1.537 -> 1.511 ms (within noise) -- microseconds against a proof's tens of milliseconds.
enum { SC_ORDER_RETURNS = 0, SC_ORDER_THREADFENCE = 1, SC_ORDER_RELEASE_TICKET = 2 };
template <int F>
__device__ __forceinline__ void sc_round_epilogue(const unsigned long long *acc /* shared, 27 */, unsigned long long *__restrict__ gacc, u32 nblocks,
                                                  fe256 *__restrict__ out3, u32 seq, u32 order) {
    __shared__ unsigned long long tot[27];
    __shared__ int last;
    if (nblocks == 1) {                                        // a small round: this block's sums are the totals
        sc_finish_parallel<F>(acc, out3, seq);
        return;
    }
    unsigned long long seen = 0;
    if (threadIdx.x < 27) seen = atomicAdd(&gacc[threadIdx.x], acc[threadIdx.x]);
    if (seen == ~0ull) tot[0] = seen;                          // never true (limb sums stay below 2^60): keeps the returned value live
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");           // the additions' returns have arrived: they are performed (see above)
    if (order == SC_ORDER_THREADFENCE) __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long t = order == SC_ORDER_RELEASE_TICKET ? __hip_atomic_fetch_add(&gacc[27], 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT)
                                                                      : atomicAdd(&gacc[27], 1ull);
        last = t == (unsigned long long)(nblocks - 1);
    }
    __syncthreads();
    if (!last) return;
    if (order == SC_ORDER_THREADFENCE) __threadfence();
    if (threadIdx.x < 27) tot[threadIdx.x] = atomicExch(&gacc[threadIdx.x], 0ull);
    __syncthreads();
    if (threadIdx.x == 0) atomicExch(&gacc[27], 0ull);
    sc_finish_parallel<F>(tot, out3, seq);
}

// One sum-check round, first half: with pow = 2^(ell-i) and (t0, t1, e0, e1) =
// (T[b], T[b+pow], E[b], E[b+pow]):
//   xsq = sum (t1-t0)(e1-e0),  x = sum (e1-e0) t0 + (t1-t0) e0,  con = sum t0 e0.
// x = sum t1 e1 - con - xsq, so three products per pair suffice; their limb products are accumulated
// unreduced (fe_wide18) and reduced once per thread.  Each block leaves 27 64-bit limb sums
// (xsq, sum t1 e1, con) in partial[block][27].
template <int F>
__global__ void __launch_bounds__(256) k_sc_coeffs(const fe256 *__restrict__ T, const fe256 *__restrict__ E, u32 pow,
                                                  unsigned long long *__restrict__ partial, unsigned long long *__restrict__ gacc,
                                                  fe256 *__restrict__ out3, u32 seq, u32 order) {
    __shared__ unsigned long long acc[27];
    if (threadIdx.x < 27) acc[threadIdx.x] = 0;
    __syncthreads();
    fe_wide18 aq, a11, ac;
    wide18_zero(aq);
    wide18_zero(a11);
    wide18_zero(ac);
    u32 since = 0;
    for (u32 b = blockIdx.x * blockDim.x + threadIdx.x; b < pow; b += gridDim.x * blockDim.x) {
        const fe t0 = fe_from_table(load_fe256(T + b)), t1 = fe_from_table(load_fe256(T + b + pow));
        const fe e0 = fe_from_table(load_fe256(E + b)), e1 = fe_from_table(load_fe256(E + b + pow));
        const fe ts = fe_sub<F, 2>(t1, t0);   // < 3
        const fe es = fe_sub<F, 2>(e1, e0);
        wide18_mac(aq, ts.l, es.l);
        wide18_mac(a11, t1.l, e1.l);
        wide18_mac(ac, t0.l, e0.l);
        if (++since == 4) {
            wide18_carry(aq);
            wide18_carry(a11);
            wide18_carry(ac);
            since = 0;
        }
    }
    const fe rq = wide18_reduce<F>(aq), r11 = wide18_reduce<F>(a11), rc = wide18_reduce<F>(ac);
    fe_wide wq, wx, wc;   // wx carries sum t1*e1; the final kernel turns it into x
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        wq.l[i] = rq.l[i];
        wx.l[i] = r11.l[i];
        wc.l[i] = rc.l[i];
    }
    // wave-level tree first (shuffles), then one LDS atomic per limb per wave
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const unsigned long long a = wave_sum63(wq.l[i]), b = wave_sum63(wx.l[i]), c = wave_sum63(wc.l[i]);
        if ((threadIdx.x & 63) == 63) {
            atomicAdd(&acc[i], a);
            atomicAdd(&acc[9 + i], b);
            atomicAdd(&acc[18 + i], c);
        }
    }
    __syncthreads();
    if (gacc) { sc_round_epilogue<F>(acc, gacc, gridDim.x, out3, seq, order); return; }
    if (threadIdx.x < 27) partial[(size_t)blockIdx.x * 27 + threadIdx.x] = acc[threadIdx.x];
}

// Sums the per-block limb sums -- 37 groups of 27 threads, a group reads the 27 consecutive sums of a block, blocks round robin --
// and posts (xsq, x, con) as canonical integers where the host polls (pinned memory, then the sequence word): no copy, no stream wait.
template <int F>
__global__ void __launch_bounds__(1024) k_sc_coeffs_final(const unsigned long long *__restrict__ partial, u32 nblocks,
                                                         fe256 *__restrict__ host3, u32 seq) {
    __shared__ unsigned long long tot[27];
    if (threadIdx.x < 27) tot[threadIdx.x] = 0;
    __syncthreads();
    const u32 slot = threadIdx.x % 27, grp = threadIdx.x / 27;
    if (grp < 37) {
        // four loads in flight per thread: one after the other they cost their latency each (2048 blocks: 21 us for 440 KB)
        unsigned long long s = 0, s1 = 0, s2 = 0, s3 = 0;
        u32 k = grp;
        for (; k + 3 * 37 < nblocks; k += 4 * 37) {
            s += partial[(size_t)k * 27 + slot];
            s1 += partial[(size_t)(k + 37) * 27 + slot];
            s2 += partial[(size_t)(k + 2 * 37) * 27 + slot];
            s3 += partial[(size_t)(k + 3 * 37) * 27 + slot];
        }
        for (; k < nblocks; k += 37) s += partial[(size_t)k * 27 + slot];
        s += s1 + s2 + s3;
        if (s) atomicAdd(&tot[slot], s);
    }
    sc_finish_parallel<F>(tot, host3, seq);                   // limb sums of (xsq, sum t1*e1, con); begins with a barrier
}

// Second half of the round: X[b] = X[b]*(1 - r) + X[b+pow]*r = X[b] + r*(X[b+pow] - X[b]) for
// both tables, in place.  r arrives as a canonical integer.
template <int F>
__global__ void __launch_bounds__(256) k_sc_fold(const fe256 *Tsrc, fe256 *T, fe256 *__restrict__ E, u32 pow, fe256 r_int) {
    // Tsrc == T (in place) or the pristine copy of the table (first fold of a step: no reset copy needed);
    // a thread reads b and b+pow and writes b only, so in-place is safe
    const fe r = fe_from_integer<F>(r_int);
    for (u32 b = blockIdx.x * blockDim.x + threadIdx.x; b < pow; b += gridDim.x * blockDim.x) {
        const fe t0 = fe_from_table(load_fe256(Tsrc + b)), t1 = fe_from_table(load_fe256(Tsrc + b + pow));
        const fe e0 = fe_from_table(load_fe256(E + b)), e1 = fe_from_table(load_fe256(E + b + pow));
        const fe tn = fe_add<F>(t0, fe_mul<F>(r, fe_sub<F, 2>(t1, t0)));   // < 2.03
        const fe en = fe_add<F>(e0, fe_mul<F>(r, fe_sub<F, 2>(e1, e0)));
        store_fe256(T + b, fe_to_table<F>(tn));
        store_fe256(E + b, fe_to_table<F>(en));
    }
}

// Fold of round i fused with the coefficient sums of round i+1: with h = pow/2, thread b < h
// folds the entries {b, b+h} of both tables (reading their partners at +pow), writes them, and
// feeds the fresh values straight into the next round's three sums -- one pass over the tables
// per round instead of two.
template <int F>
__global__ void __launch_bounds__(256) k_sc_fold_coeffs(const fe256 *Tsrc, fe256 *T, fe256 *__restrict__ E, u32 pow, fe256 r_int,
                                                       unsigned long long *__restrict__ partial, unsigned long long *__restrict__ gacc,
                                                       fe256 *__restrict__ out3, u32 seq, u32 order) {
    __shared__ unsigned long long acc[27];
    if (threadIdx.x < 27) acc[threadIdx.x] = 0;
    __syncthreads();
    const fe r = fe_from_integer<F>(r_int);
    const u32 h = pow >> 1;
    fe_wide18 aq, a11, ac;
    wide18_zero(aq);
    wide18_zero(a11);
    wide18_zero(ac);
    u32 since = 0;
    for (u32 b = blockIdx.x * blockDim.x + threadIdx.x; b < h; b += gridDim.x * blockDim.x) {
        fe t0, t1, e0, e1;
        {
            const fe a0 = fe_from_table(load_fe256(Tsrc + b)), a1 = fe_from_table(load_fe256(Tsrc + b + pow));
            t0 = fe_canon<F>(fe_add<F>(a0, fe_mul<F>(r, fe_sub<F, 2>(a1, a0))));
            const fe c0 = fe_from_table(load_fe256(Tsrc + b + h)), c1 = fe_from_table(load_fe256(Tsrc + b + h + pow));
            t1 = fe_canon<F>(fe_add<F>(c0, fe_mul<F>(r, fe_sub<F, 2>(c1, c0))));
        }
        {
            const fe a0 = fe_from_table(load_fe256(E + b)), a1 = fe_from_table(load_fe256(E + b + pow));
            e0 = fe_canon<F>(fe_add<F>(a0, fe_mul<F>(r, fe_sub<F, 2>(a1, a0))));
            const fe c0 = fe_from_table(load_fe256(E + b + h)), c1 = fe_from_table(load_fe256(E + b + h + pow));
            e1 = fe_canon<F>(fe_add<F>(c0, fe_mul<F>(r, fe_sub<F, 2>(c1, c0))));
        }
        store_fe256(T + b, fe_pack(t0));
        store_fe256(T + b + h, fe_pack(t1));
        store_fe256(E + b, fe_pack(e0));
        store_fe256(E + b + h, fe_pack(e1));
        const fe ts = fe_sub<F, 2>(t1, t0);
        const fe es = fe_sub<F, 2>(e1, e0);
        wide18_mac(aq, ts.l, es.l);
        wide18_mac(a11, t1.l, e1.l);
        wide18_mac(ac, t0.l, e0.l);
        if (++since == 4) {
            wide18_carry(aq);
            wide18_carry(a11);
            wide18_carry(ac);
            since = 0;
        }
    }
    const fe rq = wide18_reduce<F>(aq), r11 = wide18_reduce<F>(a11), rc = wide18_reduce<F>(ac);
    fe_wide wq, wx, wc;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        wq.l[i] = rq.l[i];
        wx.l[i] = r11.l[i];
        wc.l[i] = rc.l[i];
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const unsigned long long a = wave_sum63(wq.l[i]), b2 = wave_sum63(wx.l[i]), c = wave_sum63(wc.l[i]);
        if ((threadIdx.x & 63) == 63) {
            atomicAdd(&acc[i], a);
            atomicAdd(&acc[9 + i], b2);
            atomicAdd(&acc[18 + i], c);
        }
    }
    __syncthreads();
    if (gacc) { sc_round_epilogue<F>(acc, gacc, gridDim.x, out3, seq, order); return; }
    if (threadIdx.x < 27) partial[(size_t)blockIdx.x * 27 + threadIdx.x] = acc[threadIdx.x];
}

// The same round for small tables, with the work of an item spread over the four waves of a workgroup: what a small round costs is
// the dependent chain of ONE thread (four folds, three products, three reductions: ~12 products one after the other, 17-20 us
// whatever the size), so wave w folds one of the four entries of item `lane` (t0, t1, e0, e1), the values meet in LDS, and waves
// 0..2 take one of the three products each -- a plain Montgomery product, reduced at once: with one product per thread there is
// nothing for a lazy reduction to save.  Two products deep instead of twelve.  Always a one-launch round.
template <int F>
__global__ void __launch_bounds__(256) k_sc_fold_coeffs_split(const fe256 *Tsrc, fe256 *T, fe256 *E, u32 pow, fe256 r_int,
                                                             unsigned long long *__restrict__ gacc, fe256 *__restrict__ out3, u32 seq, u32 order) {
    __shared__ u32 sh[4][64][9];
    __shared__ unsigned long long acc[27];
    const u32 role = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const u32 h = pow >> 1;
    if (threadIdx.x < 27) acc[threadIdx.x] = 0;
    const fe256 *src = role < 2 ? Tsrc : (const fe256 *)E;
    fe256 *dst = role < 2 ? T : E;
    const u32 off = (role & 1u) ? h : 0u;
    u32 base = blockIdx.x * 64u;                               // uniform over the workgroup
    fe a0 = fe_zero(), d = fe_zero();
    if (base + lane < h) {
        a0 = fe_from_table(load_fe256(src + base + lane + off));
        d = fe_sub<F, 2>(fe_from_table(load_fe256(src + base + lane + off + pow)), a0);
    }
    const fe r = fe_from_integer<F>(r_int);
    unsigned long long s[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) s[i] = 0;
    for (;;) {
        const u32 b = base + lane;
        fe v = fe_zero();
        if (b < h) {
            v = fe_canon<F>(fe_add<F>(a0, fe_mul<F>(r, d)));
            store_fe256(dst + b + off, fe_pack(v));
        }
#pragma unroll
        for (int i = 0; i < 9; ++i) sh[role][lane][i] = v.l[i];
        __syncthreads();
        if (role < 3) {                                        // 0: (t1-t0)(e1-e0), 1: t1 e1, 2: t0 e0; an idle lane holds zeros
            fe x, y;
            if (role == 0) {
                fe t0, t1, e0, e1;
#pragma unroll
                for (int i = 0; i < 9; ++i) { t0.l[i] = sh[0][lane][i]; t1.l[i] = sh[1][lane][i]; e0.l[i] = sh[2][lane][i]; e1.l[i] = sh[3][lane][i]; }
                REEF_SET_BOUND(t0, 1.0); REEF_SET_BOUND(t1, 1.0); REEF_SET_BOUND(e0, 1.0); REEF_SET_BOUND(e1, 1.0);
                x = fe_sub<F, 2>(t1, t0);
                y = fe_sub<F, 2>(e1, e0);
            } else {
                const u32 a = role == 1 ? 1u : 0u;
#pragma unroll
                for (int i = 0; i < 9; ++i) { x.l[i] = sh[a][lane][i]; y.l[i] = sh[2 + a][lane][i]; }
                REEF_SET_BOUND(x, 1.0); REEF_SET_BOUND(y, 1.0);
            }
            const fe p = fe_mul<F>(x, y);                      // < 2, limbs normalised
#pragma unroll
            for (int i = 0; i < 9; ++i) s[i] += p.l[i];
        }
        base += gridDim.x * 64u;
        if (base >= h) break;
        __syncthreads();                                       // the next items overwrite sh
        a0 = fe_zero();
        d = fe_zero();
        if (base + lane < h) {
            a0 = fe_from_table(load_fe256(src + base + lane + off));
            d = fe_sub<F, 2>(fe_from_table(load_fe256(src + base + lane + off + pow)), a0);
        }
    }
    if (role < 3) {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            const unsigned long long a = wave_sum63(s[i]);
            if (lane == 63) acc[9 * role + i] = a;
        }
    }
    __syncthreads();
    sc_round_epilogue<F>(acc, gacc, gridDim.x, out3, seq, order);
}

// gen_eq_table: eq[i] = sum_{k: qs[k] = i} rs[k] + rs[nq] * prod_j (bit_j(i) ? last_q[j] : 1 - last_q[j]).
// The product splits into a factor of the high index bits and one of the low bits, so two small
// tables (2^hi and 2^lo entries, a few hundred KB, cache-resident) turn the O(N*ell) loop of the
// reference into one product per entry.
template <int F>
__global__ void __launch_bounds__(256) k_sc_eq_factors(const fe256 *__restrict__ last_q_int, u32 ell, u32 lo_bits,
                                                      fe256 rs_last_int, fe256 *__restrict__ fac_hi, fe256 *__restrict__ fac_lo) {
    const u32 hi_bits = ell - lo_bits;
    const u32 n_hi = 1u << hi_bits, n_lo = 1u << lo_bits;
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_hi + n_lo) return;
    const bool is_hi = t < n_hi;
    const u32 idx = is_hi ? t : t - n_hi;
    const u32 j0 = is_hi ? lo_bits : 0, nb = is_hi ? hi_bits : lo_bits;
    fe acc = is_hi ? fe_from_integer<F>(rs_last_int) : fe_one<F>();   // rs[nq] rides on the high factor
    for (u32 k = 0; k < nb; ++k) {
        const fe q = fe_from_integer<F>(load_fe256(last_q_int + j0 + k));
        const fe om = fe_sub<F, 2>(fe_one<F>(), q);
        acc = fe_mul<F>(acc, ((idx >> k) & 1u) ? q : om);
    }
    store_fe256((is_hi ? fac_hi : fac_lo) + idx, fe_to_table<F>(acc));
}
template <int F>
__global__ void __launch_bounds__(256) k_sc_eq_table(const fe256 *__restrict__ fac_hi, const fe256 *__restrict__ fac_lo,
                                                    u32 ell, u32 lo_bits, fe256 *__restrict__ out) {
    const u32 n = 1u << ell;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const fe a = fe_from_table(load_fe256(fac_hi + (i >> lo_bits)));
        const fe b = fe_from_table(load_fe256(fac_lo + (i & ((1u << lo_bits) - 1u))));
        store_fe256(out + i, fe_to_table<F>(fe_mul<F>(a, b)));
    }
}
// eq[qs[k]] += rs[k].  qs may repeat: the first mass of an index adds all of them, the others do nothing -- a thread per mass, no
// order to keep (one thread in a loop: 37 us for 64 masses, most of gen_eq_table at 2^21 entries)
template <int F>
__global__ void __launch_bounds__(64) k_sc_eq_points(const fe256 *__restrict__ rs_int, const u32 *__restrict__ qs, u32 nq, fe256 *__restrict__ eq) {
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nq) return;
    const u32 q = qs[k];
    for (u32 j = 0; j < k; ++j)
        if (qs[j] == q) return;
    fe sum = fe_from_table(load_fe256(eq + q));
    for (u32 j = k; j < nq; ++j)
        if (qs[j] == q) sum = fe_canon<F>(fe_add<F>(sum, fe_from_integer<F>(load_fe256(rs_int + j))));
    store_fe256(eq + q, fe_pack(sum));
}

// ---- the EQ table kept as what it is: a rank-one table plus a few point masses --------------------------------------------
// gen_eq_table (r1cs_helper.rs:508-544) gives  EQ[i] = FH[i >> lo] * FL[i & (2^lo - 1)] + sum_k rs[k] [i == qs[k]]  (FH carries
// rs[nq]).  A round folds the TOP index bit (pairs b, b + pow; :491-503), i.e. a bit of the FH index, and
//   EQ'[b] = EQ[b] + r (EQ[b + pow] - EQ[b]) = FH'[b >> lo] * FL[b & ..] + masses',   FH'[h] = FH[h] + r (FH[h + H/2] - FH[h]),
// a mass (q, w) becoming (q mod pow, w * (q >= pow ? r : 1 - r)).  So while the rounds fold FH bits (the first ell - lo of
// them) EQ is never written or read as a table: the three sums of a round (:455-476) are, with u = column index,
//   con = sum_u FL[u] * sum_h FH[h] T[h, u],   sum t1 e1 = sum_u FL[u] * sum_h FH[h + H/2] T[h + H/2, u],
//   xsq = sum_u FL[u] * sum_h (FH[h + H/2] - FH[h]) (T[h + H/2, u] - T[h, u])          (h < H/2, T as a matrix of 2^lo columns)
// plus the masses' share (k_sc_r1_final) -- one pass over T per round with the row factors in scalar registers, where the
// dense form streamed T and EQ and folded both.  Half the bytes and fewer than half the products per round; the EQ table
// (32 B x 2^ell written by gen_eq_table, read twice in round one) is gone.  When the FH bits are used up (pow < 2^lo) the
// 2^lo live entries are written out once (k_sc_eq_table + k_sc_r1_masses) and the dense kernels above finish the job.

// Row factors of a round, h < hn: f0[h] = FH[h], f1[h] = FH[h + hn], fd[h] = f1 - f0 (unpacked limbs: every lane reads the same h).

// Folds FH with r (has_r), moves the masses along, and tabulates the row factors of the NEXT sums (hn_next pair rows of the
// folded FH).  hc = rows of FH before the fold (a power of two); pow = entries per half before the fold.
template <int F>
__global__ void __launch_bounds__(256) k_sc_r1_prep(fe256 *__restrict__ fh, u32 hc, int has_r, fe256 r_int, u32 hn_next, fe_limbs *__restrict__ l0,
                                                   fe_limbs *__restrict__ l1, fe_limbs *__restrict__ ld, u32 *__restrict__ mq, fe256 *__restrict__ mw,
                                                   u32 nq, u32 pow) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 hh = hc >> 1;                                   // rows after the fold
    fe r = fe_zero();
    if (has_r) r = fe_from_integer<F>(r_int);
    if (has_r && t < nq) {                                    // masses: (q, w) -> (q mod pow, w * (q >= pow ? r : 1 - r))
        const u32 q = mq[t];
        const fe w = fe_from_table(load_fe256(mw + t));
        const fe k = q >= pow ? r : fe_sub<F, 2>(fe_one<F>(), r);
        store_fe256(mw + t, fe_to_table<F>(fe_mul<F>(w, k)));
        mq[t] = q >= pow ? q - pow : q;
    }
    if (has_r && hn_next == 0) {                              // last FH bit: a single row is left
        if (t == 0) {
            const fe a = fe_from_table(load_fe256(fh)), b = fe_from_table(load_fe256(fh + 1));
            store_fe256(fh, fe_to_table<F>(fe_add<F>(a, fe_mul<F>(r, fe_sub<F, 2>(b, a)))));
        }
        return;
    }
    if (t >= hn_next) return;                                 // hn_next = rows_now / 2
    fe a, b;
    if (has_r) {      // thread t folds the rows t and t + hn_next (reads t, t + hh, t + hn_next, t + hn_next + hh: its own indices only)
        const fe a0 = fe_from_table(load_fe256(fh + t)), a1 = fe_from_table(load_fe256(fh + t + hh));
        const fe b0 = fe_from_table(load_fe256(fh + t + hn_next)), b1 = fe_from_table(load_fe256(fh + t + hn_next + hh));
        a = fe_canon<F>(fe_add<F>(a0, fe_mul<F>(r, fe_sub<F, 2>(a1, a0))));
        b = fe_canon<F>(fe_add<F>(b0, fe_mul<F>(r, fe_sub<F, 2>(b1, b0))));
        store_fe256(fh + t, fe_pack(a));
        store_fe256(fh + t + hn_next, fe_pack(b));
    } else {
        a = fe_from_table(load_fe256(fh + t));
        b = fe_from_table(load_fe256(fh + t + hn_next));
    }
    l0[t] = fe_to_limbs(a);
    l1[t] = fe_to_limbs(b);
    ld[t] = fe_to_limbs(fe_canon<F>(fe_sub<F, 2>(b, a)));
}

// Every block of a rank-one sums kernel leaves R1_SLOTS limb sums: what adds to xsq [0,9), sum t1 e1 [9,18), con [18,27), and
// what is taken from xsq [27,36) (the masses and the per-side kernels of a structured table use the last one).
static constexpr u32 R1_SLOTS = 36;
// The blocks of a round's sums kernels do not leave their sums side by side (k_sc_r1_final read 1000-2300 x 288 bytes through ONE
// workgroup: 6-11 us of every structured round): a block ADDS its 36 limb sums to one of R1_GROUPS accumulator sets, chosen by
// its number -- ~64-146 additions per word, spread over the kernel's run time and off the round's critical path -- and the final
// kernel reads 16 x 36 words and leaves them at zero for the next round (the accumulators are zero between rounds).
static constexpr u32 R1_GROUPS = 16;
__device__ __forceinline__ void r1_emit(unsigned long long *__restrict__ accs, const unsigned long long *acc /* shared, R1_SLOTS */, u32 block) {
    if (threadIdx.x < R1_SLOTS) {
        const unsigned long long v = acc[threadIdx.x];
        if (v) atomicAdd(&accs[(block % R1_GROUPS) * R1_SLOTS + threadIdx.x], v);
    }
}

// The shared tail of the two sum kernels: every thread multiplies its three column sums by FL[u], the block leaves its limb sums.
template <int F, bool S11 = true>
__device__ __forceinline__ void r1_block_sums(fe_wide18 &aq, fe_wide18 &a11, fe_wide18 &ac, bool live, const fe256 *__restrict__ fl, u32 u,
                                              unsigned long long *acc /* shared, R1_SLOTS, zeroed */, unsigned long long *__restrict__ accs) {
    fe_wide wq, wx, wc;
    wide_zero(wq);
    wide_zero(wx);
    wide_zero(wc);
    if (live) {
        const fe f = fe_from_table(load_fe256(fl + u));
        const fe rq = fe_mul<F>(wide18_reduce<F>(aq), f), rc = fe_mul<F>(wide18_reduce<F>(ac), f);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            wq.l[i] = rq.l[i];
            wc.l[i] = rc.l[i];
        }
        if constexpr (S11) {
            const fe r11 = fe_mul<F>(wide18_reduce<F>(a11), f);
#pragma unroll
            for (int i = 0; i < 9; ++i) wx.l[i] = r11.l[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const unsigned long long a = wave_sum63(wq.l[i]), b = wave_sum63(wx.l[i]), c = wave_sum63(wc.l[i]);
        if ((threadIdx.x & 63) == 63) {
            atomicAdd(&acc[i], a);
            atomicAdd(&acc[9 + i], b);
            atomicAdd(&acc[18 + i], c);
        }
    }
    __syncthreads();
    r1_emit(accs, acc, blockIdx.y * gridDim.x + blockIdx.x);
}

// Sums of a round from T alone: thread = column u, blockIdx.y = a chunk of the hn pair rows (h, h + hn).
template <int F>
__global__ void __launch_bounds__(256) k_sc_r1_coeffs(const fe256 *__restrict__ T, u32 lo_bits, u32 hn, u32 rows_per_chunk,
                                                     const fe_limbs *__restrict__ f0, const fe_limbs *__restrict__ f1, const fe_limbs *__restrict__ fd,
                                                     const fe256 *__restrict__ fl, unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long acc[R1_SLOTS];
    if (threadIdx.x < R1_SLOTS) acc[threadIdx.x] = 0;
    __syncthreads();
    const u32 cols = 1u << lo_bits, u = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = u < cols;
    fe_wide18 aq, a11, ac;
    wide18_zero(aq);
    wide18_zero(a11);
    wide18_zero(ac);
    if (live) {
        // Rows are dealt out to the gridDim.y row groups round-robin (h = blockIdx.y, + gridDim.y, ...): at any moment the whole
        // grid reads one window of gridDim.y consecutive rows in each half, as a linear stream would, instead of gridDim.y
        // streams 2^lo entries apart.  The next row's entries and factors are requested before this row's products.
        const u32 step = gridDim.y;
        const fe256 *lo = T + u, *hi = T + ((u64)hn << lo_bits) + u;
        (void)rows_per_chunk;
        u32 h = blockIdx.y;
        fe256 n0 = {}, n1 = {};
        fe_limbs g0 = {}, g1 = {}, gd = {};
        if (h < hn) {
            n0 = load_fe256(lo + ((u64)h << lo_bits));
            n1 = load_fe256(hi + ((u64)h << lo_bits));
            g0 = f0[h]; g1 = f1[h]; gd = fd[h];
        }
        u32 since = 0;
        for (; h < hn; h += step) {
            const fe256 c0 = n0, c1 = n1;
            const fe_limbs k0 = g0, k1 = g1, kd = gd;
            if (h + step < hn) {
                n0 = load_fe256(lo + ((u64)(h + step) << lo_bits));
                n1 = load_fe256(hi + ((u64)(h + step) << lo_bits));
                g0 = f0[h + step]; g1 = f1[h + step]; gd = fd[h + step];
            }
            const fe t0 = fe_from_table(c0), t1 = fe_from_table(c1);
            const fe ts = fe_sub<F, 2>(t1, t0);
            wide18_mac(aq, ts.l, kd.l);
            wide18_mac(a11, t1.l, k1.l);
            wide18_mac(ac, t0.l, k0.l);
            if (++since == 4) {
                wide18_carry(aq);
                wide18_carry(a11);
                wide18_carry(ac);
                since = 0;
            }
        }
    }
    r1_block_sums<F>(aq, a11, ac, live, fl, u, acc, partial);
}

// Fold with r (rows h, h + 2*hn of the 4*hn rows of Tsrc) and, in the same pass, the sums of the next round over the folded
// table (pair rows h, h + hn of its 2*hn rows): thread = column u, blockIdx.y = a chunk of h < hn.  In place when Tsrc == T:
// a thread reads and writes its own entries only.
// S11 = false: sum t1 e1 is not accumulated -- the previous round's polynomial at r is what this round's g(0) + g(1) must be
// (the sum-check identity), so k_sc_r1_final takes it as claim - con: two products per pair instead of three.
// `list` (nlist entries, or nullptr: all h < hn): the rows this launch takes -- a structured pristine table hands the rows whose
// sources are all small or constant to k_sc_r1_fold_coeffs_cs and the rest to this kernel.
template <int F, bool S11>
__global__ void __launch_bounds__(256) k_sc_r1_fold_coeffs(const fe256 *Tsrc, fe256 *T, u32 lo_bits, u32 hn, const u32 *__restrict__ list, u32 nlist, fe256 r_int,
                                                          const fe_limbs *__restrict__ f0, const fe_limbs *__restrict__ f1,
                                                          const fe_limbs *__restrict__ fd, const fe256 *__restrict__ fl, unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long acc[R1_SLOTS];
    if (threadIdx.x < R1_SLOTS) acc[threadIdx.x] = 0;
    __syncthreads();
    const u32 cols = 1u << lo_bits, u = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = u < cols;
    const fe r = fe_from_integer<F>(r_int);
    fe_wide18 aq, a11, ac;
    wide18_zero(aq);
    wide18_zero(a11);
    wide18_zero(ac);
    if (live) {
        const u64 half = (u64)(2 * hn) << lo_bits;            // entries per half of Tsrc
        // rows round-robin over the row groups, next row's entries and factors requested first (see k_sc_r1_coeffs)
        const u32 step = gridDim.y;
        const u32 cnt = list ? nlist : hn;
        u32 k = blockIdx.y;
        u32 h = 0;
        fe256 na0 = {}, na1 = {}, nc0 = {}, nc1 = {};
        fe_limbs g0 = {}, g1 = {}, gd = {};
        if (k < cnt) {
            h = list ? list[k] : k;
            const u64 b0 = ((u64)h << lo_bits) + u, b1 = ((u64)(h + hn) << lo_bits) + u;
            na0 = load_fe256(Tsrc + b0); na1 = load_fe256(Tsrc + b0 + half);
            nc0 = load_fe256(Tsrc + b1); nc1 = load_fe256(Tsrc + b1 + half);
            g0 = f0[h]; g1 = f1[h]; gd = fd[h];
        }
        u32 since = 0;
        for (; k < cnt; k += step) {
            const u64 b0 = ((u64)h << lo_bits) + u, b1 = ((u64)(h + hn) << lo_bits) + u;
            const fe256 pa0 = na0, pa1 = na1, pc0 = nc0, pc1 = nc1;
            const fe_limbs k0 = g0, k1 = g1, kd = gd;
            if (k + step < cnt) {
                h = list ? list[k + step] : k + step;
                const u64 x0 = ((u64)h << lo_bits) + u, x1 = ((u64)(h + hn) << lo_bits) + u;
                na0 = load_fe256(Tsrc + x0); na1 = load_fe256(Tsrc + x0 + half);
                nc0 = load_fe256(Tsrc + x1); nc1 = load_fe256(Tsrc + x1 + half);
                g0 = f0[h]; gd = fd[h];
                if constexpr (S11) g1 = f1[h];
            }
            const fe a0 = fe_from_table(pa0), a1 = fe_from_table(pa1);
            const fe c0 = fe_from_table(pc0), c1 = fe_from_table(pc1);
            const fe t0 = fe_canon<F>(fe_add<F>(a0, fe_mul<F>(r, fe_sub<F, 2>(a1, a0))));
            const fe t1 = fe_canon<F>(fe_add<F>(c0, fe_mul<F>(r, fe_sub<F, 2>(c1, c0))));
            store_fe256(T + b0, fe_pack(t0));
            store_fe256(T + b1, fe_pack(t1));
            const fe ts = fe_sub<F, 2>(t1, t0);
            wide18_mac(aq, ts.l, kd.l);
            if constexpr (S11) wide18_mac(a11, t1.l, k1.l);
            wide18_mac(ac, t0.l, k0.l);
            if (++since == 4) {
                wide18_carry(aq);
                if constexpr (S11) wide18_carry(a11);
                wide18_carry(ac);
                since = 0;
            }
        }
    }
    r1_block_sums<F, S11>(aq, a11, ac, live, fl, u, acc, partial);
}

// The fold alone (T only; EQ's share is k_sc_r1_prep): entries b < pow.
template <int F>
__global__ void __launch_bounds__(256) k_sc_r1_fold(const fe256 *Tsrc, fe256 *T, u32 pow, fe256 r_int) {
    const fe r = fe_from_integer<F>(r_int);
    for (u32 b = blockIdx.x * blockDim.x + threadIdx.x; b < pow; b += gridDim.x * blockDim.x) {
        const fe t0 = fe_from_table(load_fe256(Tsrc + b)), t1 = fe_from_table(load_fe256(Tsrc + b + pow));
        store_fe256(T + b, fe_to_table<F>(fe_add<F>(t0, fe_mul<F>(r, fe_sub<F, 2>(t1, t0)))));
    }
}

// Block sums -> (xsq, x, con) with the masses' share: a mass w at b (an e0) adds w t0 to con and takes w (t1 - t0) from xsq;
// at b + pow (an e1) it adds w t1 to sum t1 e1 and w (t1 - t0) to xsq.  One thread per mass, limb sums through LDS.
// `ident`: out3 still holds the previous round's (xsq, x, con) and r_int is the challenge it was folded with; sum t1 e1 is then
// g_prev(r) - con and the partial sums carry no t1 e1 column.
template <int F>
__global__ void __launch_bounds__(1024) k_sc_r1_final(unsigned long long *__restrict__ partial, const fe256 *__restrict__ T, u32 pow,
                                                     const u32 *__restrict__ mq, const fe256 *__restrict__ mw, u32 nq, int ident, fe256 r_int,
                                                     fe256 *out3, fe256 *__restrict__ host3, u32 seq) {
    __shared__ unsigned long long tot[36];                    // xsq, sum t1 e1, con, and what the masses take from xsq
    __shared__ u32 back[4][9], outc[3][9];
    if (threadIdx.x < 36) tot[threadIdx.x] = 0;
    __syncthreads();
    // r and the previous round's three coefficients into the field (the sum-check identity needs them), one lane each, by the last
    // lanes of the workgroup -- which have no share in the blocks' sums -- while the others read them: the loads and the products are off the tail
    if (ident && threadIdx.x >= 1020) {
        const u32 j = threadIdx.x - 1020;
        const fe a = fe_from_integer<F>(j == 0 ? r_int : load_fe256(out3 + (j - 1)));
#pragma unroll
        for (int i = 0; i < 9; ++i) back[j][i] = a.l[i];
    }
    if (threadIdx.x < R1_GROUPS * R1_SLOTS) {                 // the accumulator sets of the round's kernels: read, and left at zero for the next round
        const unsigned long long s = partial[threadIdx.x];
        partial[threadIdx.x] = 0;
        if (s) atomicAdd(&tot[threadIdx.x % R1_SLOTS], s);
    }
    for (u32 k = threadIdx.x; k < nq; k += blockDim.x) {
        const u32 q = mq[k];
        const bool upper = q >= pow;
        const u32 b = upper ? q - pow : q;
        const fe w = fe_from_table(load_fe256(mw + k));
        const fe t0 = fe_from_table(load_fe256(T + b)), t1 = fe_from_table(load_fe256(T + b + pow));
        const fe d = fe_mul<F>(w, fe_sub<F, 2>(t1, t0));      // < 2, limbs normalised
        const fe s = fe_mul<F>(w, upper ? t1 : t0);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            atomicAdd(&tot[(upper ? 0 : 27) + i], (unsigned long long)d.l[i]);
            atomicAdd(&tot[(upper ? 9 : 18) + i], (unsigned long long)s.l[i]);
        }
    }
    __syncthreads();
    __shared__ u32 conv[4][9];
    if ((threadIdx.x & 63) == 0 && threadIdx.x < 256) {       // the four limb groups are folded back by four waves at once
        const u32 k = threadIdx.x >> 6;
        fe_wide w;
#pragma unroll
        for (int i = 0; i < 9; ++i) w.l[i] = tot[9 * k + i];
        const fe x = fe_from_limb_sums<F>(w);   // < 2
#pragma unroll
        for (int i = 0; i < 9; ++i) conv[k][i] = x.l[i];
    }
    __syncthreads();
    // The tail: lane 0 evaluates the claim, then lanes 0..2 of the first wave turn one coefficient each into an integer and post it
    // -- three products deep where one thread went through nine (3 us of every structured round).
    if (threadIdx.x == 0) {
        fe v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int i = 0; i < 9; ++i) v[k].l[i] = conv[k][i];
            REEF_SET_BOUND(v[k], 2.0);
        }
        const fe xsq = fe_canon<F>(fe_sub<F, 2>(v[0], v[3]));
        if (ident) {                                          // sum t1 e1 = (xsq' r + x') r + con' - con
            fe r, pq, px, pc;
#pragma unroll
            for (int i = 0; i < 9; ++i) { r.l[i] = back[0][i]; pq.l[i] = back[1][i]; px.l[i] = back[2][i]; pc.l[i] = back[3][i]; }
            REEF_SET_BOUND(r, 2.0); REEF_SET_BOUND(pq, 2.0); REEF_SET_BOUND(px, 2.0); REEF_SET_BOUND(pc, 2.0);
            const fe claim = fe_add<F>(fe_mul<F>(fe_add<F>(fe_mul<F>(pq, r), px), r), pc);   // < 3
            v[1] = fe_canon<F>(fe_sub<F, 2>(claim, v[2]));
        }
        const fe x = fe_canon<F>(fe_sub<F, 2>(fe_sub<F, 2>(v[1], v[2]), xsq));
        const fe con = fe_canon<F>(v[2]);
#pragma unroll
        for (int i = 0; i < 9; ++i) { outc[0][i] = xsq.l[i]; outc[1][i] = x.l[i]; outc[2][i] = con.l[i]; }
    }
    __syncthreads();
    if (threadIdx.x < 64) {                                   // one wave: the s_waitcnt of the signal covers the stores of lanes 0..2
        if (threadIdx.x < 3) {
            fe c;
#pragma unroll
            for (int i = 0; i < 9; ++i) c.l[i] = outc[threadIdx.x][i];
            REEF_SET_BOUND(c, 1.0);
            const fe256 o = fe_to_integer<F>(c);
            store_fe256(out3 + threadIdx.x, o);               // kept on the device: the next fused round's identity reads them
            sc_post_fe256(host3 + threadIdx.x, o);            // and posted to the host, which polls the sequence number
        }
        if (threadIdx.x == 0) sc_signal_host(host3, seq);
    }
}

// The masses onto a written-out EQ table (weights in table form).  Indices may repeat: the first mass of an index adds the
// weights of all of them, the others do nothing -- a thread per mass, no order to keep (one thread in a loop took 50 us for 64).
template <int F>
__global__ void __launch_bounds__(256) k_sc_r1_masses(const u32 *__restrict__ mq, const fe256 *__restrict__ mw, u32 nq, fe256 *__restrict__ eq) {
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nq) return;
    const u32 q = mq[k];
    for (u32 j = 0; j < k; ++j)
        if (mq[j] == q) return;
    fe sum = fe_from_table(load_fe256(eq + q));
    for (u32 j = k; j < nq; ++j)
        if (mq[j] == q) sum = fe_canon<F>(fe_add<F>(sum, fe_from_table(load_fe256(mw + j))));
    store_fe256(eq + q, fe_pack(sum));
}
// rs[k] (integers) -> mass weights in table form, the lookup positions into the array the folds move along, and the sum of FL --
// which is ONE whatever the point: FL[u] = prod_j (bit_j(u) ? q_j : 1 - q_j) sums to prod_j (q_j + 1 - q_j) over the cube (rounds
// 3-4 added it up with a kernel of its own)
template <int F>
__global__ void __launch_bounds__(256) k_sc_r1_mass_init(const fe256 *__restrict__ rs_int, const u32 *__restrict__ qs, u32 nq, fe256 *__restrict__ mw,
                                                        u32 *__restrict__ mq, fe256 *__restrict__ sum_fl) {
    const u32 k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nq) {
        store_fe256(mw + k, fe_to_table<F>(fe_from_integer<F>(load_fe256(rs_int + k))));
        mq[k] = qs[k];
    }
    if (k == 0) store_fe256(sum_fl, fe_to_table<F>(fe_one<F>()));
}

// ---- a pristine table with structure: constant rows and rows of small entries ----------------------------------------------
// Reef's lookup tables are mostly not field elements: the document half of the hybrid table holds symbols (< |alphabet| + 3,
// framework.rs:978-1011) and zeros, its public half is the transition table followed by ONE value repeated up to the half
// (r1cs.rs:481-484: `calc_fill`), a plain document table is symbols throughout.  With T as a matrix of 2^lo columns a row is
//   K  constant (every entry equals the first),   S  small (every entry < 2^30),   W  anything else,
// found once when the table is set (k_sc_classify; S rows also get a 4-byte copy).  The first round of every folding step reads
// the pristine table, so its sums and its fold use that: a K row contributes in closed form, an S entry is a 4-byte read and a
// 9-multiply-add product, only W rows are read as 32-byte field elements.  After the first fold the table is dense.
static constexpr u32 SC_SMALL_BITS = 30;

// flags[row] (preset to 3): bit 0 survives while every entry of the row is < 2^30, bit 1 while every entry equals the first.
static __global__ void __launch_bounds__(256) k_sc_classify(const fe256 *__restrict__ in_int, u32 n, u32 len, u32 lo_bits, u32 *__restrict__ flags,
                                                    u32 *__restrict__ s32) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= len) return;
    const u32 first = (i >> lo_bits) << lo_bits;
    fe256 v = {}, f = {};
    if (i < n) v = load_fe256(in_int + i);
    if (first < n) f = load_fe256(in_int + first);
    bool small = v.w[0] < (1u << SC_SMALL_BITS), same = v.w[0] == f.w[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) {
        small = small && v.w[k] == 0;
        same = same && v.w[k] == f.w[k];
    }
    s32[i] = v.w[0];
    const u32 bad = (small ? 0u : 1u) | (same ? 0u : 2u);
    if (lo_bits >= 6) {                                  // a wave's 64 entries lie in one row: one atomic per wave, not per entry (a row of 2^13 entries
        const u32 wbad = (__any(bad & 1u) ? 1u : 0u) | (__any(bad & 2u) ? 2u : 0u);   // that are not all equal used to send 2^13 atomics to one word: 43 ms for
        if (wbad && (threadIdx.x & 63u) == 0) atomicAnd(&flags[i >> lo_bits], ~wbad);  // a 2^26-entry table, profiles/r05_cfg4_prove_hbm.txt before the change)
    } else if (bad) {
        atomicAnd(&flags[i >> lo_bits], ~bad);
    }
}

// value = sum w[i] 2^(29 i) < 2^31 M (a constant below M plus two products of an entry < 2^30 and a reduced element): the
// canonical residue.  q = floor(value / 2^254) >= floor(value / M); value - q M = (value mod 2^254) - q (M - 2^254) > -2^158.
template <int F> __device__ __forceinline__ fe fe_reduce_small(const u64 (&w)[9]) {
    u32 t[9];
    u64 c = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const u64 v = w[i] + c;
        t[i] = (u32)v & LIMB_MASK;
        c = v >> LIMB_BITS;
    }
    const u32 q = (t[8] >> 22) | ((u32)c << 7);               // c < 2^25: value < 2^286
    fe r;
    i64 b = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const i64 v = (i64)t[i] - (i64)((u64)q * FC<F>::MOD[i]) + b;
        r.l[i] = (u32)v & LIMB_MASK;
        b = v >> LIMB_BITS;   // arithmetic
    }
    const i64 top = (i64)(t[8] & 0x3FFFFFu) + b;              // q 2^254 against q MOD[8] 2^232: gone
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

// ---- the table set from parts (reef_sc_set_table_parts) ---------------------------------------------------------------------
// What the caller knows about the table, by value: up to SC_MAX_PARTS runs laid end to end from entry 0.  start[p] .. start[p + 1]
// are the entries of part p (an empty part matches nothing; the starts past the last part repeat the total, beyond it T is zero).
// ptr[p]: device memory -- canonical integers (FE), unsigned little-endian symbols of `elem_bytes` (SYMBOLS), or for a FILL TWO
// fe256: the value as an integer and in the resident table form (the host converts the one value).
static constexpr u32 SC_MAX_PARTS = 8;
static constexpr u32 SC_PART_FE = 0, SC_PART_SYMBOLS = 1, SC_PART_FILL = 2, SC_PART_NONE = 3;
struct ScPartsArg {
    const unsigned char *ptr[SC_MAX_PARTS];
    u32 start[SC_MAX_PARTS + 1];
    u32 kind_eb[SC_MAX_PARTS];           // kind | elem_bytes << 8
};
struct ScPartRef { const unsigned char *ptr; u32 kind, eb, off, end; };
// the part entry i lies in (constant indices only: the descriptors stay in scalar registers, nothing goes to scratch)
static __device__ __forceinline__ ScPartRef sc_part_of(const ScPartsArg &a, u32 i) {
    ScPartRef r = {nullptr, SC_PART_NONE, 0u, 0u, 0u};
#pragma unroll
    for (u32 p = 0; p < SC_MAX_PARTS; ++p)
        if (i >= a.start[p] && i < a.start[p + 1]) {
            r.ptr = a.ptr[p];
            r.kind = a.kind_eb[p] & 0xffu;
            r.eb = a.kind_eb[p] >> 8;
            r.off = i - a.start[p];
            r.end = a.start[p + 1];
        }
    return r;
}
// entry i of the table as the canonical integer the caller would have written out; never reads outside the part
static __device__ __forceinline__ fe256 sc_part_value(const ScPartRef &r) {
    fe256 v = {};
    if (r.kind == SC_PART_FE) v = load_fe256(reinterpret_cast<const fe256 *>(r.ptr) + r.off);
    else if (r.kind == SC_PART_FILL) v = load_fe256(reinterpret_cast<const fe256 *>(r.ptr));
    else if (r.kind == SC_PART_SYMBOLS)
        v.w[0] = r.eb == 1 ? (u32)r.ptr[r.off] : r.eb == 2 ? (u32)reinterpret_cast<const unsigned short *>(r.ptr)[r.off] : reinterpret_cast<const u32 *>(r.ptr)[r.off];
    return v;
}
// the resident table form of v < 2^32: v * ONE (ONE = R' mod M, canonical limbs) is below 2^32 M < 2^286, fe_reduce_small's
// range, and the canonical residue is unique -- the words fe_to_table(fe_from_caller(v, 0)) gives, for 9 multiplies
template <int F> static __device__ __forceinline__ fe256 sc_table_form_u32(u32 v) {
    u64 w[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) w[i] = (u64)v * FC<F>::ONE[i];
    return fe_pack(fe_reduce_small<F>(w));
}
static __device__ __forceinline__ u32 sc_swap_pair(u32 v) {          // the value of lane ^ 1: quad_perm:[1,0,3,2]
    return (u32)__builtin_amdgcn_update_dpp(0, (int)v, 0xb1, 0xf, 0xf, false);
}

// T0 <- the parts (resident form), s32 <- their low words, flags cleared as k_sc_classify clears them: ONE pass over the len entries
// in place of k_fe_import, the zero fill of the tail and k_sc_classify.  flags == nullptr: the table is too small for the row
// structure, T0 alone is written.  The kernel stores 36 bytes per entry and reads 1 to 4 for a symbol, so the stores decide:
// a wave takes `sub` consecutive tiles of 128 entries; in a tile lane 2k computes entries k and 64 + k, lane 2k + 1 entries 32 + k
// and 96 + k, the two lanes of a pair swap halves (8 DPP moves per lane), and each of the four store instructions of the tile
// writes 1 KiB without a gap: lane l the 16 bytes at l * 16.  Symbols of 1 or 2 bytes are read a dword per lane where the tile
// lies in one part and its first symbol is 4-byte aligned (then handed to the lane that needs them through ds_bpermute), 4-byte
// symbols a dword per entry; tiles that straddle parts, and unaligned ones, take the part lookup entry by entry.
template <int F>
static __global__ void __launch_bounds__(256) k_sc_set_parts(const ScPartsArg a, u32 len, u32 lo_bits, u32 sub, fe256 *__restrict__ T0, u32 *__restrict__ flags,
                                                             u32 *__restrict__ s32) {
    const u32 lane = threadIdx.x & 63u, k = lane >> 1, odd = lane & 1u;
    const u32 wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    for (u32 s = 0; s < sub; ++s) {
        const u64 t64 = ((u64)wave * sub + s) << 7;
        if (t64 >= len) break;                              // the same for every lane of the wave
        const u32 t0 = (u32)t64;
        u32 e[2] = {t0 + k + 32u * odd, t0 + 64u + k + 32u * odd};
        fe256 v[2] = {};
        u32 kind[2];
        const unsigned char *src[2];
        const ScPartRef r0 = sc_part_of(a, t0);
        const bool wide = r0.kind == SC_PART_SYMBOLS && r0.eb < 4u && (u64)t0 + 128u <= r0.end && t0 + 128u <= len &&
                          ((reinterpret_cast<size_t>(r0.ptr) + (size_t)r0.off * r0.eb) & 3u) == 0;
        if (wide) {                                          // 128 or 256 bytes of symbols, all inside the part: a dword per lane
            const u32 *dw = reinterpret_cast<const u32 *>(r0.ptr + (size_t)r0.off * r0.eb);
            const u32 d = lane < 32u * r0.eb ? dw[lane] : 0u;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const u32 byte = (e[j] - t0) * r0.eb;
                const u32 got = (u32)__shfl((int)d, (int)(byte >> 2)) >> ((byte & 3u) * 8u);
                v[j].w[0] = r0.eb == 1 ? got & 0xffu : got & 0xffffu;
                kind[j] = SC_PART_SYMBOLS;
                src[j] = nullptr;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                ScPartRef r = sc_part_of(a, e[j]);
                if (e[j] >= len) r.kind = SC_PART_NONE;          // only a table shorter than a tile
                v[j] = sc_part_value(r);
                kind[j] = r.kind;
                src[j] = r.ptr;
            }
        }
        if (flags) {
            u32 bad[2];
            fe256 f = {};
            u32 first_at = 0xffffffffu;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const u32 first = (e[j] >> lo_bits) << lo_bits;
                if (first != first_at) {                      // a row may straddle parts: its first entry through the same lookup
                    f = sc_part_value(sc_part_of(a, first));
                    first_at = first;
                }
                bool small = v[j].w[0] < (1u << SC_SMALL_BITS), same = v[j].w[0] == f.w[0];
#pragma unroll
                for (int w = 1; w < 8; ++w) {
                    small = small && v[j].w[w] == 0;
                    same = same && v[j].w[w] == f.w[w];
                }
                bad[j] = (small ? 0u : 1u) | (same ? 0u : 2u);
                if (e[j] < len) s32[e[j]] = v[j].w[0];
            }
            if (lo_bits >= 6) {                               // the 64 entries of slot j lie in one row: one atomic for them
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const u32 wbad = (__any(bad[j] & 1u) ? 1u : 0u) | (__any(bad[j] & 2u) ? 2u : 0u);
                    if (wbad && lane == 0) atomicAnd(&flags[e[j] >> lo_bits], ~wbad);
                }
            } else {
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    if (bad[j] && e[j] < len) atomicAnd(&flags[e[j] >> lo_bits], ~bad[j]);
            }
        }
        fe256 out[2];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (kind[j] == SC_PART_FE) out[j] = fe_to_table<F>(fe_from_caller<F>(v[j], 0));
            else if (kind[j] == SC_PART_FILL) out[j] = load_fe256(reinterpret_cast<const fe256 *>(src[j]) + 1);
            else out[j] = sc_table_form_u32<F>(v[j].w[0]);      // a symbol, or zero past the parts
        }
        // every lane is here again: the even lane keeps the low halves of its two entries and takes the low halves of its
        // neighbour's, the odd lane the high halves
        u32x4 *q = reinterpret_cast<u32x4 *>(T0 + t0);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            u32 fst[4], snd[4];                             // what this lane writes of entries k and 32 + k of the slot
            const u32 pick = 0u - odd;                      // bit selects, not `odd ? .. : ..`: the compiler turns that into an indexed
#pragma unroll                                              // read from scratch
            for (int w = 0; w < 4; ++w) {
                const u32 l = out[j].w[w], h = out[j].w[4 + w];
                const u32 mine = (h & pick) | (l & ~pick), theirs = sc_swap_pair((l & pick) | (h & ~pick));
                fst[w] = (theirs & pick) | (mine & ~pick);
                snd[w] = (mine & pick) | (theirs & ~pick);
            }
            const u32 ea = t0 + 64u * j + k, eb = ea + 32u;   // the entries the two stores write a half of
            if (ea < len) q[128u * j + lane] = mk_u32x4(fst[0], fst[1], fst[2], fst[3]);
            if (eb < len) q[128u * j + 64u + lane] = mk_u32x4(snd[0], snd[1], snd[2], snd[3]);
        }
    }
}

// Round-one sums of the rows of ONE side and ONE class (WIDE: W rows, 32-byte entries; else S rows, 4-byte entries): with
// t = T0[h + row_off, u],  A[u] = sum fa[h] t,  B[u] = sum fd[h] t  over the listed h (fa = f0 on side 0, f1 on side 1; row_off = side * hn).
// Side 0 leaves (sum FL A, sum FL B) as (con, what is taken from xsq), side 1 as (sum t1 e1, what adds to xsq).
template <int F, bool WIDE>
__global__ void __launch_bounds__(256) k_sc_r1s_rows(const fe256 *__restrict__ T0, const u32 *__restrict__ s32, u32 lo_bits, u32 row_off, u32 side,
                                                    const u32 *__restrict__ list, u32 nlist, const fe_limbs *__restrict__ fa,
                                                    const fe_limbs *__restrict__ fd, const fe256 *__restrict__ fl, unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long acc[R1_SLOTS];
    if (threadIdx.x < R1_SLOTS) acc[threadIdx.x] = 0;
    __syncthreads();
    const u32 cols = 1u << lo_bits, u = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = u < cols;
    fe ra = fe_zero(), rb = fe_zero();
    if (live) {
        const u32 step = gridDim.y;
        const u64 off = ((u64)row_off << lo_bits) + u;        // round one: side * hn; the deferred fold's sums: b * hq, side = b & 1
        if constexpr (WIDE) {
            fe_wide18 wa, wb;
            wide18_zero(wa);
            wide18_zero(wb);
            u32 since = 0;
            for (u32 k = blockIdx.y; k < nlist; k += step) {
                const u32 h = list[k];
                const fe t = fe_from_table(load_fe256(T0 + ((u64)h << lo_bits) + off));
                wide18_mac(wa, t.l, fa[h].l);
                wide18_mac(wb, t.l, fd[h].l);
                if (++since == 4) {
                    wide18_carry(wa);
                    wide18_carry(wb);
                    since = 0;
                }
            }
            ra = wide18_reduce<F>(wa);
            rb = wide18_reduce<F>(wb);
        } else {
            fe_wide wa, wb;
            wide_zero(wa);
            wide_zero(wb);
            u32 since = 0;
            // four rows per trip: their row numbers, factors and entries are requested together (a row alone waits for three
            // dependent scalar loads: 72 us for the 3840 document rows of a 2^26-entry hybrid table, most of it latency)
            u32 k = blockIdx.y;
            for (; k + 3 * step < nlist; k += 4 * step) {
                const u32 h0 = list[k], h1 = list[k + step], h2 = list[k + 2 * step], h3 = list[k + 3 * step];
                const u32 t0 = s32[((u64)h0 << lo_bits) + off], t1 = s32[((u64)h1 << lo_bits) + off];
                const u32 t2 = s32[((u64)h2 << lo_bits) + off], t3 = s32[((u64)h3 << lo_bits) + off];
                const fe_limbs a0 = fa[h0], d0 = fd[h0], a1 = fa[h1], d1 = fd[h1], a2 = fa[h2], d2 = fd[h2], a3 = fa[h3], d3 = fd[h3];
#pragma unroll
                for (int i = 0; i < 9; ++i) {
                    wa.l[i] += (u64)t0 * a0.l[i] + (u64)t1 * a1.l[i] + (u64)t2 * a2.l[i] + (u64)t3 * a3.l[i];   // 4 x 2^59
                    wb.l[i] += (u64)t0 * d0.l[i] + (u64)t1 * d1.l[i] + (u64)t2 * d2.l[i] + (u64)t3 * d3.l[i];
                }
                if (++since == 2) {                            // 8 products of < 2^59 per limb, then carry
                    wide_carry(wa);
                    wide_carry(wb);
                    since = 0;
                }
            }
            wide_carry(wa);
            wide_carry(wb);
            for (; k < nlist; k += step) {                     // at most three rows
                const u32 h = list[k];
                const u32 t = s32[((u64)h << lo_bits) + off];
                const fe_limbs a = fa[h], d = fd[h];
#pragma unroll
                for (int i = 0; i < 9; ++i) {
                    wa.l[i] += (u64)t * a.l[i];
                    wb.l[i] += (u64)t * d.l[i];
                }
            }
            ra = fe_from_wide<F>(wa);
            rb = fe_from_wide<F>(wb);
        }
        const fe f = fe_from_table(load_fe256(fl + u));
        ra = fe_mul<F>(ra, f);
        rb = fe_mul<F>(rb, f);
    }
    const u32 sa = side ? 9u : 18u, sb = side ? 0u : 27u;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        unsigned long long a = live ? ra.l[i] : 0ull, b = live ? rb.l[i] : 0ull;
        for (int d = 32; d > 0; d >>= 1) {
            a += __shfl_down(a, d, WAVE);
            b += __shfl_down(b, d, WAVE);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&acc[sa + i], a);
            atomicAdd(&acc[sb + i], b);
        }
    }
    __syncthreads();
    r1_emit(partial, acc, blockIdx.y * gridDim.x + blockIdx.x);
}

// The constant rows of one side (a thread per row, a few blocks): c_h = T0[(h + row_off) 2^lo]; (sum FL) * sum fa[h] c_h and the same with fd.
// Up to four such row sets in ONE launch (blockIdx.y picks the set): the kernel is a latency chain of ~10 us whatever the number
// of rows, and the deferred fold has one set per source block.
struct ScConstSets {
    u32 row_off[4], side[4], nlist[4];
    const u32 *list[4];
    const fe_limbs *fa[4], *fd[4];
};
template <int F>
__global__ void __launch_bounds__(256) k_sc_r1s_const(const fe256 *__restrict__ T0, u32 lo_bits, ScConstSets sets, const fe256 *__restrict__ sum_fl,
                                                     unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long acc[R1_SLOTS];
    if (threadIdx.x < R1_SLOTS) acc[threadIdx.x] = 0;
    __syncthreads();
    const u32 row_off = sets.row_off[blockIdx.y], side = sets.side[blockIdx.y], nlist = sets.nlist[blockIdx.y];
    const u32 *__restrict__ list = sets.list[blockIdx.y];
    const fe_limbs *__restrict__ fa = sets.fa[blockIdx.y], *__restrict__ fd = sets.fd[blockIdx.y];
    fe_wide wa, wb;
    wide_zero(wa);
    wide_zero(wb);
    for (u32 k = blockIdx.x * blockDim.x + threadIdx.x; k < nlist; k += gridDim.x * blockDim.x) {
        const u32 h = list[k];
        const fe c = fe_from_table(load_fe256(T0 + ((u64)(h + row_off) << lo_bits)));
        const fe a = fe_mul<F>(c, fe_from_limbs(fa[h], 1.0)), b = fe_mul<F>(c, fe_from_limbs(fd[h], 1.0));
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            wa.l[i] += a.l[i];
            wb.l[i] += b.l[i];
        }
    }
    const u32 sa = side ? 9u : 18u, sb = side ? 0u : 27u;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        unsigned long long a = wa.l[i], b = wb.l[i];
        for (int d = 32; d > 0; d >>= 1) {
            a += __shfl_down(a, d, WAVE);
            b += __shfl_down(b, d, WAVE);
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(&acc[sa + i], a);
            atomicAdd(&acc[sb + i], b);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {                                   // times sum FL, back to limb sums
        const fe sf = fe_from_table(load_fe256(sum_fl));
        fe_wide ta, tb;
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            ta.l[i] = acc[sa + i];
            tb.l[i] = acc[sb + i];
        }
        const fe pa = fe_mul<F>(fe_from_wide<F>(ta), sf), pb = fe_mul<F>(fe_from_wide<F>(tb), sf);
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            acc[sa + i] = pa.l[i];
            acc[sb + i] = pb.l[i];
        }
    }
    __syncthreads();
    r1_emit(partial, acc, blockIdx.y * gridDim.x + blockIdx.x);
}

// First fold of a step, rows whose four sources are all K or S: per h < hn the constant parts
//   KA[h] = [K] c(h) (1 - r) + [K] c(h + 2hn) r,    KC[h] = [K] c(h + hn) (1 - r) + [K] c(h + 3hn) r     ([K]: that row is constant)
// and the mask of the sources that are S rows (bit 0: h, 1: h + 2hn, 2: h + hn, 3: h + 3hn); flags as k_sc_classify left them.
template <int F>
__global__ void __launch_bounds__(256) k_sc_r1_kprep(const fe256 *__restrict__ T0, const u32 *__restrict__ flags, u32 lo_bits, u32 hn, fe256 r_int,
                                                    fe_limbs *__restrict__ ka, fe_limbs *__restrict__ kc, u32 *__restrict__ smask) {
    const u32 h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= hn) return;
    const fe r = fe_from_integer<F>(r_int);
    const fe omr = fe_sub<F, 2>(fe_one<F>(), r);
    const u32 rows[4] = {h, h + 2 * hn, h + hn, h + 3 * hn};
    fe part[4];
    u32 mask = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const u32 fl = flags[rows[k]];
        part[k] = fe_zero();
        if (fl & 2u) part[k] = fe_mul<F>(fe_from_table(load_fe256(T0 + ((u64)rows[k] << lo_bits))), (k & 1) ? r : omr);
        else if (fl & 1u) mask |= 1u << k;
    }
    ka[h] = fe_to_limbs(fe_canon<F>(fe_add<F>(part[0], part[1])));
    kc[h] = fe_to_limbs(fe_canon<F>(fe_add<F>(part[2], part[3])));
    bool fast = true;                                         // bit 7: all four sources are K or S (the quadruple is on the fast list)
#pragma unroll
    for (int k = 0; k < 4; ++k) fast = fast && (flags[rows[k]] & 3u) != 0;
    smask[h] = mask | (fast ? 0x80u : 0u);
}

// k_sc_r1_fold_coeffs for the listed rows, all of whose sources are constant or small: t' = K + s0 (1 - r) + s1 r with 4-byte
// reads and 9-multiply-add products (fe_reduce_small), written out as a dense table; the next round's sums as in the dense kernel.
// WRITE = false (round 4): the sums only -- the folded rows are NOT written.  A row pair whose next fold also has nothing but
// constant and small sources is materialised one round later, straight from the 4-byte sources (k_sc_r2_fold_coeffs_cs): the
// dense table is first written at a quarter of the pristine size instead of half, and never read at half size.
template <int F, bool S11, bool WRITE = true>
__global__ void __launch_bounds__(256) k_sc_r1_fold_coeffs_cs(const u32 *__restrict__ s32, fe256 *__restrict__ T, u32 lo_bits, u32 hn, const u32 *__restrict__ list,
                                                             u32 nlist, fe256 r_int, const fe_limbs *__restrict__ ka, const fe_limbs *__restrict__ kc,
                                                             const u32 *__restrict__ smask, const fe_limbs *__restrict__ f0, const fe_limbs *__restrict__ f1,
                                                             const fe_limbs *__restrict__ fd, const fe256 *__restrict__ fl,
                                                             unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long acc[R1_SLOTS];
    if (threadIdx.x < R1_SLOTS) acc[threadIdx.x] = 0;
    __syncthreads();
    const u32 cols = 1u << lo_bits, u = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = u < cols;
    const fe r = fe_canon<F>(fe_from_integer<F>(r_int));
    const fe omr = fe_canon<F>(fe_sub<F, 2>(fe_one<F>(), r));
    fe_wide18 aq, a11, ac;
    wide18_zero(aq);
    wide18_zero(a11);
    wide18_zero(ac);
    if (live) {
        const u64 half = (u64)(2 * hn) << lo_bits;
        const u32 step = gridDim.y;
        u32 since = 0;
        // the next row's number, constants, factors and entries are requested before this row's arithmetic (a row alone waits
        // for a chain of dependent scalar loads)
        u32 k = blockIdx.y;
        u32 nh = 0, nsa0 = 0, nsa1 = 0, nsc0 = 0, nsc1 = 0;
        fe_limbs nkA = {}, nkC = {}, nk0 = {}, nk1 = {}, nkd = {};
        auto fetch = [&](u32 kk) {
            nh = list[kk];
            const u32 m = smask[nh];
            const u64 b0 = ((u64)nh << lo_bits) + u, b1 = ((u64)(nh + hn) << lo_bits) + u;
            nsa0 = (m & 1u) ? s32[b0] : 0u; nsa1 = (m & 2u) ? s32[b0 + half] : 0u;
            nsc0 = (m & 4u) ? s32[b1] : 0u; nsc1 = (m & 8u) ? s32[b1 + half] : 0u;
            nkA = ka[nh]; nkC = kc[nh]; nk0 = f0[nh]; nkd = fd[nh];
            if constexpr (S11) nk1 = f1[nh];
        };
        if (k < nlist) fetch(k);
        for (; k < nlist; k += step) {
            const u32 h = nh;
            const u32 sa0 = nsa0, sa1 = nsa1, sc0 = nsc0, sc1 = nsc1;
            const fe_limbs kA = nkA, kC = nkC, k0 = nk0, k1 = nk1, kd = nkd;
            const u64 b0 = ((u64)h << lo_bits) + u, b1 = ((u64)(h + hn) << lo_bits) + u;
            if (k + step < nlist) fetch(k + step);
            u64 wa[9], wc[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                wa[i] = (u64)kA.l[i] + (u64)sa0 * omr.l[i] + (u64)sa1 * r.l[i];
                wc[i] = (u64)kC.l[i] + (u64)sc0 * omr.l[i] + (u64)sc1 * r.l[i];
            }
            const fe t0 = fe_reduce_small<F>(wa), t1 = fe_reduce_small<F>(wc);
            if constexpr (WRITE) {
                store_fe256(T + b0, fe_pack(t0));
                store_fe256(T + b1, fe_pack(t1));
            }
            const fe ts = fe_sub<F, 2>(t1, t0);
            wide18_mac(aq, ts.l, kd.l);
            if constexpr (S11) wide18_mac(a11, t1.l, k1.l);
            wide18_mac(ac, t0.l, k0.l);
            if (++since == 4) {
                wide18_carry(aq);
                if constexpr (S11) wide18_carry(a11);
                wide18_carry(ac);
                since = 0;
            }
        }
    }
    r1_block_sums<F, S11>(aq, a11, ac, live, fl, u, acc, partial);
}

// ---- the first fold, deferred by one round (round 4) ----------------------------------------------------------------------------
// With hq = a quarter of the pristine table's rows and t'[x] (x < 2 hq) the table after the first fold (challenge r1),
//   t'[h]      = KA[h] + s[h] (1 - r1) + s[h + 2hq] r1,        t'[h + hq] = KC[h] + s[h + hq] (1 - r1) + s[h + 3hq] r1      (h < hq)
// the second fold (r2) pairs t'[y] with t'[y + hq]:  t''[y] = (1 - r2) t'[y] + r2 t'[y + hq]  -- for a y whose quadruple is all
// constant / small that is ONE constant and four 4-byte sources with the coefficients (1-r1)(1-r2), r1(1-r2), (1-r1)r2, r1 r2:
// a 36-multiply-add row and one light reduction.  The sums of round three pair t''[g] with t''[g + hq/2] (g < hq/2).
template <int F> __device__ __forceinline__ fe fe_of_limbs(const fe_limbs &a) {
    fe x;
#pragma unroll
    for (int i = 0; i < 9; ++i) x.l[i] = a.l[i];
    REEF_SET_BOUND(x, 1.0);
    return x;
}
// The sums of round two need no t' either: with the pristine rows in four blocks b of hq rows (row = h + b hq),
//   sum_h f0[h] t'[h, u] = sum_h f0[h] KA[h] + sum_h (1 - r1) f0[h] s[h, u] + sum_h r1 f0[h] s[h + 2hq, u]          (side 0: b = 0, 2)
// and likewise with f1 / fd on t'[h + hq] (side 1: b = 1, 3) -- the ROUND-ONE sums kernels (k_sc_r1s_rows: 18 multiply-adds per 4-byte
// entry; k_sc_r1s_const for constant rows) with the row factors of round two scaled by (1 - r1) or r1, block by block.
// fa[b][h] = w_b * (b odd ? f1 : f0)[h],  fdb[b][h] = w_b * fd[h],  w_b = b < 2 ? 1 - r1 : r1                         (h < hq)
template <int F>
__global__ void __launch_bounds__(256) k_sc_r2s_factors(const fe_limbs *__restrict__ f0, const fe_limbs *__restrict__ f1, const fe_limbs *__restrict__ fd, u32 hq,
                                                       fe256 r1_int, fe_limbs *__restrict__ fa, fe_limbs *__restrict__ fdb) {
    const u32 h = blockIdx.x * blockDim.x + threadIdx.x;
    if (h >= hq) return;
    const fe r = fe_from_integer<F>(r1_int);
    const fe omr = fe_sub<F, 2>(fe_one<F>(), r);
    const fe a0 = fe_of_limbs<F>(f0[h]), a1 = fe_of_limbs<F>(f1[h]), d = fe_of_limbs<F>(fd[h]);
#pragma unroll
    for (int b = 0; b < 4; ++b) {
        const fe w = b < 2 ? omr : r;
        fa[(size_t)b * hq + h] = fe_to_limbs(fe_canon<F>(fe_mul<F>(w, (b & 1) ? a1 : a0)));
        fdb[(size_t)b * hq + h] = fe_to_limbs(fe_canon<F>(fe_mul<F>(w, d)));
    }
}
// K2A[g] = (1 - r2) KA[g] + r2 KC[g],  K2C[g] = the same for the quadruple g + hn2            (g < hn2 = hq / 2)
template <int F>
__global__ void __launch_bounds__(256) k_sc_r2_kprep(const fe_limbs *__restrict__ ka, const fe_limbs *__restrict__ kc, u32 hn2, fe256 r2_int,
                                                    fe_limbs *__restrict__ k2a, fe_limbs *__restrict__ k2c) {
    const u32 g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= hn2) return;
    const fe r = fe_from_integer<F>(r2_int);
    const fe a0 = fe_of_limbs<F>(ka[g]), c0 = fe_of_limbs<F>(kc[g]), a1 = fe_of_limbs<F>(ka[g + hn2]), c1 = fe_of_limbs<F>(kc[g + hn2]);
    k2a[g] = fe_to_limbs(fe_canon<F>(fe_add<F>(a0, fe_mul<F>(r, fe_sub<F, 2>(c0, a0)))));
    k2c[g] = fe_to_limbs(fe_canon<F>(fe_add<F>(a1, fe_mul<F>(r, fe_sub<F, 2>(c1, a1)))));
}
// The entries of t' that the masses of the next round read (k_sc_r1_final: T[q mod pow'], T[q mod pow' + pow']) -- a handful --
// written for the rows whose fold is deferred (and, identically, for the other constant / small ones).  One thread per entry.
template <int F>
__global__ void __launch_bounds__(256) k_sc_defer_points(const u32 *__restrict__ s32, fe256 *__restrict__ T, u32 lo_bits, u32 hq, u32 pow_next,
                                                        const u32 *__restrict__ mq, u32 nq, fe256 r1_int, const fe_limbs *__restrict__ ka,
                                                        const fe_limbs *__restrict__ kc, const u32 *__restrict__ smask) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2 * nq) return;
    const u32 p = (mq[t >> 1] % pow_next) + (t & 1u) * pow_next;
    const u32 x = p >> lo_bits, u = p & ((1u << lo_bits) - 1u);
    const u32 h = x % hq, side = x / hq;
    const u32 m = smask[h];
    if (!(m & 0x80u) || side > 1) return;
    const fe r = fe_canon<F>(fe_from_integer<F>(r1_int));
    const fe omr = fe_canon<F>(fe_sub<F, 2>(fe_one<F>(), r));
    const u64 half = (u64)(2 * hq) << lo_bits;
    const u64 b = ((u64)(h + side * hq) << lo_bits) + u;
    const u32 e0 = (m & (side ? 4u : 1u)) ? s32[b] : 0u, e1 = (m & (side ? 8u : 2u)) ? s32[b + half] : 0u;
    const fe_limbs kk = side ? kc[h] : ka[h];
    u64 w[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) w[i] = (u64)kk.l[i] + (u64)e0 * omr.l[i] + (u64)e1 * r.l[i];
    store_fe256(T + p, fe_pack(fe_reduce_small<F>(w)));
}
// The second fold of the listed g < hn2 (all eight sources constant or small) from the sources themselves, written out dense, and
// the sums of round three, as k_sc_r1_fold_coeffs would take them from the folded table.
template <int F, bool S11>
__global__ void __launch_bounds__(256) k_sc_r2_fold_coeffs_cs(const u32 *__restrict__ s32, fe256 *__restrict__ T, u32 lo_bits, u32 hq, const u32 *__restrict__ list,
                                                             u32 nlist, fe256 r1_int, fe256 r2_int, const fe_limbs *__restrict__ k2a, const fe_limbs *__restrict__ k2c,
                                                             const u32 *__restrict__ smask, const fe_limbs *__restrict__ f0, const fe_limbs *__restrict__ f1,
                                                             const fe_limbs *__restrict__ fd, const fe256 *__restrict__ fl,
                                                             unsigned long long *__restrict__ partial) {
    __shared__ unsigned long long acc[R1_SLOTS];
    if (threadIdx.x < R1_SLOTS) acc[threadIdx.x] = 0;
    __syncthreads();
    const u32 cols = 1u << lo_bits, u = blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = u < cols;
    const u32 hn2 = hq >> 1;
    const fe r1 = fe_from_integer<F>(r1_int), r2 = fe_from_integer<F>(r2_int);
    const fe o1 = fe_sub<F, 2>(fe_one<F>(), r1), o2 = fe_sub<F, 2>(fe_one<F>(), r2);
    const fe c00 = fe_canon<F>(fe_mul<F>(o1, o2)), c10 = fe_canon<F>(fe_mul<F>(r1, o2)), c01 = fe_canon<F>(fe_mul<F>(o1, r2)), c11 = fe_canon<F>(fe_mul<F>(r1, r2));
    fe_wide18 aq, a11, ac;
    wide18_zero(aq);
    wide18_zero(a11);
    wide18_zero(ac);
    if (live) {
        const u64 half = (u64)(2 * hq) << lo_bits, quarter = (u64)hq << lo_bits;
        const u32 step = gridDim.y;
        u32 since = 0;
        u32 k = blockIdx.y;
        u32 ng = 0, ns[8] = {};
        fe_limbs nkA = {}, nkC = {}, nk0 = {}, nk1 = {}, nkd = {};
        auto fetch = [&](u32 kk) {
            ng = list[kk];
            const u32 m0 = smask[ng], m1 = smask[ng + hn2];
            const u64 b0 = ((u64)ng << lo_bits) + u, b1 = ((u64)(ng + hn2) << lo_bits) + u;
            ns[0] = (m0 & 1u) ? s32[b0] : 0u; ns[1] = (m0 & 2u) ? s32[b0 + half] : 0u;
            ns[2] = (m0 & 4u) ? s32[b0 + quarter] : 0u; ns[3] = (m0 & 8u) ? s32[b0 + quarter + half] : 0u;
            ns[4] = (m1 & 1u) ? s32[b1] : 0u; ns[5] = (m1 & 2u) ? s32[b1 + half] : 0u;
            ns[6] = (m1 & 4u) ? s32[b1 + quarter] : 0u; ns[7] = (m1 & 8u) ? s32[b1 + quarter + half] : 0u;
            nkA = k2a[ng]; nkC = k2c[ng]; nk0 = f0[ng]; nkd = fd[ng];
            if constexpr (S11) nk1 = f1[ng];
        };
        if (k < nlist) fetch(k);
        for (; k < nlist; k += step) {
            const u32 g = ng;
            u32 s[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) s[j] = ns[j];
            const fe_limbs kA = nkA, kC = nkC, k0 = nk0, k1 = nk1, kd = nkd;
            if (k + step < nlist) fetch(k + step);
            u64 wa[9], wc[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                wa[i] = (u64)kA.l[i] + (u64)s[0] * c00.l[i] + (u64)s[1] * c10.l[i] + (u64)s[2] * c01.l[i] + (u64)s[3] * c11.l[i];
                wc[i] = (u64)kC.l[i] + (u64)s[4] * c00.l[i] + (u64)s[5] * c10.l[i] + (u64)s[6] * c01.l[i] + (u64)s[7] * c11.l[i];
            }
            const fe t0 = fe_reduce_small<F>(wa), t1 = fe_reduce_small<F>(wc);   // value < (2^32 - 3) M < 2^286: within fe_reduce_small's range
            store_fe256(T + ((u64)g << lo_bits) + u, fe_pack(t0));
            store_fe256(T + ((u64)(g + hn2) << lo_bits) + u, fe_pack(t1));
            const fe ts = fe_sub<F, 2>(t1, t0);
            wide18_mac(aq, ts.l, kd.l);
            if constexpr (S11) wide18_mac(a11, t1.l, k1.l);
            wide18_mac(ac, t0.l, k0.l);
            if (++since == 4) {
                wide18_carry(aq);
                if constexpr (S11) wide18_carry(a11);
                wide18_carry(ac);
                since = 0;
            }
        }
    }
    r1_block_sums<F, S11>(aq, a11, ac, live, fl, u, acc, partial);
}

// reef_sc_lookup: out[j] = T0[idx[j]] as a canonical integer, one index per lane.  T0 is the pristine table in resident form whatever it
// was set from -- k_fe_import (integers) and k_sc_set_parts (FE runs, the FILL's table form, symbols of every width, zero past the
// parts) both write all `len` entries of it -- and no fold ever writes it, so the answer is the same before, between and after rounds.
// The host has checked every index against len; the kernel checks again and writes nothing for one that is not below it.
template <int F>
static __global__ void __launch_bounds__(256) k_sc_lookup(const fe256 *__restrict__ T0, u64 len, const u64 *__restrict__ idx, u32 k, fe256 *__restrict__ out) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const u64 i = idx[j];
    if (i >= len) return;
    store_fe256(out + j, fe_to_caller<F>(fe_from_table(load_fe256(T0 + i)), 0));
}

}  // namespace reef
