// The verifier's half of an inner-product argument (include/reef_msm.h 3j): EE::verify_batch at the end of CompressedSNARK::verify
// [R] and HyraxPC::verify_eval inside verify_consistency (src/backend/commitment.rs:446-492) share one check,
//
//   s_j    = prod_i (bit_{k-1-i}(j) ? r_i : r_i^-1)                      (round 0 pairs with the most significant index bit, as 3h's folds)
//   P_hat  = comm + c q + sum_i r_i^2 L_i + sum_i r_i^-2 R_i
//   G_hat  = <s, key>,  b_hat = <s, b>
//   accept = [ P_hat == a_hat G_hat + (a_hat b_hat) q (+ blind h) ]
//
// ipa_check_engine.inc drives it:
//   k_ic_tables  s split in two: hi over the first k - m challenges, lo over the last m (eq-table scheme of k_sp_eq)
//   k_ic_eqb     b = sum_t w_t pad(eq(p_t)) built in place of an uploaded b (reef_ipa_check_eq)
//   k_ic_s       s_j = hi[j >> m] lo[j & (2^m - 1)] as the canonical integers the key's MSM reads, and the limb sums of s_j b_j in the
//                same pass (sp_block_sums / k_sp_finish)
//   the one-off points (c q, r_i^2 L_i, r_i^-2 R_i, comm, (a_hat b_hat) q, blind h), beside the G_hat MSM on a second stream:
//     the route that ships: k_normalize, k_import_key into a small plain key of the ctx's own, one MSM over it for
//                  D = P_hat - (a_hat b_hat) q - blind h (k_ic_ab forms c - a_hat b_hat on the device), a second one for P_hat
//                  when it is asked for; k_ic_final_key compares D with a_hat G_hat
//     the route measured against it (+experiment build, REEF_IPA_CHECK_ROUTE=lanes): k_ic_terms, one lane per point by
//                  double-and-add, and k_ic_final, which sums both sides; 2.1-2.9 ms of one dependent chain (profiles/r10_ipa_check_timing.txt)
//   the comparison of two points needs no inversion (xyzz_same_point)
// Scalars over field F = 1 - C, points on curve C.

namespace reef {

// tabs[0 .. 2^hb) = hi, tabs[2^hb .. 2^hb + 2^m) = lo (internal form).  f[2 i] = r_i^-1, f[2 i + 1] = r_i (internal form), hb + m of them.
template <int F>
__global__ void __launch_bounds__(256) k_ic_tables(const fe256 *__restrict__ f, u32 hb, u32 m, fe256 *__restrict__ tabs) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x, nh = 1u << hb;
    if (t >= nh + (1u << m)) return;
    const bool lo = t >= nh;
    const u32 idx = lo ? t - nh : t, bits = lo ? m : hb, off = lo ? hb : 0;
    fe acc = fe_one<F>();
    for (u32 i = 0; i < bits; ++i) acc = fe_mul<F>(acc, fe_from_table(load_fe256(f + 2 * (off + i) + ((idx >> (bits - 1 - i)) & 1u))));
    store_fe256(tabs + t, fe_to_table<F>(acc));
}

struct IcEq {
    u32 npoints;
    u32 vars[2];
    u32 off[2];          // where point t's factors start in f: f[off + 2 j] = 1 - p_j, f[off + 2 j + 1] = p_j
    fe256 w[2];          // the weights, internal form
};
// b[j] = sum_t w_t (j < 2^vars_t ? eq(p_t)[j] : 0) for j < nb, internal form; p_0 pairs with the most significant bit (k_sp_eq)
template <int F>
__global__ void __launch_bounds__(256) k_ic_eqb(IcEq a, const fe256 *__restrict__ f, u32 nb, fe256 *__restrict__ b) {
    const u32 j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= nb) return;
    fe sum = fe_zero();
    REEF_SET_BOUND(sum, 1.0);
    for (u32 t = 0; t < a.npoints; ++t) {
        const u32 v = a.vars[t];
        if (j >> v) continue;
        fe e = fe_from_table(a.w[t]);
        for (u32 i = 0; i < v; ++i) e = fe_mul<F>(e, fe_from_table(load_fe256(f + a.off[t] + 2 * i + ((j >> (v - 1 - i)) & 1u))));
        sum = fe_canon<F>(fe_add<F>(sum, e));
    }
    store_fe256(b + j, fe_pack(sum));
}

// b's form in k_ic_s: the SP_FORM_* of spartan_kernels.inc (table: k_ic_eqb's; integer / Montgomery: the caller's)
// s_out[j] = s_j (canonical integers) for j < n -- or scale s_j (scaled; scale: internal form), so that the MSM over them is a_hat G_hat
// and no 255-step chain follows it; partial[block][0..9) = the limb sums of s_j b_j over j < b_len
template <int F>
__global__ void __launch_bounds__(SP_THREADS) k_ic_s(const fe256 *__restrict__ tabs, u32 hb, u32 m, u32 n, const fe256 *__restrict__ b, u32 b_len,
                                                     int b_form, fe256 scale, int scaled, fe256 *__restrict__ s_out,
                                                     unsigned long long *__restrict__ partial) {
    const fe256 *hi = tabs, *lo = tabs + (1u << hb);
    const u32 mask = (1u << m) - 1;
    u64 acc[1][9];
#pragma unroll
    for (int i = 0; i < 9; ++i) acc[0][i] = 0;
    for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const fe s = fe_mul<F>(fe_from_table(load_fe256(hi + (j >> m))), fe_from_table(load_fe256(lo + (j & mask))));
        store_fe256(s_out + j, fe_to_integer<F>(scaled ? fe_mul<F>(s, fe_from_table(scale)) : s));
        if (j < b_len) {
            const fe256 raw = load_fe256(b + j);
            const fe bv = b_form == SP_FORM_TABLE ? fe_from_table(raw) : fe_canon<F>(fe_from_caller<F>(raw, b_form == SP_FORM_MONT));
            sp_acc(acc[0], fe_mul<F>(s, bv));
        }
    }
    sp_block_sums<1>(acc, partial);
}

// What the check hands back, on the device until the call's one wait
struct IcOut {
    jacobian256 p_hat;
    fe256 b_hat;         // the caller's form
    u32 accept, pad[7];
};

// out[t] = scalars[t] * pts[t] for t < nt (ABI Jacobian points, canonical integer scalars), one lane each: plain double-and-add,
// the latency of one 255-bit chain whatever nt is.  Term ab_idx takes a_hat * b_hat (both internal form, on the device) instead.
template <int C>
__global__ void __launch_bounds__(64) k_ic_terms(const jacobian256 *__restrict__ pts, const fe256 *__restrict__ scalars, u32 nt, u32 ab_idx,
                                                 fe256 a_hat, const fe256 *__restrict__ b_hat, xyzz_mem *__restrict__ out) {
    constexpr int F = 1 - C;
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nt) return;
    fe256 k = load_fe256(scalars + t);
    if (t == ab_idx) k = fe_to_integer<F>(fe_mul<F>(fe_from_table(a_hat), fe_from_table(load_fe256(b_hat))));
    const xyzz p = xyzz_from_abi_jacobian<C>(pts[t]);
    xyzz acc = xyzz_identity();
    for (int i = 254; i >= 0; --i) {
        acc = xyzz_dbl<C>(acc);
        if ((k.w[i >> 5] >> (i & 31)) & 1u) acc = xyzz_add<C>(acc, p);
    }
    out[t] = xyzz_to_mem(acc);
}

// Two points in XYZZ form are the same group element: X1 ZZ2 == X2 ZZ1 and Y1 ZZZ2 == Y2 ZZZ1 (ZZ = Z^2, ZZZ = Z^3: the Jacobian
// X1 Z2^2 == X2 Z1^2, Y1 Z2^3 == Y2 Z1^3), no inversion; the identity equals the identity only.
template <int C> __device__ __forceinline__ bool xyzz_same_point(const xyzz &a, const xyzz &b) {
    const bool a_inf = xyzz_is_inf<C>(a), b_inf = xyzz_is_inf<C>(b);
    if (a_inf || b_inf) return a_inf && b_inf;
    const fe dx = fe_sub<C, 2>(fe_mul<C>(a.x, b.zz), fe_mul<C>(b.x, a.zz));
    const fe dy = fe_sub<C, 2>(fe_mul<C>(a.y, b.zzz), fe_mul<C>(b.y, a.zzz));
    return fe_is_zero<C>(dx) && fe_is_zero<C>(dy);
}

// The key route's scalar of q: row[0] = c - a_hat b_hat (canonical integer; c, a_hat, b_hat internal form).  One thread.
template <int F>
__global__ void __launch_bounds__(64) k_ic_ab(fe256 c, fe256 a_hat, const fe256 *__restrict__ b_hat, fe256 *__restrict__ row) {
    if (blockIdx.x | threadIdx.x) return;
    const fe ab = fe_mul<F>(fe_from_table(a_hat), fe_from_table(load_fe256(b_hat)));
    store_fe256(row, fe_to_integer<F>(fe_sub<F, 2>(fe_from_table(c), ab)));
}
// The key route's end: accept = [D == a_hat G_hat]; g_scaled: g_hat holds a_hat G_hat already, else the 255-step chain runs here
// (only when the caller asked for G_hat itself).  p: P_hat when it was asked for, or NULL.  One thread.
template <int C>
__global__ void __launch_bounds__(64) k_ic_final_key(const jacobian256 *__restrict__ d, const jacobian256 *__restrict__ p,
                                                     const jacobian256 *__restrict__ g_hat, fe256 a_hat_int, int g_scaled,
                                                     const fe256 *__restrict__ b_hat, int form, IcOut *__restrict__ out) {
    constexpr int F = 1 - C;
    if (blockIdx.x | threadIdx.x) return;
    const xyzz g = xyzz_from_abi_jacobian<C>(load_jacobian256(g_hat));
    xyzz acc = g_scaled ? g : xyzz_identity();
    for (int i = g_scaled ? -1 : 254; i >= 0; --i) {
        acc = xyzz_dbl<C>(acc);
        if ((a_hat_int.w[i >> 5] >> (i & 31)) & 1u) acc = xyzz_add<C>(acc, g);
    }
    out->accept = xyzz_same_point<C>(xyzz_from_abi_jacobian<C>(load_jacobian256(d)), acc) ? 1u : 0u;
    jacobian256 ph;
#pragma unroll
    for (int i = 0; i < 8; ++i) ph.x.w[i] = ph.y.w[i] = ph.z.w[i] = 0;
    if (p) ph = load_jacobian256(p);
    store_jacobian256(&out->p_hat, ph);
    store_fe256(&out->b_hat, sp_out<F>(fe_from_table(load_fe256(b_hat)), form));
}

// Thread 0: P_hat = comm + terms[0 .. np); thread 1: rhs = a_hat G_hat + terms[np .. nt); then thread 0 compares and writes out
// (b_hat: internal form in, `form` out).  g_scaled: g_hat holds a_hat G_hat already (k_ic_s scaled s).  One block of 64.
template <int C>
__global__ void __launch_bounds__(64) k_ic_final(const jacobian256 *__restrict__ comm, const xyzz_mem *__restrict__ terms, u32 np, u32 nt,
                                                 const jacobian256 *__restrict__ g_hat, fe256 a_hat_int, int g_scaled, const fe256 *__restrict__ b_hat,
                                                 int form, IcOut *__restrict__ out) {
    constexpr int F = 1 - C;
    __shared__ xyzz_mem rhs_mem;
    if (threadIdx.x == 1) {
        const xyzz g = xyzz_from_abi_jacobian<C>(*g_hat);
        xyzz acc = g_scaled ? g : xyzz_identity();
        for (int i = g_scaled ? -1 : 254; i >= 0; --i) {
            acc = xyzz_dbl<C>(acc);
            if ((a_hat_int.w[i >> 5] >> (i & 31)) & 1u) acc = xyzz_add<C>(acc, g);
        }
        for (u32 t = np; t < nt; ++t) acc = xyzz_add<C>(acc, xyzz_from_mem(terms[t]));
        rhs_mem = xyzz_to_mem(acc);
    }
    xyzz p = xyzz_identity();
    if (threadIdx.x == 0) {
        p = xyzz_from_abi_jacobian<C>(*comm);
        for (u32 t = 0; t < np; ++t) p = xyzz_add<C>(p, xyzz_from_mem(terms[t]));
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    out->accept = xyzz_same_point<C>(p, xyzz_from_mem(rhs_mem)) ? 1u : 0u;
    out->p_hat = xyzz_to_abi_jacobian<C>(p);
    store_fe256(&out->b_hat, sp_out<F>(fe_from_table(load_fe256(b_hat)), form));
}

// ---------------------------------------------------------------- a batch of checks against one key (include/reef_msm.h 3m)
// m proofs over the same n collapse into one equation under the caller's weights rho_i:
//   sum_i rho_i (comm_i + c_i q_i + sum_t r_it^2 L_it + sum_t r_it^-2 R_it - (a_hat_i b_hat_i) q_i - blind_i h_i)  ==  < S, key >
//   S_j = sum_i w_i s^(i)_j,  w_i = rho_i a_hat_i
//   k_ic_tables_batch  the m pairs of challenge tables in one launch, w_i folded into proof i's hi table
//   k_ic_s_batch       S as the canonical integers the key's MSM reads: one product per proof and entry, five products per
//                      Montgomery reduction (wide18_mont), the reduced groups summed limb by limb and made canonical once
//   k_ic_final_batch   the comparison (xyzz_same_point)
// b_hat_i has a closed form of O(k) products and is formed on the host (ipa_check_engine.inc), so every scalar of every one-off
// point is known before anything is enqueued: k_ic_eqb, the per-entry products s_j b_j and k_ic_ab have no counterpart here.

// Proof p's tables at tabs + p ntab, ntab = 2^hb + 2^m: hi over its first hb challenges times w[p], as canonical INTEGERS, then lo over
// its last m, internal form -- the Montgomery product of the two is the canonical-integer residue of w s_j, with no conversion after
// it.  f[2 (p (hb + m) + i)] = r_i^-1, f[.. + 1] = r_i of proof p; w: internal form.
template <int F>
__global__ void __launch_bounds__(256) k_ic_tables_batch(const fe256 *__restrict__ f, const fe256 *__restrict__ w, u32 hb, u32 m, u32 nproofs,
                                                         fe256 *__restrict__ tabs) {
    const u32 nh = 1u << hb, ntab = nh + (1u << m);
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= (u64)nproofs * ntab) return;
    const u32 p = (u32)(g / ntab), t = (u32)(g % ntab);
    const bool lo = t >= nh;
    const u32 idx = lo ? t - nh : t, bits = lo ? m : hb, off = lo ? hb : 0;
    const fe256 *fp = f + 2 * (size_t)p * (hb + m);
    fe acc = lo ? fe_one<F>() : fe_from_table(load_fe256(w + p));
    for (u32 i = 0; i < bits; ++i) acc = fe_mul<F>(acc, fe_from_table(load_fe256(fp + 2 * (off + i) + ((idx >> (bits - 1 - i)) & 1u))));
    store_fe256(tabs + g, lo ? fe_to_table<F>(acc) : fe_to_integer<F>(acc));
}

// s_out[j] = sum_p hi_p[j >> m] lo_p[j & (2^m - 1)] mod M for j < n, canonical integers.  UNI (m >= 6 and n a multiple of 64): the 64
// entries of a wave share j >> m, so a proof's hi entry is one load per wave.  Limb bounds: the tables are canonical (limbs < 2^29), a
// product adds 9 terms < 2^58 to a column, the columns are carried after the fourth product of a group and wide18_mont carries again:
// five products < 5 M^2 give a residue < 2 M with exact limbs.  At most 4096 / 5 + 1 such residues are added limb by limb (< 2^40
// per limb, value < 2^11 M: fe_from_limb_sums takes 2^30 M).  No scratch, no atomics: an entry is one thread's.
template <int F, bool UNI>
__global__ void __launch_bounds__(SP_THREADS) k_ic_s_batch(const fe256 *__restrict__ tabs, u32 hb, u32 m, u32 n, u32 nproofs, fe256 *__restrict__ s_out) {
    const u32 nh = 1u << hb, ntab = nh + (1u << m), mask = (1u << m) - 1;
    for (u32 j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        u32 jh = j >> m;
        if constexpr (UNI) jh = (u32)__builtin_amdgcn_readfirstlane((int)jh);
        const fe256 *hi = tabs + jh, *lo = tabs + nh + (j & mask);
        fe_wide sums;
        wide_zero(sums);
        u32 p = 0;
        for (; p + 5 <= nproofs; p += 5) {
            fe_wide18 w;
            wide18_zero(w);
#pragma unroll
            for (int t = 0; t < 5; ++t) {
                wide18_mac(w, fe_from_table(load_fe256(hi)).l, fe_from_table(load_fe256(lo)).l);
                if (t == 3) wide18_carry(w);
                hi += ntab;
                lo += ntab;
            }
            const fe r = wide18_mont<F>(w, 2.0);
#pragma unroll
            for (int i = 0; i < 9; ++i) sums.l[i] += r.l[i];
        }
        if (p < nproofs) {                                      // the last one to four proofs: no carry between them
            fe_wide18 w;
            wide18_zero(w);
            for (; p < nproofs; ++p) {
                wide18_mac(w, fe_from_table(load_fe256(hi)).l, fe_from_table(load_fe256(lo)).l);
                hi += ntab;
                lo += ntab;
            }
            const fe r = wide18_mont<F>(w, 2.0);
#pragma unroll
            for (int i = 0; i < 9; ++i) sums.l[i] += r.l[i];
        }
        store_fe256(s_out + j, fe_pack(fe_from_limb_sums<F>(sums)));
    }
}

// accept = [d == g] as group elements: the two sides of the combined equation.  One thread.
template <int C>
__global__ void __launch_bounds__(64) k_ic_final_batch(const jacobian256 *__restrict__ d, const jacobian256 *__restrict__ g, u32 *__restrict__ accept) {
    if (blockIdx.x | threadIdx.x) return;
    *accept = xyzz_same_point<C>(xyzz_from_abi_jacobian<C>(load_jacobian256(d)), xyzz_from_abi_jacobian<C>(load_jacobian256(g))) ? 1u : 0u;
}

}  // namespace reef
