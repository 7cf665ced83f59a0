// Row N4 of SURVEY.md 8f: the Poseidon Merkle commitment of the document (`--merkle`,
// src/backend/merkle_tree.rs:25-114) as batched hash kernels over the scalar field of the curve
// (Reef: G1::Scalar = Fq).  One thread per tree node, one Poseidon permutation per node:
//   leaf   i   = H4(2i, doc[2i], 2i+1, doc[2i+1])     (an odd tail hashes (2i, doc[2i], 0, 0))      merkle_tree.rs:31-50, :87-92
//   parent i   = H2(child[2i], child[2i+1])             (an odd tail hashes (child[2i], 0))          merkle_tree.rs:53-71, :93-98
// H_k(x) = P([tag_k, x_1..x_k, 0..])[1] with P the Poseidon permutation of width 5: what neptune's Sponge (arity U4,
// Mode::Simplex, IOPattern [Absorb(k), Squeeze(1)]) computes for one absorb-then-squeeze [R].  The permutation's
// round constants, its MDS matrix and the two domain tags are INPUTS (neptune's PoseidonConstants and the tags its
// SAFE API derives from the IO patterns live in a crate that is not in the reference tree): the Rust binding passes
// them, so the tree is the reference's tree by construction; the oracle and the tests use stand-in constants.
//
// Included by kernels_<curve>.hip after fe_vec.h; F = scalar field of the curve.
namespace reef {

static constexpr int POS_T = 5;    // width: arity 4 + the capacity element

// A sum of up to five products takes ONE Montgomery reduction (lazy 18-column accumulation, fe_vec.h: wide18_mont); operands
// normalised with sum (A/M)(B/M) < 128; result exact limbs, value < 2 M.

struct PoseidonDev {
    const fe256 *rc;      // dense form: POS_T * (rf + rp) round constants, round-major.  Sparse form: the rf full rounds only, the
                          // first one after the partial rounds carrying what the partial rounds pushed forward.  Internal form.
    const fe256 *mds;     // POS_T * POS_T, internal form: new[j] = sum_i state[i] * mds[i*POS_T + j]
    const fe256 *sparse;  // sparse form, (rp - 1) x 10 per partial round but the last: c, a, v[1..4], w[1..4]; NULL: dense form
    const fe256 *last;    // sparse form, last partial round: c, then the dense matrix D*M (25)
    u32 rf, rp;           // full rounds (half before, half after the partial ones), partial rounds
};

template <int F> __device__ __forceinline__ fe pos_sbox(const fe &x) {   // x^5; x < 4
    const fe x2 = fe_sqr<F>(x);           // 16/128 -> < 1.13
    const fe x4 = fe_sqr<F>(x2);
    return fe_mul<F>(x4, x);              // < 1.04
}
// s <- s * m (row vector times matrix), every output one 5-term dot product with ONE reduction; sum of (s_i/M) < 128
template <int F> __device__ __forceinline__ void pos_mds(fe (&s)[POS_T], const fe256 *__restrict__ m) {
    fe n[POS_T];
#pragma unroll
    for (int j = 0; j < POS_T; ++j) {
        fe_wide18 w;
        wide18_zero(w);
#pragma unroll
        for (int i = 0; i < POS_T; ++i) {
            const fe e = fe_from_table(load_fe256(m + i * POS_T + j));
            wide18_mac(w, s[i].l, e.l);
            if (i == 3) wide18_carry(w);                                     // four products fit between carries
        }
        n[j] = wide18_mont<F>(w, 2.0);
    }
#pragma unroll
    for (int j = 0; j < POS_T; ++j) s[j] = n[j];
}
template <int F> __device__ __forceinline__ void pos_full_round(fe (&s)[POS_T], const fe256 *__restrict__ rc, const fe256 *__restrict__ mds) {
#pragma unroll
    for (int i = 0; i < POS_T; ++i) s[i] = pos_sbox<F>(fe_add<F>(s[i], fe_from_table(load_fe256(rc + i))));   // < 3 into the S-box
    pos_mds<F>(s, mds);
}
// The permutation as defined (every round: constants, S-box, dense matrix).
template <int F> __device__ __forceinline__ void poseidon_permute_dense(fe (&s)[POS_T], const PoseidonDev &p) {
    const u32 rounds = p.rf + p.rp, half = p.rf / 2;
    for (u32 r = 0; r < rounds; ++r) {
        const bool full = r < half || r >= half + p.rp;
        if (full) {
            pos_full_round<F>(s, p.rc + r * POS_T, p.mds);
        } else {
#pragma unroll
            for (int i = 0; i < POS_T; ++i) s[i] = fe_add<F>(s[i], fe_from_table(load_fe256(p.rc + r * POS_T + i)));
            s[0] = pos_sbox<F>(s[0]);
            pos_mds<F>(s, p.mds);
        }
    }
}
// The same function with the partial rounds in their sparse form (merkle_engine.inc derives the constants; the Poseidon
// paper's appendix B optimisation, re-derived for the row-vector convention used here):
//   * a partial round's constants on elements 1..4 commute with its S-box (which touches element 0 only), so they are
//     pushed through the matrix into the next round's constants: one constant per partial round;
//   * M_k = S_k * D_k with D_k = diag(1, D^) and S_k = [[a, v], [w, I]]; D_k commutes with the next round's S-box and
//     constant and is merged into the next matrix (M_{k+1} = D_k * M), so a partial round is
//         s0 <- (s0 + c)^5;  new0 = a*s0 + sum_i w_i*s_i;  s_j <- v_j*s0 + s_j  (j = 1..4);  s0 <- new0
//     9 products with 5 reductions where the dense form has 25 with 5 (and 4 more additions); the last partial round
//     applies the accumulated dense matrix.  Exact field arithmetic: the outputs are the dense form's, bit for bit.
template <int F> __device__ __forceinline__ void poseidon_permute_sparse(fe (&s)[POS_T], const PoseidonDev &p) {
    const u32 half = p.rf / 2;
    const fe one = fe_one<F>();
    for (u32 r = 0; r < half; ++r) pos_full_round<F>(s, p.rc + r * POS_T, p.mds);
    for (u32 k = 0; k + 1 < p.rp; ++k) {
        const fe256 *c = p.sparse + (size_t)k * 10;
        const fe s0 = pos_sbox<F>(fe_add<F>(s[0], fe_from_table(load_fe256(c))));          // < 1.04
        fe_wide18 w;
        wide18_zero(w);
        wide18_mac(w, s0.l, fe_from_table(load_fe256(c + 1)).l);
#pragma unroll
        for (int i = 1; i < POS_T; ++i) {
            wide18_mac(w, s[i].l, fe_from_table(load_fe256(c + 5 + i)).l);                  // s_i < 18 (renormalised below): sum < 74
            if (i == 3) wide18_carry(w);
        }
#pragma unroll
        for (int j = 1; j < POS_T; ++j) s[j] = fe_add<F>(fe_mul<F>(fe_from_table(load_fe256(c + 1 + j)), s0), s[j]);   // grows by < 2 per round
        s[0] = wide18_mont<F>(w, 2.0);
        if ((k & 7u) == 7u) {
#pragma unroll
            for (int j = 1; j < POS_T; ++j) s[j] = fe_mul<F>(s[j], one);                    // back below 2
        }
    }
    if (p.rp) {
        s[0] = pos_sbox<F>(fe_add<F>(s[0], fe_from_table(load_fe256(p.last))));
        pos_mds<F>(s, p.last + 1);
    }
    for (u32 r = half; r < p.rf; ++r) pos_full_round<F>(s, p.rc + r * POS_T, p.mds);
}
template <int F> __device__ __forceinline__ void poseidon_permute(fe (&s)[POS_T], const PoseidonDev &p) {
    if (p.sparse) poseidon_permute_sparse<F>(s, p);
    else poseidon_permute_dense<F>(s, p);
}
__device__ __forceinline__ fe256 fe256_of_u64(u64 v) {
    fe256 r;
    r.w[0] = (u32)v; r.w[1] = (u32)(v >> 32);
#pragma unroll
    for (int k = 2; k < 8; ++k) r.w[k] = 0;
    return r;
}

// Leaves: node i over symbols 2i, 2i+1 of `doc` (n symbols, 32-bit each: Reef's alphabet indices, framework.rs:978-1011).  `doc` may be a SLICE
// of the document that starts at symbol index_base (even): the hash takes the symbols' positions in the whole document.
template <int F>
__global__ void __launch_bounds__(256) k_pos_leaves(const u32 *__restrict__ doc, u64 n, u64 index_base, PoseidonDev p, fe256 tag, fe256 *__restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 nodes = (n + 1) / 2;
    if (i >= nodes) return;
    fe s[POS_T];
    s[0] = fe_from_table(tag);
    s[1] = fe_from_integer<F>(fe256_of_u64(index_base + 2 * i));
    s[2] = fe_from_integer<F>(fe256_of_u64(doc[2 * i]));
    if (2 * i + 1 < n) {
        s[3] = fe_from_integer<F>(fe256_of_u64(index_base + 2 * i + 1));
        s[4] = fe_from_integer<F>(fe256_of_u64(doc[2 * i + 1]));
    } else {
        s[3] = fe_zero(); s[4] = fe_zero();
        REEF_SET_BOUND(s[3], 1.0); REEF_SET_BOUND(s[4], 1.0);
    }
    poseidon_permute<F>(s, p);
    store_fe256(out + i, fe_to_table<F>(s[1]));
}
// Parents: node i over children 2i, 2i+1 of the level below (m nodes).
template <int F>
__global__ void __launch_bounds__(256) k_pos_nodes(const fe256 *__restrict__ below, u64 m, PoseidonDev p, fe256 tag, fe256 *__restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 nodes = (m + 1) / 2;
    if (i >= nodes) return;
    fe s[POS_T];
    s[0] = fe_from_table(tag);
    s[1] = fe_from_table(load_fe256(below + 2 * i));
    s[2] = fe_zero();
    REEF_SET_BOUND(s[2], 1.0);
    if (2 * i + 1 < m) s[2] = fe_from_table(load_fe256(below + 2 * i + 1));
    s[3] = fe_zero(); s[4] = fe_zero();
    REEF_SET_BOUND(s[3], 1.0); REEF_SET_BOUND(s[4], 1.0);
    poseidon_permute<F>(s, p);
    store_fe256(out + i, fe_to_table<F>(s[1]));
}

// ---- the same hashes with FIVE LANES PER HASH, for the levels that do not fill the chip --------------------------------
// A hash is ~1000 dependent field products for its thread (~0.4 ms whatever the width of the level), so the upper levels of
// a tree -- and every level of a small document's -- are a latency chain: 16 levels of a 2^16-symbol document cost 6.8 ms.
// Here the five state elements of a hash sit in five consecutive lanes (12 hashes per wave, one wave per workgroup) and
// meet through LDS: a full round is S-box (3 products) + one 5-term dot product per lane (2.2) instead of 5 x both; a sparse
// partial round is sqr, sqr, mul, ONE exchange, mul -- lane 0 finishes its S-box while lanes 1..4 use the same multiply
// slot for w_i*s_i, then lane 0 multiplies a*s0' while lanes 1..4 multiply v_i*s0' -- 4 product-times instead of 12.
// Same constants, same arithmetic, same digests as poseidon_permute_sparse (tests/test_gpu_merkle.py compares whole trees).
static constexpr u32 POS_SPREAD_PER_WAVE = 12;         // hashes per wave (60 lanes)
static constexpr u32 POS_SPREAD_MAX_NODES = 16384;     // levels up to this many nodes take the five-lane form (swept: 8192..32768 within 3 %)
struct PosSpreadLds { u32 l[2][9][64]; };              // two buffers (one barrier per exchange), limb-major: conflict-free

__device__ __forceinline__ void pos_spread_put(PosSpreadLds &L, int buf, int lane, const fe &v) {
#pragma unroll
    for (int i = 0; i < 9; ++i) L.l[buf][i][lane] = v.l[i];
}
__device__ __forceinline__ fe pos_spread_get(const PosSpreadLds &L, int buf, int src) {
    fe r;
#pragma unroll
    for (int i = 0; i < 9; ++i) r.l[i] = L.l[buf][i][src];
    REEF_SET_BOUND(r, 32.0);
    return r;
}
// s <- (state of this lane's hash) * column `elem` of m, through LDS buffer `buf`
template <int F>
__device__ __forceinline__ fe pos_spread_mds(const fe &s, int elem, int base, int lane, const fe256 *__restrict__ m, PosSpreadLds &L, int buf) {
    pos_spread_put(L, buf, lane, s);
    __syncthreads();
    fe_wide18 w;
    wide18_zero(w);
#pragma unroll
    for (int i = 0; i < POS_T; ++i) {
        const fe e = fe_from_table(load_fe256(m + i * POS_T + elem));
        const fe si = pos_spread_get(L, buf, base + i);
        wide18_mac(w, si.l, e.l);
        if (i == 3) wide18_carry(w);
    }
    return wide18_mont<F>(w, 2.0);
}
template <int F>
__device__ __forceinline__ fe poseidon_permute_spread(fe s, int elem, int base, int lane, const PoseidonDev &p, PosSpreadLds &L) {
    const u32 half = p.rf / 2;
    const fe one = fe_one<F>();
    int buf = 0;
    for (u32 r = 0; r < half; ++r) {
        s = pos_sbox<F>(fe_add<F>(s, fe_from_table(load_fe256(p.rc + r * POS_T + elem))));
        s = pos_spread_mds<F>(s, elem, base, lane, p.mds, L, buf);
        buf ^= 1;
    }
    for (u32 k = 0; k + 1 < p.rp; ++k) {
        const fe256 *c = p.sparse + (size_t)k * 10;
        // lane 0: x = s0 + c, s0' = x^5; lanes 1..4 ride along and use the last multiply for w_i * s_i
        fe x = s;
        if (elem == 0) x = fe_add<F>(s, fe_from_table(load_fe256(c)));
        const fe x2 = fe_sqr<F>(x);
        const fe x4 = fe_sqr<F>(x2);
        const fe f1 = elem == 0 ? x4 : fe_from_table(load_fe256(c + 5 + elem));        // x^4 | w_i
        const fe m1 = fe_mul<F>(f1, elem == 0 ? x : s);                                 // s0' | w_i * s_i   (both < 2)
        pos_spread_put(L, buf, lane, m1);
        __syncthreads();
        const fe s0p = pos_spread_get(L, buf, base);
        const fe f2 = fe_from_table(load_fe256(c + 1 + elem));                          // a | v_i
        const fe m2 = fe_mul<F>(f2, s0p);                                               // a * s0' | v_i * s0'
        if (elem == 0) {
            fe acc = m2;                                                                // + sum_i w_i * s_i: < 10
#pragma unroll
            for (int i = 1; i < POS_T; ++i) acc = fe_add<F>(acc, pos_spread_get(L, buf, base + i));
            s = acc;
        } else {
            s = fe_add<F>(m2, s);                                                       // grows by < 2 per round
            if ((k & 7u) == 7u) s = fe_mul<F>(s, one);                                  // back below 2
        }
        buf ^= 1;
    }
    if (p.rp) {
        if (elem == 0) s = pos_sbox<F>(fe_add<F>(s, fe_from_table(load_fe256(p.last))));
        s = pos_spread_mds<F>(s, elem, base, lane, p.last + 1, L, buf);
        buf ^= 1;
    }
    for (u32 r = half; r < p.rf; ++r) {
        s = pos_sbox<F>(fe_add<F>(s, fe_from_table(load_fe256(p.rc + r * POS_T + elem))));
        s = pos_spread_mds<F>(s, elem, base, lane, p.mds, L, buf);
        buf ^= 1;
    }
    return s;
}
// LEAVES: node i over symbols 2i, 2i + 1 of doc (a slice that starts at symbol index_base of the document); otherwise over children 2i, 2i + 1
// of `below` (m of them).  One wave per block.
template <int F, bool LEAVES>
__global__ void __launch_bounds__(64) k_pos_spread(const u32 *__restrict__ doc, const fe256 *__restrict__ below, u64 m, u64 index_base, PoseidonDev p, fe256 tag,
                                                  fe256 *__restrict__ out) {
    __shared__ PosSpreadLds L;
    const int lane = threadIdx.x, elem = lane % POS_T, base = lane - elem;
    const u64 i = (u64)blockIdx.x * POS_SPREAD_PER_WAVE + (u32)(lane / POS_T);
    const u64 nodes = (m + 1) / 2;
    const bool live = lane < (int)(POS_SPREAD_PER_WAVE * POS_T) && i < nodes;
    fe s = fe_zero();
    REEF_SET_BOUND(s, 1.0);
    if (live) {
        if (elem == 0) s = fe_from_table(tag);
        else if constexpr (LEAVES) {
            const u64 sym = 2 * i + (u64)((elem - 1) >> 1);                              // elements 1, 2: symbol 2i; 3, 4: symbol 2i + 1
            if (sym < m) s = fe_from_integer<F>(fe256_of_u64((elem & 1) ? index_base + sym : (u64)doc[sym]));
        } else {
            if (elem <= 2 && 2 * i + (u64)(elem - 1) < m) s = fe_from_table(load_fe256(below + 2 * i + (u64)(elem - 1)));
        }
    }
    const int safe_base = lane < (int)(POS_SPREAD_PER_WAVE * POS_T) ? base : 55;         // idle lanes 60..63 read a live group's slots
    s = poseidon_permute_spread<F>(s, lane < (int)(POS_SPREAD_PER_WAVE * POS_T) ? elem : 0, safe_base, lane, p, L);
    if (live && elem == 1) store_fe256(out + i, fe_to_table<F>(s));
}

// ---- the resident tree (merkle_resident_engine.inc): openings gathered from it, and the root recomputed from claimed openings ----
static constexpr u32 MERKLE_MAX_LEVELS = 33;           // documents are shorter than 2^33 symbols
struct MerkleShape {                                   // the levels of a resident tree: level h is tree[off[h] .. off[h] + len[h])
    u64 off[MERKLE_MAX_LEVELS], len[MERKLE_MAX_LEVELS];
    u64 n;                                             // symbols of the document
    u32 levels;
};
// make_wits as arrays (merkle_tree.rs:116-190), one thread per (query, depth), into a packed staging buffer in the caller's form:
// opposite[k * L] | path[k * L] (want_path) | opposite_idx[k] | symbols[k].  Every idx[j] < n (checked on the host).
template <int F>
__global__ void __launch_bounds__(256) k_merkle_open(const u32 *__restrict__ doc, const fe256 *__restrict__ tree, MerkleShape sh, const u64 *__restrict__ idx, u64 k,
                                                   int to_mont, int want_path, fe256 *__restrict__ opposite, fe256 *__restrict__ path,
                                                   u64 *__restrict__ opposite_idx, u32 *__restrict__ symbols) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 L = sh.levels;
    if (t >= k * L) return;
    const u64 j = t / L;
    const u32 h = (u32)(t - j * L);
    const u64 q = idx[j];
    fe256 opp = fe256_of_u64(0);                       // zero is zero in either form
    if (h == 0) {
        const u64 sib = q ^ 1;
        const bool have = sib < sh.n;                  // only an even last symbol has no sibling
        const u32 v = have ? doc[sib] : 0u;
        if (v) opp = to_mont ? fe_to_abi<F>(fe_from_integer<F>(fe256_of_u64(v))) : fe256_of_u64(v);
        opposite_idx[j] = have ? sib : 0;
        symbols[j] = doc[q];
    } else {
        const u64 sib = (q >> h) ^ 1;                  // the sibling of the path's node in level h - 1
        if (sib < sh.len[h - 1]) opp = fe_to_caller<F>(fe_from_table(load_fe256(tree + sh.off[h - 1] + sib)), to_mont);
    }
    store_fe256(opposite + t, opp);
    if (want_path) store_fe256(path + t, fe_to_caller<F>(fe_from_table(load_fe256(tree + sh.off[h] + (q >> (h + 1)))), to_mont));
}

// The inputs of one depth of a claimed opening: `self` is the symbol's side (depth 0) or the running digest, `opp` the claimed sibling.
// Depth 0 is H4(idx, sym, opp_idx, opp) or H4(opp_idx, opp, idx, sym) by bit 0 of idx; depth h >= 1 is H2(digest, opp) or H2(opp, digest) by
// bit h (merkle_tree.rs:222-249).  Returns element `elem` of the state the hash starts from.
template <int F>
__device__ __forceinline__ fe merkle_path_input(int elem, u32 h, u64 q, u32 sym, u64 oidx, const fe256 &opp_raw, int is_mont, const fe &digest, const fe256 &tag_leaf,
                                                const fe256 &tag_node) {
    fe z = fe_zero();
    REEF_SET_BOUND(z, 1.0);
    const bool left = ((q >> h) & 1) == 0;             // the path's node is the left child
    if (elem == 0) return fe_from_table(h == 0 ? tag_leaf : tag_node);
    if (h == 0) {
        const bool own = left ? elem <= 2 : elem >= 3; // elements 1, 2: the left (index, symbol); 3, 4: the right
        if (elem & 1) return fe_from_integer<F>(fe256_of_u64(own ? q : oidx));
        return own ? fe_from_integer<F>(fe256_of_u64(sym)) : fe_from_caller<F>(opp_raw, is_mont);
    }
    if (elem > 2) return z;
    return (elem == 1) == left ? digest : fe_from_caller<F>(opp_raw, is_mont);
}
// Five lanes per hash, 12 paths per wave, one wave per block: a path is a chain of L dependent hashes, the running digest kept in lane
// elem == 1 of its group.  The permutation meets at barriers, so EVERY lane runs all L depths: idle groups hash zeros to the end.
// opposite: k * L elements in the caller's form (below the modulus: checked on the host); accept[j] = the recomputed root is `root`'s.
template <int F>
__global__ void __launch_bounds__(64) k_pos_paths(const u64 *__restrict__ idx, const u32 *__restrict__ symbols, const u64 *__restrict__ opposite_idx,
                                                 const fe256 *__restrict__ opposite, u64 k, u32 levels, int is_mont, PoseidonDev p, fe256 tag_leaf, fe256 tag_node,
                                                 const fe256 *__restrict__ root, u32 *__restrict__ accept) {
    __shared__ PosSpreadLds L;
    const int lane = threadIdx.x, elem = lane % POS_T, base = lane - elem;
    const bool in_group = lane < (int)(POS_SPREAD_PER_WAVE * POS_T);
    const u64 j = (u64)blockIdx.x * POS_SPREAD_PER_WAVE + (u32)(lane / POS_T);
    const bool live = in_group && j < k;
    const int safe_base = in_group ? base : 55, safe_elem = in_group ? elem : 0;         // idle lanes 60..63 read a live group's slots
    const u64 q = live ? idx[j] : 0, oidx = live ? opposite_idx[j] : 0;
    const u32 sym = live ? symbols[j] : 0;
    fe s = fe_zero();
    REEF_SET_BOUND(s, 1.0);
    for (u32 h = 0; h < levels; ++h) {
        fe digest;                                                                       // of depth h - 1: every lane takes it from lane elem == 1 of its group
#pragma unroll
        for (int i = 0; i < 9; ++i) digest.l[i] = (u32)__shfl((int)s.l[i], safe_base + 1, 64);
        REEF_SET_BOUND(digest, 2.0);
        fe in = fe_zero();
        REEF_SET_BOUND(in, 1.0);
        if (live) {
            fe256 opp_raw = fe256_of_u64(0);
            if (elem == 1 || elem == 2 || elem == 4) opp_raw = load_fe256(opposite + j * levels + h);
            in = merkle_path_input<F>(elem, h, q, sym, oidx, opp_raw, is_mont, digest, tag_leaf, tag_node);
        }
        s = poseidon_permute_spread<F>(in, safe_elem, safe_base, lane, p, L);
    }
    if (live && elem == 1) {
        const fe256 got = fe_to_table<F>(s), want = load_fe256(root);
        u32 diff = 0;
#pragma unroll
        for (int w = 0; w < 8; ++w) diff |= got.w[w] ^ want.w[w];
        accept[j] = diff == 0 ? 1u : 0u;
    }
}
// The same check with a thread per path, for more paths than fill the chip five lanes at a time (as the tree's wide levels).
template <int F>
__global__ void __launch_bounds__(256) k_pos_paths_wide(const u64 *__restrict__ idx, const u32 *__restrict__ symbols, const u64 *__restrict__ opposite_idx,
                                                       const fe256 *__restrict__ opposite, u64 k, u32 levels, int is_mont, PoseidonDev p, fe256 tag_leaf, fe256 tag_node,
                                                       const fe256 *__restrict__ root, u32 *__restrict__ accept) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= k) return;
    const u64 q = idx[j], oidx = opposite_idx[j];
    const u32 sym = symbols[j];
    fe digest = fe_zero();
    REEF_SET_BOUND(digest, 1.0);
    for (u32 h = 0; h < levels; ++h) {
        const fe256 opp_raw = load_fe256(opposite + j * levels + h);
        fe s[POS_T];
#pragma unroll
        for (int e = 0; e < POS_T; ++e) s[e] = merkle_path_input<F>(e, h, q, sym, oidx, opp_raw, is_mont, digest, tag_leaf, tag_node);
        poseidon_permute<F>(s, p);
        digest = s[1];
    }
    const fe256 got = fe_to_table<F>(digest), want = load_fe256(root);
    u32 diff = 0;
#pragma unroll
    for (int w = 0; w < 8; ++w) diff |= got.w[w] ^ want.w[w];
    accept[j] = diff == 0 ? 1u : 0u;
}

}  // namespace reef
