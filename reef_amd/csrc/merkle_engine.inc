// Host side of the Poseidon Merkle commitment (row N4); included after mle_engine.inc.
namespace reef {

static inline u64 merkle_nodes(u64 n) {   // nodes of all levels for an n-symbol document (merkle_tree.rs:25-80)
    u64 total = 0, m = (n + 1) / 2;
    for (;;) {
        total += m;
        if (m <= 1) break;
        m = (m + 1) / 2;
    }
    return total;
}

// ---- sparse form of the partial rounds: constants derived on the host, once per parameter set (merkle_kernels.inc) ----
template <int F> struct PosSparse {
    std::vector<uint8_t> key;        // rf, rp, is_mont, the caller's round constants and matrix: what the entry was derived from
    std::vector<fe256> consts;       // table form: rc_full[rf*5] | mds[25] | sparse[(rp-1)*10] | last[26]
    bool ok = false;
};
template <int F> static fe pos_canon(const fe &x) { return fe_from_table(fe_to_table<F>(x)); }
template <int F> static fe pos_addc(const fe &a, const fe &b) { return pos_canon<F>(fe_add<F>(a, b)); }
template <int F> static fe pos_subc(const fe &a, const fe &b) { return pos_canon<F>(fe_sub<F, 2>(a, b)); }      // operands canonical
template <int F> static fe pos_mulc(const fe &a, const fe &b) { return pos_canon<F>(fe_mul<F>(a, b)); }
// out = in^-1 for a 4 x 4 matrix of canonical elements (Gauss-Jordan); false when singular
template <int F> static bool pos_inv4(const fe (&in)[4][4], fe (&out)[4][4]) {
    fe a[4][8];
    const fe zero = pos_canon<F>(fe_zero()), one = pos_canon<F>(fe_one<F>());
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) { a[i][j] = in[i][j]; a[i][4 + j] = i == j ? one : zero; }
    for (int col = 0; col < 4; ++col) {
        int piv = -1;
        for (int r = col; r < 4; ++r)
            if (!fe_is_zero<F>(a[r][col])) { piv = r; break; }
        if (piv < 0) return false;
        if (piv != col)
            for (int j = 0; j < 8; ++j) std::swap(a[piv][j], a[col][j]);
        const fe inv = pos_canon<F>(fe_inv<F>(a[col][col]));
        for (int j = 0; j < 8; ++j) a[col][j] = pos_mulc<F>(a[col][j], inv);
        for (int r = 0; r < 4; ++r) {
            if (r == col || fe_is_zero<F>(a[r][col])) continue;
            const fe f = a[r][col];
            for (int j = 0; j < 8; ++j) a[r][j] = pos_subc<F>(a[r][j], pos_mulc<F>(f, a[col][j]));
        }
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) out[i][j] = a[i][4 + j];
    return true;
}
// Fills e.consts from the caller's parameters; e.ok = false when some 4 x 4 block is singular (the dense form is used then).
template <int F> static void pos_derive_sparse(const reef_poseidon_params *pp, bool is_mont, PosSparse<F> &e) {
    const u32 rf = pp->full_rounds, rp = pp->partial_rounds, half = rf / 2;
    auto in = [&](const reef_fe &v) {
        fe256 raw;
        memcpy(&raw, &v, sizeof raw);
        return pos_canon<F>(fe_from_caller<F>(raw, is_mont));
    };
    fe M[POS_T][POS_T];
    for (int i = 0; i < POS_T; ++i)
        for (int j = 0; j < POS_T; ++j) M[i][j] = in(pp->mds[i * POS_T + j]);
    e.consts.assign((size_t)rf * POS_T + POS_T * POS_T + (rp > 1 ? (size_t)(rp - 1) * 10 : 0) + 26, fe256{});
    fe256 *rc_full = e.consts.data(), *mds = rc_full + (size_t)rf * POS_T, *sp = mds + POS_T * POS_T, *last = sp + (rp > 1 ? (size_t)(rp - 1) * 10 : 0);
    for (u32 r = 0; r < half; ++r)
        for (int i = 0; i < POS_T; ++i) rc_full[r * POS_T + i] = fe_to_table<F>(in(pp->round_constants[r * POS_T + i]));
    for (int i = 0; i < POS_T * POS_T; ++i) mds[i] = fe_to_table<F>(M[i / POS_T][i % POS_T]);
    const fe zero = pos_canon<F>(fe_zero());
    // (1) constants: element 0 stays in its round, elements 1..4 go through the matrix into the next round
    fe carry[POS_T] = {zero, zero, zero, zero, zero};
    std::vector<fe> c0(rp, zero);
    for (u32 k = 0; k < rp; ++k) {
        fe c[POS_T];
        for (int i = 0; i < POS_T; ++i) c[i] = pos_addc<F>(in(pp->round_constants[(half + k) * POS_T + i]), carry[i]);
        c0[k] = c[0];
        for (int j = 0; j < POS_T; ++j) {
            fe acc = zero;
            for (int i = 1; i < POS_T; ++i) acc = pos_addc<F>(acc, pos_mulc<F>(c[i], M[i][j]));
            carry[j] = acc;
        }
    }
    for (u32 r = half; r < rf; ++r)
        for (int i = 0; i < POS_T; ++i) {
            fe v = in(pp->round_constants[(rp + r) * POS_T + i]);
            if (r == half) v = pos_addc<F>(v, carry[i]);
            rc_full[r * POS_T + i] = fe_to_table<F>(v);
        }
    // (2) matrices: M_k = S_k * D_k, M_{k+1} = D_k * M
    fe Mk[POS_T][POS_T];
    for (int i = 0; i < POS_T; ++i)
        for (int j = 0; j < POS_T; ++j) Mk[i][j] = M[i][j];
    e.ok = true;
    for (u32 k = 0; k + 1 < rp; ++k) {
        fe D[4][4], Di[4][4];
        for (int i = 0; i < 4; ++i)
            for (int j = 0; j < 4; ++j) D[i][j] = Mk[1 + i][1 + j];
        if (!pos_inv4<F>(D, Di)) { e.ok = false; return; }
        fe256 *o = sp + (size_t)k * 10;
        o[0] = fe_to_table<F>(c0[k]);
        o[1] = fe_to_table<F>(Mk[0][0]);                                             // a
        for (int j = 0; j < 4; ++j) {                                                // v = Mk[0][1:] * D^-1
            fe acc = zero;
            for (int l = 0; l < 4; ++l) acc = pos_addc<F>(acc, pos_mulc<F>(Mk[0][1 + l], Di[l][j]));
            o[2 + j] = fe_to_table<F>(acc);
        }
        for (int i = 0; i < 4; ++i) o[6 + i] = fe_to_table<F>(Mk[1 + i][0]);        // w
        fe Nx[POS_T][POS_T];                                                         // D_k * M: row 0 of M as it is, rows 1..4 mixed by D^
        for (int j = 0; j < POS_T; ++j) {
            Nx[0][j] = M[0][j];
            for (int i = 0; i < 4; ++i) {
                fe acc = zero;
                for (int l = 0; l < 4; ++l) acc = pos_addc<F>(acc, pos_mulc<F>(D[i][l], M[1 + l][j]));
                Nx[1 + i][j] = acc;
            }
        }
        for (int i = 0; i < POS_T; ++i)
            for (int j = 0; j < POS_T; ++j) Mk[i][j] = Nx[i][j];
    }
    if (rp) {
        last[0] = fe_to_table<F>(c0[rp - 1]);
        for (int i = 0; i < POS_T * POS_T; ++i) last[1 + i] = fe_to_table<F>(Mk[i / POS_T][i % POS_T]);
    }
}

// ---- what reef_merkle_commit and the resident tree (merkle_resident_engine.inc) share: the argument checks, the constants on the
// device, the kernels of the levels ----
static reef_status merkle_check_params(const reef_poseidon_params *pp) {
    if (pp->width != POS_T) { set_error("Poseidon width %u: only width 5 (arity 4, Reef's U4) is built", pp->width); return REEF_ERR_ARG; }
    if (pp->full_rounds == 0 || (pp->full_rounds & 1) || pp->full_rounds > 64 || pp->partial_rounds > 1024) { set_error("bad round numbers"); return REEF_ERR_ARG; }
    return REEF_OK;
}
static std::vector<u64> merkle_level_sizes(u64 n) {   // node counts of the levels of an n-symbol document, level 0 first
    std::vector<u64> sizes;
    u64 m = (n + 1) / 2;
    sizes.push_back(m);
    while (m > 1) { m = (m + 1) / 2; sizes.push_back(m); }
    return sizes;
}
template <int F> struct PosSetup {
    PoseidonDev pd{};
    fe256 tags[2];          // leaf, node: internal form, handed to the kernels by value
    bool sparse = false;
};
// The permutation's constants on the device, in table form; alloc(which, void **, bytes) gives the two device buffers: 0 the constants, 1 a
// staging one of at least two elements that the caller may reuse once this has returned.  Waits for `s`.
template <int F, class Alloc>
static reef_status pos_setup(hipStream_t s, const reef_poseidon_params *pp, bool is_mont, Alloc &&alloc, PosSetup<F> &out) {
    const u32 rf = pp->full_rounds, rp = pp->partial_rounds;
    const u32 nrc = POS_T * (rf + rp), nmat = POS_T * POS_T;
    // Sparse partial rounds: constants derived once per parameter set on the host (a few ms), then looked up by the caller's
    // bytes.  REEF_POSEIDON_DENSE=1, or a singular block, keeps the permutation in its defining dense form.
    static std::mutex sp_mu;
    static PosSparse<F> sp_entry;
    static const bool force_dense = [] { const char *e = exp_env("REEF_POSEIDON_DENSE"); return e && atoi(e) != 0; }();
    std::vector<fe256> sparse_consts;
    if (!force_dense && rp >= 1) {
        std::vector<uint8_t> key(12 + (size_t)(nrc + nmat) * sizeof(fe256));
        const u32 hdr[3] = {rf, rp, is_mont ? 1u : 0u};
        memcpy(key.data(), hdr, 12);
        memcpy(key.data() + 12, pp->round_constants, (size_t)nrc * sizeof(fe256));
        memcpy(key.data() + 12 + (size_t)nrc * sizeof(fe256), pp->mds, (size_t)nmat * sizeof(fe256));
        std::lock_guard<std::mutex> lk(sp_mu);
        if (sp_entry.key != key) {
            pos_derive_sparse<F>(pp, is_mont, sp_entry);
            sp_entry.key = std::move(key);
        }
        if (sp_entry.ok) sparse_consts = sp_entry.consts;
    }
    const bool sparse = !sparse_consts.empty();
    void *raw = nullptr, *cst = nullptr;
    PoseidonDev pd{};
    pd.rf = rf; pd.rp = rp;
    const fe256 *d_tags = nullptr;
    if (sparse) {                                   // table form already: rc_full | mds | sparse | last, then the two tags through the import kernel
        const size_t nsp = sparse_consts.size();
        REEF_TRY(alloc(0, &cst, (nsp + 2) * sizeof(fe256)));
        REEF_TRY(alloc(1, &raw, 2 * sizeof(fe256)));
        fe256 tg[2];
        memcpy(&tg[0], &pp->tag_leaf, sizeof(fe256));
        memcpy(&tg[1], &pp->tag_node, sizeof(fe256));
        REEF_HIP_TRY(hipMemcpyAsync(cst, sparse_consts.data(), nsp * sizeof(fe256), hipMemcpyHostToDevice, s));
        REEF_HIP_TRY(hipMemcpyAsync(raw, tg, sizeof tg, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_fe_import<F>, dim3(1), dim3(256), 0, s, (const fe256 *)raw, 2u, (int)is_mont, (fe256 *)cst + nsp);
        REEF_HIP_TRY(hipStreamSynchronize(s));      // sparse_consts and tg leave scope below; the kernels read device copies
        pd.rc = (const fe256 *)cst;
        pd.mds = pd.rc + (size_t)rf * POS_T;
        const fe256 *sp = pd.mds + nmat;
        pd.last = sp + (rp > 1 ? (size_t)(rp - 1) * 10 : 0);
        pd.sparse = rp > 1 ? sp : pd.last;          // non-null selects the sparse form
        d_tags = (const fe256 *)cst + nsp;
    } else {
        const u32 nconst = nrc + nmat + 2;
        std::vector<fe256> hc(nconst);
        memcpy(hc.data(), pp->round_constants, nrc * sizeof(fe256));
        memcpy(hc.data() + nrc, pp->mds, nmat * sizeof(fe256));
        memcpy(hc.data() + nrc + nmat, &pp->tag_leaf, sizeof(fe256));
        memcpy(hc.data() + nrc + nmat + 1, &pp->tag_node, sizeof(fe256));
        REEF_TRY(alloc(1, &raw, nconst * sizeof(fe256)));
        REEF_TRY(alloc(0, &cst, nconst * sizeof(fe256)));
        REEF_HIP_TRY(hipMemcpyAsync(raw, hc.data(), nconst * sizeof(fe256), hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(k_fe_import<F>, dim3(ceil_div(nconst, 256)), dim3(256), 0, s, (const fe256 *)raw, nconst, (int)is_mont, (fe256 *)cst);
        REEF_HIP_TRY(hipStreamSynchronize(s));      // hc leaves scope
        pd.rc = (const fe256 *)cst;
        pd.mds = pd.rc + nrc;
        d_tags = pd.mds + nmat;
    }
    REEF_HIP_TRY(hipMemcpyAsync(out.tags, d_tags, 2 * sizeof(fe256), hipMemcpyDeviceToHost, s));
    REEF_HIP_TRY(hipStreamSynchronize(s));                              // the tags go to the kernels by value (internal form)
    out.pd = pd;
    out.sparse = sparse;
    return REEF_OK;
}
// levels that do not fill the chip are latency chains of one hash: five lanes per hash there (merkle_kernels.inc);
// REEF_POSEIDON_SPREAD=0 keeps a thread per node everywhere
template <int F> static bool pos_spread_form(const PosSetup<F> &ps, u64 nodes) {
    static const bool spread_on = !(exp_env("REEF_POSEIDON_SPREAD") && atoi(exp_env("REEF_POSEIDON_SPREAD")) == 0);
    static const u64 spread_max = [] { const char *e = exp_env("REEF_POSEIDON_SPREAD_MAX"); return e ? (u64)strtoull(e, nullptr, 10) : (u64)POS_SPREAD_MAX_NODES; }();
    return spread_on && ps.sparse && nodes <= spread_max;
}
// Enqueues the levels sizes[0..] into `tree`, level 0 first, from the n symbols of d_doc (a slice that starts at symbol index_base) -- or,
// d_doc == nullptr, from a level 0 that is in place already.
template <int F>
static void merkle_hash_levels(hipStream_t s, const u32 *d_doc, u64 n, u64 index_base, const std::vector<u64> &sizes, const PosSetup<F> &ps, fe256 *tree) {
    fe256 *lvl = tree;
    u64 m = sizes[0];
    const PoseidonDev &pd = ps.pd;
    if (!d_doc) {}
    else if (pos_spread_form<F>(ps, m))
        hipLaunchKernelGGL((k_pos_spread<F, true>), dim3((u32)ceil_div(m, POS_SPREAD_PER_WAVE)), dim3(64), 0, s, d_doc, (const fe256 *)nullptr, (u64)n, index_base, pd, ps.tags[0], lvl);
    else
        hipLaunchKernelGGL(k_pos_leaves<F>, dim3((u32)ceil_div(m, 256)), dim3(256), 0, s, d_doc, (u64)n, index_base, pd, ps.tags[0], lvl);
    for (size_t h = 1; h < sizes.size(); ++h) {
        const u64 up = sizes[h];
        if (pos_spread_form<F>(ps, up))
            hipLaunchKernelGGL((k_pos_spread<F, false>), dim3((u32)ceil_div(up, POS_SPREAD_PER_WAVE)), dim3(64), 0, s, (const u32 *)nullptr, (const fe256 *)lvl, m, (u64)0, pd,
                               ps.tags[1], lvl + m);
        else
            hipLaunchKernelGGL(k_pos_nodes<F>, dim3((u32)ceil_div(up, 256)), dim3(256), 0, s, (const fe256 *)lvl, m, pd, ps.tags[1], lvl + m);
        lvl += m;
        m = up;
    }
}

template <int C>
static reef_status v_merkle_commit(const reef_poseidon_params *pp, const uint32_t *doc, size_t n, int doc_loc, bool is_mont, reef_fe *tree_out,
                                   int out_loc, reef_fe *root_out, const MerkleSlice *sl) {
    constexpr int F = 1 - C;
    const bool from_nodes = sl && sl->nodes_in;
    if (from_nodes) n = 2 * sl->nodes_n;               // as many bottom nodes as a document of this length has
    if (!pp || !pp->round_constants || !pp->mds || (n && !doc && !from_nodes) || (!tree_out && !root_out && !sl)) { set_error("null argument"); return REEF_ERR_ARG; }
    if (sl && (sl->index_base & 1)) { set_error("a block of the tree starts at an even symbol"); return REEF_ERR_ARG; }
    REEF_TRY(merkle_check_params(pp));
    if (n == 0 || n >= (1ull << 33)) { set_error("document length out of range"); return REEF_ERR_ARG; }
    ScratchStream ss;
    REEF_TRY(ss.init());
    PosSetup<F> ps;
    REEF_TRY(pos_setup<F>(ss.s, pp, is_mont, [&](int, void **p, size_t bytes) { return ss.alloc(p, bytes); }, ps));
    // node counts: the whole tree stops at one node; a block runs the levels it was told to (a ragged last block carries its single node on)
    std::vector<u64> sizes;
    if (sl) {
        u64 m_ = (n + 1) / 2;
        sizes.push_back(m_);
        for (u32 h = 0; h < sl->levels; ++h) { m_ = (m_ + 1) / 2; sizes.push_back(m_); }
    } else sizes = merkle_level_sizes(n);
    u64 total = 0;
    for (u64 v : sizes) total += v;
    const u32 *d_doc = nullptr;
    void *tree = nullptr;
    if (!from_nodes) REEF_TRY(stage_in<u32>(ss, &d_doc, doc, n, doc_loc));
    REEF_TRY(ss.alloc(&tree, total * sizeof(fe256)));
    if (from_nodes) {
        const u64 m = sizes[0];
        void *nraw = nullptr;
        REEF_TRY(ss.alloc(&nraw, m * sizeof(fe256)));
        REEF_HIP_TRY(hipMemcpyAsync(nraw, sl->nodes_in, m * sizeof(fe256), hipMemcpyHostToDevice, ss.s));
        hipLaunchKernelGGL(k_fe_import<F>, dim3((u32)ceil_div(m, 256)), dim3(256), 0, ss.s, (const fe256 *)nraw, (u32)m, (int)is_mont, (fe256 *)tree);
    }
    merkle_hash_levels<F>(ss.s, from_nodes ? nullptr : d_doc, n, sl ? sl->index_base : 0, sizes, ps, (fe256 *)tree);
    REEF_HIP_TRY(hipGetLastError());
    // export: the whole tree (level by level, leaves' parents first) and / or the root, in the form the caller's field elements have
    void *exp = nullptr;
    REEF_TRY(ss.alloc(&exp, total * sizeof(fe256)));
    hipLaunchKernelGGL(k_fe_export<F>, dim3((u32)ceil_div(total, 256)), dim3(256), 0, ss.s, (const fe256 *)tree, total, 0, (int)is_mont, (fe256 *)exp);
    if (tree_out) {
        REEF_HIP_TRY(hipMemcpyAsync(tree_out, exp, total * sizeof(fe256), out_loc == REEF_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ss.s));
    }
    if (root_out) REEF_HIP_TRY(hipMemcpyAsync(root_out, (fe256 *)exp + (total - 1), sizeof(fe256), hipMemcpyDeviceToHost, ss.s));
    if (sl) {                                                           // a block: every level to its place in the caller's tree
        u64 off = 0;
        for (size_t h = 0; h < sizes.size(); ++h) {
            if (sl->level_out && sl->level_out[h])
                REEF_HIP_TRY(hipMemcpyAsync(sl->level_out[h], (fe256 *)exp + off, sizes[h] * sizeof(fe256), hipMemcpyDeviceToHost, ss.s));
            if (h + 1 == sizes.size() && sl->top_out) REEF_HIP_TRY(hipMemcpyAsync(sl->top_out, (fe256 *)exp + off, sizeof(fe256), hipMemcpyDeviceToHost, ss.s));
            off += sizes[h];
        }
    }
    REEF_HIP_TRY(hipStreamSynchronize(ss.s));
    return REEF_OK;
}

}  // namespace reef
