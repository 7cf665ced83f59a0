// C++ host-side mirror of the nova-snark provider interface as eniac/Reef calls it, over the C ABI
// of include/reef_msm.h (header only).  Reef is Rust; this image has no Rust toolchain, so the host
// side above the ABI is written in C++ with the reference's names and argument meaning:
//
//   CommitmentGens<CURVE>::commit(v, blind)       CE::commit(&gens, &v, &blind)          src/backend/commitment.rs:349-351,360-361,422,430
//   CommitmentGens<CURVE>::fold(w1, w2)           CommitmentGens::fold (ipa_pc)          reached from src/backend/framework.rs:695
//   CommitmentGens<CURVE>::ipa_cross_terms(..)    the two cross-term commitments of an IPA round, without folding the generators
//   CommitmentGens<CURVE>::commit_folded(..)      any commitment over folded generators (a slice of them), folds recorded not performed
//   HyraxPC<CURVE>::commit / commit_symbols       HyraxPC::commit(&poly)                 src/backend/commitment.rs:187
//   HyraxPC<CURVE>::bind_rows                     first step of HyraxPC::prove_eval      src/backend/commitment.rs:371-391 (and :357)
//   CommitmentGensOnDevices<CURVE>                the same key on several GPUs of this process (device groups, reef_msm.h section 5):
//       ::commit / ::commit_rows / ::commit_symbols   CE::commit split by Pippenger window over the devices, HyraxPC::commit rows dealt out whole
//   SumCheck                                      gen_eq_table / linear_mle_product      src/backend/r1cs_helper.rs:441-544, driven as in r1cs.rs:2318-2385
//   compress()                                    Commitment::compress                   src/backend/commitment.rs:195,351,365
//   decompress()                                  CompressedCommitment::decompress [R]   src/backend/commitment.rs:192-197 (a batch per call)
//   char_map() / doc_transform()                  doc_transform(&ab, &doc) [R] from the file's bytes      src/backend/framework.rs:978-1011, config.rs:216-284
//   CommitmentGens<CURVE>(label, n, params [, h]) CommitmentGens::new(label, n) / new_with_blinding_gen      src/backend/framework.rs:297-303, commitment.rs:146-149,176-180
//   MerkleCommitment<CURVE>(doc, pc)              MerkleCommitment::new(&doc, &pc), path_wits, make_wits     src/backend/merkle_tree.rs:25-190
//   MerkleCommitmentResident<CURVE>(doc, pc)      the same with the tree kept on the device: make_wits from it, check_paths  src/backend/merkle_tree.rs:116-256
//   Nifs<CURVE>                                   NIFS::prove's vector work (row N6)     RecursiveSNARK::prove_step, framework.rs:668-675
//   RelaxedR1CSSnark<CURVE>                       RelaxedR1CSSNARK::prove: sum-checks + EE::prove_batch      CompressedSNARK::prove, framework.rs:695-698
//   HyraxEval<CURVE>                              HyraxPC::prove_eval on a resident document                 src/backend/commitment.rs:287-405
// The last three keep the call order of INTEGRATION.md 2f-2i; the transcript is the caller's (a callback), as are the point
// operations on commitments (comm_a, q = gens_s.scale(r)).
//
// Error behaviour: Reef treats every failure as a panic (framework.rs:683,702); here every failed
// call throws reef_provider::Error carrying reef_last_error().
#pragma once
#include <algorithm>
#include <array>
#include <cstring>
#include <functional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "reef_msm.h"

namespace reef_provider {

struct Error : std::runtime_error {
    reef_status status;
    Error(reef_status s, const char *what_failed) : std::runtime_error(std::string(what_failed) + ": " + reef_last_error()), status(s) {}
};
inline void check(reef_status s, const char *what) {
    if (s != REEF_OK) throw Error(s, what);
}

using Compressed = std::array<uint8_t, 32>;

template <int CURVE> inline Compressed compress(const reef_jacobian &p) {
    Compressed c;
    check(reef_normalize(CURVE, &p, 1, REEF_HOST, nullptr, c.data()), "reef_normalize");
    return c;
}

// n encodings (host) -> affine points; throws on the first encoding that is no point, as the reference's unwrap() panics
template <int CURVE> inline std::vector<reef_affine> decompress(const Compressed *c, size_t n) {
    std::vector<reef_affine> out(n);
    uint64_t bad = 0, first = 0;
    check(reef_decompress(CURVE, n ? c->data() : nullptr, n, REEF_HOST, out.data(), &bad, &first), "reef_decompress");
    if (bad) throw std::invalid_argument("reef_decompress: encoding " + std::to_string(first) + " is not a point (" + std::to_string(bad) + " invalid)");
    return out;
}

// The map reef_doc_transform takes, indexed by code point (REEF_DOC_BYTES: by byte value), with doc_transform's rules [R]
// (src/backend/framework.rs:978-986): a character's symbol is its position in `alphabet`, a later duplicate overriding an earlier one; 0x1A
// gives alphabet.size() + 2 (EOF is inserted last and overrides the alphabet's own entry); everything else is REEF_DOC_BAD.  `remap`: the
// characters a transform rewrites before the lookup (CaseInsensitive: {'a', 'A'}) take the entry of what they become; `drop`: the characters
// a transform filters out (IgnoreWhitespace) are REEF_DOC_DROP, whatever else is said about them.  Pure host logic (host/doc_map_selftest.cpp).
inline std::vector<uint32_t> char_map(const std::u32string &alphabet, const std::vector<std::pair<char32_t, char32_t>> &remap = {},
                                      const std::u32string &drop = {}) {
    char32_t top = 0x1A;
    for (char32_t c : alphabet) top = std::max(top, c);
    for (const auto &r : remap) top = std::max(top, std::max(r.first, r.second));
    for (char32_t c : drop) top = std::max(top, c);
    std::vector<uint32_t> m((size_t)top + 1, REEF_DOC_BAD);
    for (size_t i = 0; i < alphabet.size(); ++i) m[alphabet[i]] = (uint32_t)i;
    m[0x1A] = (uint32_t)alphabet.size() + 2;
    std::vector<uint32_t> becomes(remap.size());
    for (size_t i = 0; i < remap.size(); ++i) becomes[i] = m[remap[i].second];
    for (size_t i = 0; i < remap.size(); ++i) m[remap[i].first] = becomes[i];
    for (char32_t c : drop) m[c] = REEF_DOC_DROP;
    return m;
}

// doc_transform(&ab, &doc) [R] (framework.rs:978-1011) from the file's bytes: the document's symbols, EOF, EPSILON and zeros up to a power of
// two, elem_bytes wide, written to `out` (out_cap elements at out_loc: device memory for reef_hyrax_create / reef_merkle_create / the
// SYMBOLS part of reef_sc_set_table_parts).  `map`: char_map(ab, ...); alphabet_len: ab's length.  Returns what the call found; throws
// where the reference panics (a character outside the alphabet, text that is not UTF-8).  out == nullptr measures only.
inline reef_doc_info doc_transform(const uint8_t *doc, size_t nbytes, int doc_loc, int encoding, const std::vector<uint32_t> &map, size_t alphabet_len,
                                   void *out, uint32_t elem_bytes, size_t out_cap, int out_loc) {
    reef_doc_info info = {};
    check(reef_doc_transform(doc, nbytes, doc_loc, encoding, map.empty() ? nullptr : map.data(), map.size(), (uint32_t)alphabet_len + 2,
                             (uint32_t)alphabet_len + 1, out, elem_bytes, out_cap, out_loc, &info), "reef_doc_transform");
    if (info.malformed_at < nbytes) throw std::invalid_argument("doc_transform: the document is not UTF-8 (valid up to byte " + std::to_string(info.malformed_at) + ")");
    if (info.bad) throw std::invalid_argument("doc_transform: Character in document that's not in alphabet (byte " + std::to_string(info.first_bad) + ", " + std::to_string(info.bad) + " in all)");
    return info;
}
// the same to host memory under the reference's signature: the Vec<usize> it returns
inline std::vector<size_t> doc_transform(const std::u32string &ab, const std::vector<uint8_t> &doc, int encoding = REEF_DOC_BYTES) {
    const std::vector<uint32_t> map = char_map(ab);
    size_t cap = 2;
    while (cap < doc.size() + 2) cap <<= 1;
    std::vector<uint32_t> sym(cap);
    const reef_doc_info info = doc_transform(doc.data(), doc.size(), REEF_HOST, encoding, map, ab.size(), sym.data(), 4, cap, REEF_HOST);
    return std::vector<size_t>(sym.begin(), sym.begin() + info.padded);
}

// nova-snark CommitmentGens<G>: a vector of generators (+ blinding generator h) resident on the GPU,
// pre-shifted once (commitment keys are fixed for the life of PublicParams, framework.rs:45,297-303).
template <int CURVE> class CommitmentGens {
  public:
    CommitmentGens(const reef_affine *gens, size_t n, int gens_loc = REEF_HOST, const reef_affine *h = nullptr, bool preshift = true)
        : n_(n), has_h_(h != nullptr) {
        reef_msm_opts o = {};
        o.bucket_groups = preshift ? 1 : 0;
        o.device = -1;
        check(reef_msm_ctx_create(&ctx_, CURVE, gens, n, gens_loc, &o), "reef_msm_ctx_create");
        if (h) h_ = *h;
    }
    // CommitmentGens::new(label, n) [R] / the fork's new_with_blinding_gen(label, n, &h): the n generators are derived from the label on the GPU
    // (row N1: reef_derive_generators) straight into the resident key -- they never visit the host.  pasta_curves' hash-to-curve constants are
    // the caller's (`kp`: canonical integers of the base field unless kp_is_mont).
    CommitmentGens(const std::string &label, size_t n, const reef_keygen_params &kp, const reef_affine *h = nullptr, bool kp_is_mont = false, bool preshift = true)
        : n_(n), has_h_(h != nullptr) {
        reef_affine *dev = (reef_affine *)reef_device_alloc(n * sizeof(reef_affine));
        if (!dev) throw Error(REEF_ERR_OOM, "reef_device_alloc");
        reef_status st = reef_derive_generators(CURVE, (const uint8_t *)label.data(), label.size(), n, &kp, kp_is_mont, dev, REEF_DEVICE);
        if (st == REEF_OK) {
            reef_msm_opts o = {};
            o.bucket_groups = preshift ? 1 : 0;
            o.device = -1;
            st = reef_msm_ctx_create(&ctx_, CURVE, dev, n, REEF_DEVICE, &o);
        }
        reef_device_free(dev);
        check(st, "CommitmentGens::new(label, n)");
        if (h) h_ = *h;
    }
    // the same generators on the host (what from_label returns to a caller that keeps them itself)
    static std::vector<reef_affine> from_label(const std::string &label, size_t n, const reef_keygen_params &kp, bool kp_is_mont = false) {
        std::vector<reef_affine> out(n);
        check(reef_derive_generators(CURVE, (const uint8_t *)label.data(), label.size(), n, &kp, kp_is_mont, out.data(), REEF_HOST), "reef_derive_generators");
        return out;
    }
    ~CommitmentGens() { reef_msm_ctx_destroy(ctx_); }
    CommitmentGens(const CommitmentGens &) = delete;
    CommitmentGens &operator=(const CommitmentGens &) = delete;

    size_t len() const { return n_; }
    reef_msm_ctx *handle() const { return ctx_; }
    const reef_affine *h() const { return has_h_ ? &h_ : nullptr; }

    // CE::commit: sum v_i G_i (+ blind * h).  Scalars in the pasta ABI form (Montgomery), host or device.
    reef_jacobian commit(const reef_fe *v, size_t n, const reef_fe *blind = nullptr, int v_loc = REEF_HOST) const {
        reef_jacobian out;
        if (blind) {
            if (!has_h_) throw std::logic_error("commit with a blind needs the blinding generator");
            if (v_loc != REEF_HOST) throw std::logic_error("blind and h live where the scalars live: host");
            check(reef_msm_rows(ctx_, v, 1, n, REEF_HOST, true, 0, blind, &h_, &out, REEF_HOST), "reef_msm_rows");
        } else {
            check(reef_msm(ctx_, v, n, v_loc, true, &out, REEF_HOST), "reef_msm");
        }
        return out;
    }

    // CommitmentGens::fold(w1, w2): G'_i = w1 * G_i + w2 * G_{i + n/2}; w canonical little-endian.
    static std::vector<reef_affine> fold(const reef_affine *gens, size_t n, const reef_fe &w1, const reef_fe &w2) {
        std::vector<reef_affine> out(n / 2);
        check(reef_fold(CURVE, gens, n / 2, REEF_HOST, &w1, &w2, out.data()), "reef_fold");
        return out;
    }

    // Cross terms (L, R) of IPA round k = w1s.size() over THESE generators (no fold): a = a_lo || a_hi.
    // CE::commit over the generators w1s.size() folds away from this key, slice [off, off + len), without folding them
    // (reef_msm_folded): what a CommitmentGens that records its folds returns from commit / split_at().commit
    reef_jacobian commit_folded(const reef_fe *v, size_t len, size_t off, const std::vector<reef_fe> &w1s, const std::vector<reef_fe> &w2s,
                                int v_loc = REEF_HOST) const {
        if (w1s.size() != w2s.size()) throw std::invalid_argument("challenge vectors differ in length");
        reef_jacobian out;
        check(reef_msm_folded(ctx_, v, len, off, v_loc, true, w1s.data(), w2s.data(), w1s.size(), &out, REEF_HOST), "reef_msm_folded");
        return out;
    }
    // K3, deep: the len() / 2^k generators k = w1s.size() folds away from this key, in one pass (reef_fold_deep); w canonical
    std::vector<reef_affine> fold_deep(const std::vector<reef_fe> &w1s, const std::vector<reef_fe> &w2s) const {
        if (w1s.size() != w2s.size()) throw std::invalid_argument("challenge vectors differ in length");
        std::vector<reef_affine> out(n_ >> w1s.size());
        check(reef_fold_deep(ctx_, w1s.data(), w2s.data(), w1s.size(), out.data(), REEF_HOST), "reef_fold_deep");
        return out;
    }
    std::pair<reef_jacobian, reef_jacobian> ipa_cross_terms(const reef_fe *a, size_t n_k, const std::vector<reef_fe> &w1s,
                                                            const std::vector<reef_fe> &w2s, int a_loc = REEF_HOST) const {
        if (w1s.size() != w2s.size()) throw std::logic_error("one (w1, w2) pair per round");
        std::pair<reef_jacobian, reef_jacobian> lr;
        check(reef_ipa_cross_terms(ctx_, a, n_k, a_loc, true, w1s.data(), w2s.data(), w1s.size(), &lr.first, &lr.second), "reef_ipa_cross_terms");
        return lr;
    }

  private:
    reef_msm_ctx *ctx_ = nullptr;
    size_t n_;
    reef_affine h_ = {};
    bool has_h_;
};

// `gens.fold(w1, w2)` that records the folds instead of performing them (reef_amd/provider.py FoldedGens): commit() is one MSM over the
// root's resident key (reef_msm_folded); materialize() makes the folded generators a resident key of their own, in one deep fold on the
// device (reef_msm_ctx_create_folded; with bucket_groups = 1 and at most 1024 points it has nibble tables).  The caller destroys it.
template <int CURVE> struct FoldedGens {
    const CommitmentGens<CURVE> &root;
    std::vector<reef_fe> w1s, w2s;       // canonical little-endian, one pair per fold
    size_t len() const { return root.len() >> w1s.size(); }
    FoldedGens fold(const reef_fe &w1, const reef_fe &w2) const {
        FoldedGens f{root, w1s, w2s};
        f.w1s.push_back(w1);
        f.w2s.push_back(w2);
        return f;
    }
    reef_jacobian commit(const reef_fe *v, size_t n, size_t off = 0) const { return root.commit_folded(v, n, off, w1s, w2s); }
    reef_msm_ctx *materialize(uint32_t bucket_groups = 1) const {
        reef_msm_opts o = {};
        o.bucket_groups = bucket_groups;
        o.device = -1;
        reef_msm_ctx *out = nullptr;
        check(reef_msm_ctx_create_folded(&out, root.handle(), w1s.data(), w2s.data(), w1s.size(), &o), "reef_msm_ctx_create_folded");
        return out;
    }
};

// The same commitment key kept on several GPUs of ONE process -- Reef's prover is one process (src/backend/main.rs:82) -- through the
// library's device groups: CE::commit is split by Pippenger window over the devices (the 96-byte partial sums are exchanged and added
// inside the library), the rows of HyraxPC::commit are dealt out whole.  `devices` may repeat an ordinal.
template <int CURVE> class CommitmentGensOnDevices {
  public:
    // scalars: how the caller's host scalars reach the members of a windows group -- every member uploads them over its own PCIe link (REEF_SCALARS_EACH),
    // or one upload to devices[0] and peer copies from there (REEF_SCALARS_FANOUT); which wins depends on the host's topology (reef_msm.h section 5)
    CommitmentGensOnDevices(const reef_affine *gens, size_t n, const std::vector<int> &devices, const reef_affine *h = nullptr, uint32_t split = REEF_SPLIT_WINDOWS,
                            uint32_t scalars = REEF_SCALARS_EACH)
        : n_(n), has_h_(h != nullptr) {
        reef_msm_opts o = {};
        o.bucket_groups = 1;
        reef_msm_group_opts g = {};
        g.split = split;
        g.scalars = scalars;
        check(reef_msm_group_create(&grp_, CURVE, gens, n, REEF_HOST, &o, devices.data(), devices.size(), &g), "reef_msm_group_create");
        if (h) h_ = *h;
    }
    ~CommitmentGensOnDevices() { reef_msm_group_destroy(grp_); }
    CommitmentGensOnDevices(const CommitmentGensOnDevices &) = delete;
    CommitmentGensOnDevices &operator=(const CommitmentGensOnDevices &) = delete;
    size_t len() const { return n_; }
    // where the last commit's time went (distribution of the scalars, every member's stream, the combine): the first run on a real node explains itself
    void enable_timing(bool on) const { check(reef_msm_group_enable_timing(grp_, on ? 1 : 0), "reef_msm_group_enable_timing"); }
    reef_msm_group_timing last_timing() const {
        reef_msm_group_timing t;
        check(reef_msm_group_last_timing(grp_, &t), "reef_msm_group_last_timing");
        return t;
    }

    reef_jacobian commit(const reef_fe *v, size_t n, const reef_fe *blind = nullptr) const {
        reef_jacobian out;
        if (blind) {
            if (!has_h_) throw std::logic_error("commit with a blind needs the blinding generator");
            check(reef_msm_group_rows(grp_, v, 1, n, REEF_HOST, true, 0, blind, &h_, &out), "reef_msm_group_rows");
        } else {
            check(reef_msm_group_msm(grp_, v, n, REEF_HOST, true, &out), "reef_msm_group_msm");
        }
        return out;
    }
    // HyraxPC::commit(&poly) over the devices: rows x row_len field elements / one-byte symbols, one commitment per row
    std::vector<reef_jacobian> commit_rows(const reef_fe *poly, size_t rows, size_t row_len, const reef_fe *blinds, uint32_t max_scalar_bits = 0) const {
        std::vector<reef_jacobian> out(rows);
        check(reef_msm_group_rows(grp_, poly, rows, row_len, REEF_HOST, true, max_scalar_bits, blinds, blinds ? &h_ : nullptr, out.data()), "reef_msm_group_rows");
        return out;
    }
    std::vector<reef_jacobian> commit_symbols(const uint8_t *symbols, size_t rows, size_t row_len, uint32_t symbol_bits, const reef_fe *blinds) const {
        std::vector<reef_jacobian> out(rows);
        check(reef_msm_group_rows_symbols(grp_, symbols, rows, row_len, REEF_HOST, symbol_bits, blinds, blinds ? &h_ : nullptr, true, out.data()),
              "reef_msm_group_rows_symbols");
        return out;
    }

  private:
    reef_msm_group *grp_ = nullptr;
    size_t n_;
    reef_affine h_ = {};
    bool has_h_;
};

// nova-snark (fork) HyraxPC as Reef builds it at commitment.rs:182-185: 2^right row generators and the
// blinding generator; the polynomial's 2^l evaluations are viewed as a 2^left x 2^right matrix.
template <int CURVE> class HyraxPC {
  public:
    explicit HyraxPC(const CommitmentGens<CURVE> &gens_v) : gens_(gens_v) {
        if (!gens_v.h()) throw std::logic_error("HyraxPC needs a blinding generator");
    }
    static std::pair<size_t, size_t> compute_factored_lens(size_t num_vars) { return {num_vars / 2, num_vars - num_vars / 2}; }

    // HyraxPC::commit(&poly): one commitment per matrix row, sum_j Z[i,j] G_j + blinds[i] h.
    std::vector<reef_jacobian> commit(const reef_fe *poly, size_t num_vars, const reef_fe *blinds, uint32_t max_scalar_bits = 0) const {
        const auto lr = compute_factored_lens(num_vars);
        const size_t rows = (size_t)1 << lr.first, row_len = (size_t)1 << lr.second;
        if (row_len > gens_.len()) throw std::logic_error("not enough row generators");
        std::vector<reef_jacobian> out(rows);
        check(reef_msm_rows(gens_.handle(), poly, rows, row_len, REEF_HOST, true, max_scalar_bits, blinds, gens_.h(), out.data(), REEF_HOST),
              "reef_msm_rows");
        return out;
    }
    // The same from the document symbols themselves (one byte each, < 2^symbol_bits; framework.rs:978-1011).
    std::vector<reef_jacobian> commit_symbols(const uint8_t *symbols, size_t num_vars, uint32_t symbol_bits, const reef_fe *blinds,
                                              int symbols_loc = REEF_HOST) const {
        const auto lr = compute_factored_lens(num_vars);
        const size_t rows = (size_t)1 << lr.first, row_len = (size_t)1 << lr.second;
        if (row_len > gens_.len()) throw std::logic_error("not enough row generators");
        std::vector<reef_jacobian> out(rows);
        check(reef_msm_rows_symbols(gens_.handle(), symbols, rows, row_len, symbols_loc, symbol_bits, blinds, blinds ? gens_.h() : nullptr, true,
                                    out.data(), REEF_HOST),
              "reef_msm_rows_symbols");
        return out;
    }
    // The same from 16- or 32-bit symbols (an alphabet of 254 characters or more; reef_msm_rows_symbols_wide).
    std::vector<reef_jacobian> commit_symbols(const uint16_t *symbols, size_t num_vars, uint32_t symbol_bits, const reef_fe *blinds,
                                              int symbols_loc = REEF_HOST) const {
        return commit_symbols_wide(symbols, 2, num_vars, symbol_bits, blinds, symbols_loc);
    }
    std::vector<reef_jacobian> commit_symbols(const uint32_t *symbols, size_t num_vars, uint32_t symbol_bits, const reef_fe *blinds,
                                              int symbols_loc = REEF_HOST) const {
        return commit_symbols_wide(symbols, 4, num_vars, symbol_bits, blinds, symbols_loc);
    }
    std::vector<reef_jacobian> commit_symbols_wide(const void *symbols, uint32_t elem_bytes, size_t num_vars, uint32_t symbol_bits,
                                                   const reef_fe *blinds, int symbols_loc = REEF_HOST) const {
        const auto lr = compute_factored_lens(num_vars);
        const size_t rows = (size_t)1 << lr.first, row_len = (size_t)1 << lr.second;
        if (row_len > gens_.len()) throw std::logic_error("not enough row generators");
        std::vector<reef_jacobian> out(rows);
        check(reef_msm_rows_symbols_wide(gens_.handle(), symbols, elem_bytes, rows, row_len, symbols_loc, symbol_bits, blinds,
                                         blinds ? gens_.h() : nullptr, true, out.data(), REEF_HOST),
              "reef_msm_rows_symbols_wide");
        return out;
    }
    // First step of prove_eval: LZ = L^T Z and eval = <LZ, R> for (L, R) = eq-evaluations of the two halves of `point`.
    struct BoundRows {
        std::vector<reef_fe> lz;
        reef_fe eval;
    };
    BoundRows bind_rows(const void *z, size_t n, int elem_bytes, int z_loc, const reef_fe *point, size_t num_vars, bool is_mont = true) const {
        const auto lr = compute_factored_lens(num_vars);
        BoundRows b;
        b.lz.resize((size_t)1 << lr.second);
        check(reef_mle_bound_rows(CURVE, z, n, elem_bytes, z_loc, is_mont, point, num_vars, lr.first, b.lz.data(), REEF_HOST, &b.eval),
              "reef_mle_bound_rows");
        return b;
    }

  private:
    const CommitmentGens<CURVE> &gens_;
};

// The nlookup sum-check of witness generation (r1cs.rs:2318-2385) over the scalar field of Pallas: resident
// (table, eq) pair, one call per half of linear_mle_product; the Poseidon challenge stays with the caller.
class SumCheck {
  public:
    SumCheck(size_t ell) : ell_(ell) { check(reef_sc_create(&sc_, REEF_PALLAS, (size_t)1 << ell), "reef_sc_create"); }
    ~SumCheck() { reef_sc_destroy(sc_); }
    SumCheck(const SumCheck &) = delete;
    SumCheck &operator=(const SumCheck &) = delete;

    void set_table(const reef_fe *values, size_t n, int loc = REEF_HOST) { have_next_ = false; check(reef_sc_set_table(sc_, 0, values, n, loc), "reef_sc_set_table"); }
    // the table as the runs Reef builds it from -- "nldoc": {SYMBOLS doc}; "nlhybrid": {FE table, FILL calc_fill x (half - |table|), SYMBOLS proj_doc} --
    // zero beyond them: a host symbol part uploads its bytes, not 32 per entry
    void set_table_parts(const std::vector<reef_sc_part> &parts) {
        have_next_ = false;
        check(reef_sc_set_table_parts(sc_, parts.data(), parts.size()), "reef_sc_set_table_parts");
    }
    // T[idx[j]] of the table as last set, whatever has been folded since: the v_i of a step's lookups (r1cs.rs:2066-2077).  Leaves the rounds alone.
    std::vector<reef_fe> lookup(const std::vector<uint64_t> &idx) {
        std::vector<reef_fe> v(idx.size());
        check(reef_sc_lookup(sc_, idx.data(), idx.size(), v.data(), REEF_HOST), "reef_sc_lookup");
        return v;
    }
    void start_step() { have_next_ = false; check(reef_sc_reset_table(sc_), "reef_sc_reset_table"); }   // every folding step starts from the unfolded table
    void gen_eq_table(const std::vector<reef_fe> &rs, const std::vector<uint32_t> &qs, const std::vector<reef_fe> &last_q) {
        if (rs.size() != qs.size() + 1 || last_q.size() != ell_) throw std::logic_error("gen_eq_table: |rs| = |qs| + 1, |last_q| = ell");
        have_next_ = false;
        check(reef_sc_gen_eq_table(sc_, rs.data(), qs.data(), qs.size(), last_q.data(), ell_), "reef_sc_gen_eq_table");
    }
    // round i in 1..ell: (xsq, x, con)
    std::array<reef_fe, 3> round_coeffs(size_t i) {
        std::array<reef_fe, 3> g;
        check(reef_sc_round_coeffs(sc_, (size_t)1 << (ell_ - i), g.data()), "reef_sc_round_coeffs");
        return g;
    }
    void fold(size_t i, const reef_fe &r) { check(reef_sc_fold(sc_, (size_t)1 << (ell_ - i), &r), "reef_sc_fold"); }
    // fold of round i and the coefficients of round i + 1 in one pass (i < ell)
    std::array<reef_fe, 3> fold_and_next_coeffs(size_t i, const reef_fe &r) {
        std::array<reef_fe, 3> g;
        check(reef_sc_fold_and_next_coeffs(sc_, (size_t)1 << (ell_ - i), &r, g.data()), "reef_sc_fold_and_next_coeffs");
        return g;
    }
    // The whole of the reference's linear_mle_product(table_t, table_eq, ell, i, sponge) (r1cs_helper.rs:441-506) on the resident tables: the round's
    // sums, absorb (con, x, xsq) in that order, squeeze the challenge, fold both tables; returns {r_i, xsq, x, con} like the reference.  `transcript`
    // is the caller's sponge: given {con, x, xsq} (canonical) it returns the challenge (neptune's SpongeAPI absorb(3) + squeeze(1) on the Rust side).
    // Driven round after round as r1cs.rs:2318-2385 does, each round is one pass over the tables (the fold of round i yields round i + 1's sums).
    template <class Transcript> std::array<reef_fe, 4> linear_mle_product(size_t i, Transcript &&transcript) {
        const std::array<reef_fe, 3> g = (have_next_ && next_round_ == i) ? next_ : round_coeffs(i);      // {xsq, x, con}
        const std::array<reef_fe, 3> query = {g[2], g[1], g[0]};
        const reef_fe r = transcript(query);
        have_next_ = false;
        if (i < ell_) {
            next_ = fold_and_next_coeffs(i, r);
            next_round_ = i + 1;
            have_next_ = true;
        } else {
            fold(i, r);
        }
        return {r, g[0], g[1], g[2]};
    }
    reef_fe final_value() {   // prover_mle_partial_eval(table, sc_rs) after the last fold (r1cs.rs:2379-2385)
        reef_fe v;
        check(reef_sc_read(sc_, 0, 1, &v), "reef_sc_read");
        return v;
    }

  private:
    reef_sc_ctx *sc_ = nullptr;
    size_t ell_;
    std::array<reef_fe, 3> next_ = {};     // sums of the round after the last linear_mle_product, if that call produced them
    size_t next_round_ = 0;
    bool have_next_ = false;
};

// The reference's MerkleCommitment<F> (src/backend/merkle_tree.rs:11-16): `commitment` (the root), `tree` (the levels, the leaves' parents first)
// and `doc`.  The tree is built on the GPU -- on one device, or in blocks over `devices` (reef_merkle_commit_devices) --; path_wits / make_wits
// (:116-190) are look-ups in it on the host, as in the reference.  The Poseidon constants are the caller's (neptune's, on the Rust side).
struct MerkleWit {
    bool l_or_r;          // true: the node on the path is the LEFT child
    bool has_idx;         // leaf level only (the reference's Option): opposite_idx is the sibling's document index (0 when it is missing)
    uint64_t opposite_idx;
    reef_fe opposite;     // the sibling's value, canonical (zero when it is missing)
};
template <int CURVE> class MerkleCommitment {
  public:
    MerkleCommitment(const std::vector<uint32_t> &document, const reef_poseidon_params &pc, bool pc_is_mont = false, const std::vector<int> &devices = {})
        : doc(document) {
        if (doc.empty()) throw std::invalid_argument("MerkleCommitment::new: empty document");     // the reference indexes an empty level: a panic
        std::vector<reef_fe> flat(reef_merkle_nodes(doc.size()));
        if (devices.empty())
            check(reef_merkle_commit(CURVE, &pc, doc.data(), doc.size(), REEF_HOST, pc_is_mont, flat.data(), REEF_HOST, &commitment), "reef_merkle_commit");
        else
            check(reef_merkle_commit_devices(CURVE, &pc, doc.data(), doc.size(), pc_is_mont, devices.data(), devices.size(), flat.data(), &commitment, nullptr),
                  "reef_merkle_commit_devices");
        size_t m = (doc.size() + 1) / 2, off = 0;
        for (;;) {
            tree.emplace_back(flat.begin() + off, flat.begin() + off + m);
            off += m;
            if (m <= 1) break;
            m = (m + 1) / 2;
        }
    }
    // merkle_tree.rs:128-190
    std::vector<MerkleWit> path_wits(size_t idx) const {
        if (idx >= doc.size()) throw std::out_of_range("path_wits: idx < doc.len()");
        const reef_fe zero = {};
        auto sym = [](uint32_t v) { return reef_fe{{v, 0, 0, 0}}; };
        std::vector<MerkleWit> w;
        if (idx % 2 == 0) {
            if (idx + 1 >= doc.size()) w.push_back({true, true, 0, zero});
            else w.push_back({true, true, idx + 1, sym(doc[idx + 1])});
        } else {
            w.push_back({false, true, idx - 1, sym(doc[idx - 1])});
        }
        size_t quo = idx / 2;
        for (size_t h = 0; h + 1 < tree.size(); ++h) {
            if (quo % 2 == 0) w.push_back({true, false, 0, quo + 1 >= tree[h].size() ? zero : tree[h][quo + 1]});
            else w.push_back({false, false, 0, tree[h][quo - 1]});
            quo /= 2;
        }
        return w;
    }
    // merkle_tree.rs:116-126
    std::vector<std::vector<MerkleWit>> make_wits(const std::vector<size_t> &m_lookups) const {
        std::vector<std::vector<MerkleWit>> wits;
        for (size_t q : m_lookups) wits.push_back(path_wits(q));
        return wits;
    }

    reef_fe commitment = {};
    std::vector<std::vector<reef_fe>> tree;
    std::vector<uint32_t> doc;
};
// The same commitment with the tree KEPT ON THE DEVICE (reef_merkle_create): no `tree` member, no copy of it on the host; make_wits is
// one reef_merkle_open, check_paths hashes claimed openings back to the root on the device.  Field elements cross as canonical integers.
template <int CURVE> class MerkleCommitmentResident {
  public:
    MerkleCommitmentResident(const std::vector<uint32_t> &document, const reef_poseidon_params &pc, int device = 0) {
        if (document.empty()) throw std::invalid_argument("MerkleCommitment::new: empty document");
        check(reef_merkle_create(&ctx_, CURVE, &pc, document.data(), document.size(), REEF_HOST, false, device), "reef_merkle_create");
        uint64_t n = 0;
        uint32_t lv = 0;
        const reef_status s = reef_merkle_info(ctx_, &n, &lv, nullptr, &commitment);
        if (s != REEF_OK) { reef_merkle_destroy(ctx_); check(s, "reef_merkle_info"); }
        len = (size_t)n;
        levels = lv;
    }
    ~MerkleCommitmentResident() { reef_merkle_destroy(ctx_); }
    MerkleCommitmentResident(const MerkleCommitmentResident &) = delete;
    MerkleCommitmentResident &operator=(const MerkleCommitmentResident &) = delete;
    // merkle_tree.rs:116-126; `path` (may be NULL): the digests on the way up, lookups x levels, the root last
    std::vector<std::vector<MerkleWit>> make_wits(const std::vector<size_t> &m_lookups, std::vector<reef_fe> *path = nullptr) const {
        for (size_t q : m_lookups)
            if (q >= len) throw std::out_of_range("path_wits: idx < doc.len()");
        const size_t k = m_lookups.size();
        std::vector<uint64_t> idx(m_lookups.begin(), m_lookups.end()), oidx(k);
        std::vector<reef_fe> opp(k * levels);
        if (path) path->assign(k * levels, reef_fe{});
        check(reef_merkle_open(ctx_, idx.data(), k, nullptr, oidx.data(), opp.data(), path ? path->data() : nullptr), "reef_merkle_open");
        std::vector<std::vector<MerkleWit>> wits(k);
        for (size_t j = 0; j < k; ++j)
            for (uint32_t h = 0; h < levels; ++h) wits[j].push_back({((idx[j] >> h) & 1) == 0, h == 0, h == 0 ? oidx[j] : 0, opp[j * levels + h]});
        return wits;
    }
    std::vector<MerkleWit> path_wits(size_t idx) const { return make_wits({idx})[0]; }
    // accept flags of claimed openings of m_lookups with the claimed symbols (reef_merkle_check_paths)
    std::vector<uint32_t> check_paths(const std::vector<size_t> &m_lookups, const std::vector<uint32_t> &symbols, const std::vector<std::vector<MerkleWit>> &wits) const {
        const size_t k = m_lookups.size();
        if (symbols.size() != k || wits.size() != k) throw std::invalid_argument("check_paths: one symbol and one opening per lookup");
        std::vector<uint64_t> idx(m_lookups.begin(), m_lookups.end()), oidx(k);
        std::vector<reef_fe> opp(k * levels);
        for (size_t j = 0; j < k; ++j) {
            if (wits[j].size() != levels) throw std::invalid_argument("check_paths: an opening has one wit per level");
            oidx[j] = wits[j][0].opposite_idx;
            for (uint32_t h = 0; h < levels; ++h) opp[j * levels + h] = wits[j][h].opposite;
        }
        std::vector<uint32_t> accept(k);
        check(reef_merkle_check_paths(ctx_, idx.data(), symbols.data(), oidx.data(), opp.data(), k, accept.data()), "reef_merkle_check_paths");
        return accept;
    }
    std::vector<uint32_t> symbols(const std::vector<size_t> &m_lookups) const {
        const size_t k = m_lookups.size();
        std::vector<uint64_t> idx(m_lookups.begin(), m_lookups.end());
        std::vector<uint32_t> sym(k);
        std::vector<reef_fe> opp(k * levels);
        check(reef_merkle_open(ctx_, idx.data(), k, sym.data(), nullptr, opp.data(), nullptr), "reef_merkle_open");
        return sym;
    }

    reef_fe commitment = {};
    size_t len = 0;
    uint32_t levels = 0;

  private:
    reef_merkle_ctx *ctx_ = nullptr;
};

// nova's transcript as the rows below see it [R]: absorb `len` bytes under `label`, squeeze the next challenge (below the
// modulus; the form the caller's is_mont names).  The Keccak sponge itself stays with the caller.
using Transcript = std::function<reef_fe(const char *label, const void *bytes, size_t len)>;

inline size_t log2_exact(size_t n) {
    size_t k = 0;
    while (((size_t)1 << k) < n) ++k;
    if (((size_t)1 << k) != n) throw std::invalid_argument("not a power of two");
    return k;
}

// nova-snark NIFS [R] over one resident context per curve and R1CS shape (reef_msm.h 3f).  The running
// instance and T stay on the device; the points comm_W, comm_E of the folded instance stay with the caller.
template <int CURVE> class Nifs {
  public:
    Nifs(size_t num_cons, size_t num_vars, size_t num_io, int device = 0) : num_cons_(num_cons), num_vars_(num_vars), num_io_(num_io) {
        check(reef_nifs_create(&ctx_, CURVE, num_cons, num_vars, num_io, device), "reef_nifs_create");
    }
    ~Nifs() { reef_nifs_destroy(ctx_); }
    Nifs(const Nifs &) = delete;
    Nifs &operator=(const Nifs &) = delete;
    size_t num_cons() const { return num_cons_; }
    size_t num_vars() const { return num_vars_; }
    size_t num_io() const { return num_io_; }
    reef_nifs_ctx *handle() const { return ctx_; }

    // PublicParams::setup: which 0 A, 1 B, 2 C as (row, col, value) triples; duplicates are summed
    void set_matrix(int which, const uint32_t *row, const uint32_t *col, const reef_fe *val, size_t nnz, bool is_mont = true) {
        check(reef_nifs_set_matrix(ctx_, which, row, col, val, nnz, is_mont), "reef_nifs_set_matrix");
    }
    // the running instance; nova's first step passes the first fresh instance with E = NULL (zeros) and u = 1
    void set_running(const reef_fe *W, const reef_fe *E, const reef_fe &u, const reef_fe *X, int loc = REEF_HOST, bool is_mont = true) {
        check(reef_nifs_set_running(ctx_, W, E, &u, X, loc, is_mont), "reef_nifs_set_running");
    }
    // NIFS::prove's commit_T: T of the running and the fresh instance (W2, u = 1, X2) stays on the device; comm_T = MSM(T) over
    // `key` (same curve and device, at least num_cons points), returned to the host for the transcript
    reef_jacobian commit_T(reef_msm_ctx *key, const reef_fe *W2, const reef_fe *X2, int loc = REEF_HOST, bool is_mont = true) {
        reef_jacobian comm_T;
        check(reef_nifs_commit_T(ctx_, key, W2, X2, loc, is_mont, &comm_T), "reef_nifs_commit_T");
        return comm_T;
    }
    // commit_T and CE::commit of the fresh witness from one upload of W2: {comm_W2, comm_T}, both over `key` (at least
    // max(num_cons, num_vars) points), no blinds.  State as after commit_T.
    struct StepCommitments { reef_jacobian comm_W2, comm_T; };
    StepCommitments commit_step(reef_msm_ctx *key, const reef_fe *W2, const reef_fe *X2, int loc = REEF_HOST, bool is_mont = true) {
        StepCommitments o;
        check(reef_nifs_commit_step(ctx_, key, W2, X2, loc, is_mont, &o.comm_W2, &o.comm_T), "reef_nifs_commit_step");
        return o;
    }
    // comm_W and comm_E of the running instance as it stands (either may be NULL); reads only
    void commit_running(reef_msm_ctx *key, reef_jacobian *comm_W, reef_jacobian *comm_E) const {
        check(reef_nifs_commit_running(ctx_, key, comm_W, comm_E), "reef_nifs_commit_running");
    }
    // AZ o BZ == CZ on the fresh instance of the last commit_T / commit_step: the number of rows that fail
    uint64_t check_fresh(uint64_t *first_bad_row = nullptr) const {
        uint64_t bad = 0, first = 0;
        check(reef_nifs_check_fresh(ctx_, &bad, &first), "reef_nifs_check_fresh");
        if (first_bad_row) *first_bad_row = first;
        return bad;
    }
    // W += r W2, E += r T, u += r, X += r X2
    void fold(const reef_fe &r, bool is_mont = true) { check(reef_nifs_fold(ctx_, &r, is_mont), "reef_nifs_fold"); }
    // which: 0 W, 1 E, 2 T, 3 u, 4 X; the first `count` entries
    std::vector<reef_fe> read(int which, size_t count, bool to_mont = true) const {
        std::vector<reef_fe> out(count);
        check(reef_nifs_read(ctx_, which, count, out.data(), to_mont), "reef_nifs_read");
        return out;
    }
    // is_sat_relaxed without the commitment check: the number of rows with AZ o BZ != u CZ + E
    uint64_t check_relaxed(uint64_t *first_bad_row = nullptr) const {
        uint64_t bad = 0, first = 0;
        check(reef_nifs_check_relaxed(ctx_, &bad, &first), "reef_nifs_check_relaxed");
        if (first_bad_row) *first_bad_row = first;
        return bad;
    }

  private:
    reef_nifs_ctx *ctx_ = nullptr;
    size_t num_cons_, num_vars_, num_io_;
};

// nova-snark RelaxedR1CSSNARK::prove [R] on the running instance a Nifs context holds after its last fold: the outer and inner
// sum-checks (reef_msm.h 3g), then EE::prove_batch over [E, W] (3h, 2h).  Scalars in pasta Montgomery form.
template <int CURVE> class RelaxedR1CSSnark {
  public:
    struct Proof {
        std::vector<reef_fe> tau, r_x, r_y;                  // challenges in call order (r_x[0], r_y[0]: the most significant bit)
        std::vector<std::array<reef_fe, 3>> outer;          // per outer round {e0, e2, e3}
        std::array<reef_fe, 4> claims_outer = {};           // AZ(r_x), BZ(r_x), CZ(r_x), E(r_x)
        reef_fe r_joint = {};                               // the joint-claim challenge
        std::vector<std::array<reef_fe, 2>> inner;          // per inner round {e0, e2}
        std::array<reef_fe, 3> claims_inner = {};           // ABC(r_y), z(r_y), eval_W
        reef_fe cross_term = {}, r_fold = {}, c = {}, r_ipa = {}, a_hat = {};
        std::vector<reef_jacobian> L, R;                    // per IPA round
        std::vector<reef_fe> r_rounds;                      // challenge_r per IPA round
    };
    // num_cons_pad, num_vars_pad: pk.S's padded sizes (powers of two)
    RelaxedR1CSSnark(Nifs<CURVE> &nifs, size_t num_cons_pad, size_t num_vars_pad) : nifs_(nifs), ncp_(num_cons_pad), nvp_(num_vars_pad) {
        log2_exact(ncp_);
        log2_exact(nvp_);
    }
    size_t opening_len() const { return ncp_ > nvp_ ? ncp_ : nvp_; }
    size_t outer_rounds() const { return log2_exact(ncp_); }
    size_t inner_rounds() const { return log2_exact(nvp_) + 1; }   // over z's 2 num_vars_pad entries
    size_t ipa_rounds() const { return log2_exact(opening_len()); }

    // 3g: tau, log2(num_cons_pad) cubic rounds, claims_outer, the joint claim's r, log2(2 num_vars_pad) quadratic rounds, claims_inner
    void prove_sumchecks(const Transcript &transcript, Proof &pf) const {
        reef_nifs_ctx *h = nifs_.handle();
        const size_t ell_x = outer_rounds(), ell_y = inner_rounds();
        pf.tau.clear(); pf.r_x.clear(); pf.r_y.clear(); pf.outer.clear(); pf.inner.clear();
        for (size_t j = 0; j < ell_x; ++j) pf.tau.push_back(transcript("t", nullptr, 0));
        std::array<reef_fe, 3> ev;
        check(reef_spartan_begin(h, ncp_, nvp_, pf.tau.data(), true, ev.data()), "reef_spartan_begin");
        for (size_t i = 0; i < ell_x; ++i) {
            pf.outer.push_back(ev);
            pf.r_x.push_back(transcript("outer", ev.data(), sizeof ev));
            if (i + 1 < ell_x) check(reef_spartan_outer_round(h, &pf.r_x.back(), true, ev.data()), "reef_spartan_outer_round");
            else check(reef_spartan_outer_claims(h, &pf.r_x.back(), true, pf.claims_outer.data()), "reef_spartan_outer_claims");
        }
        pf.r_joint = transcript("claims_outer", pf.claims_outer.data(), sizeof pf.claims_outer);
        std::array<reef_fe, 2> ev2;
        check(reef_spartan_inner_begin(h, &pf.r_joint, true, ev2.data()), "reef_spartan_inner_begin");
        for (size_t j = 0; j < ell_y; ++j) {
            pf.inner.push_back(ev2);
            pf.r_y.push_back(transcript("inner", ev2.data(), sizeof ev2));
            if (j + 1 < ell_y) check(reef_spartan_inner_round(h, &pf.r_y.back(), true, ev2.data()), "reef_spartan_inner_round");
            else check(reef_spartan_inner_claims(h, &pf.r_y.back(), true, pf.claims_inner.data()), "reef_spartan_inner_claims");
        }
    }
    // 3h, after prove_sumchecks.  gens_v: a key of exactly opening_len() points.  comm_a(r): the caller's comm_E + r comm_W, as the
    // bytes it absorbs; q_of(r_ipa): the caller's gens_s.scale(r_ipa), affine.  small_key: the late rounds on a folded key of that many
    // points (reef_spartan_open_set_small_key; a power of two, 0: never).
    void prove_opening(reef_msm_ctx *gens_v, const Transcript &transcript, const std::function<std::vector<uint8_t>(const reef_fe &)> &comm_a,
                       const std::function<reef_affine(const reef_fe &)> &q_of, Proof &pf, size_t small_key = 0) const {
        reef_nifs_ctx *h = nifs_.handle();
        check(reef_spartan_open_set_small_key(h, small_key), "reef_spartan_open_set_small_key");
        pf.L.clear(); pf.R.clear(); pf.r_rounds.clear();
        check(reef_spartan_open_begin(h, gens_v, true, &pf.cross_term), "reef_spartan_open_begin");
        pf.r_fold = transcript("r", &pf.cross_term, sizeof pf.cross_term);
        check(reef_spartan_open_fold(h, &pf.r_fold, true, &pf.c), "reef_spartan_open_fold");
        std::vector<uint8_t> u = comm_a(pf.r_fold);
        u.insert(u.end(), (const uint8_t *)&pf.c, (const uint8_t *)&pf.c + sizeof pf.c);
        pf.r_ipa = transcript("r", u.data(), u.size());
        const reef_affine q = q_of(pf.r_ipa);
        reef_jacobian lr[2];
        check(reef_spartan_open_ipa_begin(h, &q, &lr[0], &lr[1]), "reef_spartan_open_ipa_begin");
        const size_t rounds = ipa_rounds();
        for (size_t k = 0; k < rounds; ++k) {
            pf.L.push_back(lr[0]);
            pf.R.push_back(lr[1]);
            pf.r_rounds.push_back(transcript("challenge_r", lr, sizeof lr));
            if (k + 1 < rounds) check(reef_spartan_open_ipa_round(h, &pf.r_rounds.back(), true, &lr[0], &lr[1]), "reef_spartan_open_ipa_round");
            else check(reef_spartan_open_finish(h, &pf.r_rounds.back(), true, &pf.a_hat), "reef_spartan_open_finish");
        }
    }

    // 3k: A~, B~, C~ at (r_x, r_y), outer_rounds() and inner_rounds() entries, on the ctx's matrices alone (no running instance).
    // RelaxedR1CSSNARK::verify [R] is made of three parts.  (1) The host chain: tau, r_x, r, r_y re-drawn from the transcript, the round
    // sums chained with e1 = claim - e0, claim_outer == eq(tau, r_x) (az bz - u cz - ex) on claims_outer as claimed, eval_X =
    // sum_j eq(r_y[1..])[j] (u || X)[j] and z(r_y) = (1 - r_y[0]) eval_W + r_y[0] eval_X: O(log n) field operations.  (2) This call, for
    // claim_inner == (A~ + r B~ + r^2 C~) z(r_y).  (3) InnerProductArgument::verify below over [E, W] at (r_x, r_y[1..]) with eval_E =
    // claims_outer[3], eval_W = claims_inner[2], c = eval_E + r'^2 eval_W + r' cross.  May be called at any time, mid-prove included.
    std::array<reef_fe, 3> eval_matrices(const std::vector<reef_fe> &r_x, const std::vector<reef_fe> &r_y) const {
        if (r_x.size() != outer_rounds() || r_y.size() != inner_rounds()) throw std::invalid_argument("eval_matrices: r_x, r_y lengths");
        std::array<reef_fe, 3> ev;
        check(reef_spartan_eval_matrices(nifs_.handle(), ncp_, nvp_, r_x.data(), r_y.data(), true, ev.data()), "reef_spartan_eval_matrices");
        return ev;
    }
    // 3o: the same at many points in one call (one host wait; a matrix entry read once for two points): what a verifier of many proofs
    // over one shape calls once its host chains have run.  Entry t is bit for bit eval_matrices(r_x[t], r_y[t]).
    std::vector<std::array<reef_fe, 3>> eval_matrices_batch(const std::vector<std::vector<reef_fe>> &r_x,
                                                            const std::vector<std::vector<reef_fe>> &r_y) const {
        if (r_x.size() != r_y.size()) throw std::invalid_argument("eval_matrices_batch: one r_y per r_x");
        const size_t m = r_x.size(), lx = outer_rounds(), ly = inner_rounds();
        std::vector<reef_fe> xs, ys;
        xs.reserve(m * lx);
        ys.reserve(m * ly);
        for (size_t t = 0; t < m; ++t) {
            if (r_x[t].size() != lx || r_y[t].size() != ly) throw std::invalid_argument("eval_matrices_batch: r_x, r_y lengths");
            xs.insert(xs.end(), r_x[t].begin(), r_x[t].end());
            ys.insert(ys.end(), r_y[t].begin(), r_y[t].end());
        }
        std::vector<std::array<reef_fe, 3>> ev(m);
        if (m) check(reef_spartan_eval_matrices_batch(nifs_.handle(), ncp_, nvp_, xs.data(), ys.data(), m, true, ev[0].data()),
                     "reef_spartan_eval_matrices_batch");
        return ev;
    }

  private:
    Nifs<CURVE> &nifs_;
    size_t ncp_, nvp_;
};

// HyraxPC::prove_eval [R] over a document kept resident from NLDocCommitment::new on (reef_msm.h 3i): plain
// ipa_pc rounds (no blinding term).  Scalars in pasta Montgomery form.
template <int CURVE> class HyraxEval {
  public:
    struct Proof {
        reef_fe eval = {}, lz_blind = {}, r_q = {}, a_hat = {}, b_hat = {};
        reef_jacobian comm_lz = {};
        std::vector<reef_jacobian> L, R;
        std::vector<reef_fe> r_rounds;
    };
    // NLDocCommitment::new: z (n <= 2^num_vars entries of elem_bytes each, host or device) and the 2^left_vars row blinds
    HyraxEval(const void *z, size_t n, int elem_bytes, int z_loc, size_t num_vars, size_t left_vars, const reef_fe *row_blinds, int device = 0)
        : num_vars_(num_vars), left_(left_vars) {
        check(reef_hyrax_create(&ctx_, CURVE, z, n, elem_bytes, z_loc, true, num_vars, left_vars, row_blinds, device), "reef_hyrax_create");
    }
    ~HyraxEval() { reef_hyrax_destroy(ctx_); }
    HyraxEval(const HyraxEval &) = delete;
    HyraxEval &operator=(const HyraxEval &) = delete;
    size_t rounds() const { return num_vars_ - left_; }

    // HyraxPC::commit of the resident document: PolyCommit.comm, 2^left_vars compressed rows (host).  gens_v: the key prove takes; h:
    // exactly when the ctx holds row blinds.  The rows also stay on the device: eval_comm_own and prove_own take them from there.
    std::vector<Compressed> commit(reef_msm_ctx *gens_v, const reef_affine *h) {
        std::vector<Compressed> comm((size_t)1 << left_);
        check(reef_hyrax_commit(ctx_, gens_v, h, comm.data()->data(), nullptr, REEF_HOST), "reef_hyrax_commit");
        return comm;
    }
    // comm_LZ = sum_i L_i C_i over the committed rows, after a prove's eval_begin
    reef_jacobian eval_comm_own() const {
        reef_jacobian out;
        check(reef_hyrax_eval_comm_own(ctx_, &out), "reef_hyrax_eval_comm_own");
        return out;
    }
    // prove on the ctx's own commitment (commit came first): no row commitment is uploaded
    void prove_own(reef_msm_ctx *gens_v, const reef_fe *point, const Transcript &transcript, const std::function<reef_affine(const reef_fe &)> &q_of,
                   Proof &pf, size_t small_key = 0) const {
        prove_with(gens_v, point, transcript, q_of, pf, small_key, [&] { pf.comm_lz = eval_comm_own(); });
    }

    // proof_dot_prod_prover -> prove_eval at `point` (num_vars entries).  gens_v: a key of exactly 2^rounds() points; row_comms:
    // the 2^left_vars affine row commitments (row_comms_loc memory); q_of(r): the caller's gens_1.scale(r), affine.  small_key: the late
    // rounds on a folded key of that many points (reef_hyrax_set_small_key; a power of two, 0: never).
    void prove(reef_msm_ctx *gens_v, const reef_fe *point, const reef_affine *row_comms, int row_comms_loc, const Transcript &transcript,
               const std::function<reef_affine(const reef_fe &)> &q_of, Proof &pf, size_t small_key = 0) const {
        prove_with(gens_v, point, transcript, q_of, pf, small_key, [&] { check(reef_hyrax_eval_comm(ctx_, row_comms, row_comms_loc, &pf.comm_lz), "reef_hyrax_eval_comm"); });
    }
    // the same with the rows as Reef holds them, PolyCommit.comm: 2^left_vars compressed commitments (host), decoded on the device
    void prove(reef_msm_ctx *gens_v, const reef_fe *point, const Compressed *row_comms, const Transcript &transcript,
               const std::function<reef_affine(const reef_fe &)> &q_of, Proof &pf, size_t small_key = 0) const {
        prove_with(gens_v, point, transcript, q_of, pf, small_key, [&] {
            check(reef_hyrax_eval_comm_compressed(ctx_, row_comms->data(), REEF_HOST, &pf.comm_lz), "reef_hyrax_eval_comm_compressed");
        });
    }

  private:
    template <class CommLz>
    void prove_with(reef_msm_ctx *gens_v, const reef_fe *point, const Transcript &transcript, const std::function<reef_affine(const reef_fe &)> &q_of,
                    Proof &pf, size_t small_key, CommLz &&comm_lz) const {
        check(reef_hyrax_set_small_key(ctx_, small_key), "reef_hyrax_set_small_key");
        pf.L.clear(); pf.R.clear(); pf.r_rounds.clear();
        check(reef_hyrax_eval_begin(ctx_, gens_v, point, true, &pf.eval, &pf.lz_blind), "reef_hyrax_eval_begin");
        comm_lz();
        uint8_t u[sizeof(reef_jacobian) + sizeof(reef_fe)];
        memcpy(u, &pf.comm_lz, sizeof(reef_jacobian));
        memcpy(u + sizeof(reef_jacobian), &pf.eval, sizeof(reef_fe));
        pf.r_q = transcript("r", u, sizeof u);
        const reef_affine q = q_of(pf.r_q);
        reef_jacobian lr[2];
        check(reef_hyrax_ipa_begin(ctx_, &q, nullptr, nullptr, true, &lr[0], &lr[1]), "reef_hyrax_ipa_begin");
        const size_t k_end = rounds();
        for (size_t k = 0; k < k_end; ++k) {
            pf.L.push_back(lr[0]);
            pf.R.push_back(lr[1]);
            pf.r_rounds.push_back(transcript("challenge_r", lr, sizeof lr));
            if (k + 1 < k_end) check(reef_hyrax_ipa_round(ctx_, &pf.r_rounds.back(), nullptr, true, &lr[0], &lr[1]), "reef_hyrax_ipa_round");
            else check(reef_hyrax_finish(ctx_, &pf.r_rounds.back(), true, &pf.a_hat, &pf.b_hat), "reef_hyrax_finish");
        }
    }
    reef_hyrax_ctx *ctx_ = nullptr;
    size_t num_vars_, left_;
};

// The verifier's key of a committed document (reef_msm.h 3n): PolyCommit.comm decoded and keyed once, then
// comm_LZ = sum_i eq(point[..left])_i C_i of HyraxPC::verify_eval [R] for any number of points per call.  Scalars in pasta Montgomery form.
template <int CURVE> class HyraxVk {
  public:
    // row_comms: the 2^left_vars compressed rows (host); device -1: the current one; key_opts: as CommitmentGens' (nullptr: the default key)
    HyraxVk(const Compressed *row_comms, size_t left_vars, int device = -1, const reef_msm_opts *key_opts = nullptr) : left_(left_vars) {
        check(reef_hyrax_vk_create(&vk_, CURVE, row_comms->data(), left_vars, REEF_HOST, device, key_opts), "reef_hyrax_vk_create");
    }
    // the same from rows already in device memory (16-byte aligned)
    HyraxVk(const uint8_t *d_row_comms32, size_t left_vars, int device, const reef_msm_opts *key_opts) : left_(left_vars) {
        check(reef_hyrax_vk_create(&vk_, CURVE, d_row_comms32, left_vars, REEF_DEVICE, device, key_opts), "reef_hyrax_vk_create");
    }
    ~HyraxVk() { reef_hyrax_vk_destroy(vk_); }
    HyraxVk(const HyraxVk &) = delete;
    HyraxVk &operator=(const HyraxVk &) = delete;
    size_t left_vars() const { return left_; }

    // points: m x left_vars scalars, row-major.  comm_lz[t] for every point and, when asked for, its encoding: one call, one pass
    std::vector<reef_jacobian> comm_lz(const reef_fe *points, size_t m, std::vector<Compressed> *compressed = nullptr) const {
        std::vector<reef_jacobian> out(m);
        if (compressed) compressed->resize(m);
        if (m) check(reef_hyrax_vk_comm_lz(vk_, points, m, true, out.data(), compressed ? compressed->data()->data() : nullptr), "reef_hyrax_vk_comm_lz");
        return out;
    }

  private:
    reef_hyrax_vk *vk_ = nullptr;
    size_t left_;
};

// InnerProductArgument::verify [R]: the check EE::verify_batch and HyraxPC::verify_eval end with (reef_msm.h 3j).
// The caller has drawn the round challenges from its transcript; b = sum_t weights[t] pad(eq(points[t])) is built on the device.
// Scalars in pasta Montgomery form.  A proof that does not verify gives false; bad arguments throw.
template <int CURVE> struct InnerProductArgument {
    std::vector<reef_jacobian> L, R;     // log2(n) each
    reef_fe a_hat = {};
    // gens_v: a key of at least n points; comm, c: the instance's commitment and claimed inner product; q = gens_s.scale(r), affine;
    // rs: log2(n) round challenges; h, blind: the optional blind term (both or neither)
    bool verify(reef_msm_ctx *gens_v, size_t n, const reef_jacobian &comm, const reef_fe &c, const reef_affine &q, const std::vector<reef_fe> &rs,
                const std::vector<std::vector<reef_fe>> &points, const std::vector<reef_fe> &weights, const reef_affine *h = nullptr,
                const reef_fe *blind = nullptr) const {
        if (L.size() != rs.size() || R.size() != rs.size() || points.size() != weights.size()) return false;
        std::vector<const reef_fe *> pts;
        std::vector<size_t> vars;
        for (const auto &p : points) {
            pts.push_back(p.data());
            vars.push_back(p.size());
        }
        uint32_t accept = 0;
        check(reef_ipa_check_eq(gens_v, n, &comm, &c, &q, L.data(), R.data(), rs.data(), &a_hat, pts.data(), vars.data(), weights.data(), points.size(), h,
                                blind, true, &accept, nullptr, nullptr, nullptr), "reef_ipa_check_eq");
        return accept == 1;
    }

    // One proof of a batch: what verify takes beside the proof itself.  The vectors must outlive the call.
    struct Instance {
        const InnerProductArgument *proof;
        reef_jacobian comm;
        reef_fe c;
        reef_affine q;
        std::vector<reef_fe> rs;
        std::vector<std::vector<reef_fe>> points;
        std::vector<reef_fe> weights;
        const reef_affine *h = nullptr;
        const reef_fe *blind = nullptr;
    };
    // m proofs over the same n against the one gens_v in a single pass (reef_msm.h 3m): one MSM over the key whatever m is.  rho: one
    // non-zero weight per proof, the CALLER'S randomness, drawn after every proof is fixed.  each (may be null): resized to m; all true
    // when the batch accepts, else the single checks run (m MSMs) and say which proofs fail.
    static bool verify_batch(reef_msm_ctx *gens_v, size_t n, const std::vector<Instance> &batch, const std::vector<reef_fe> &rho,
                             std::vector<bool> *each = nullptr) {
        const size_t m = batch.size();
        if (rho.size() != m) return false;
        std::vector<reef_ipa_proof> proofs(m);
        std::vector<std::vector<const reef_fe *>> pts(m);
        std::vector<std::vector<size_t>> vars(m);
        for (size_t i = 0; i < m; ++i) {
            const Instance &in = batch[i];
            if (!in.proof || in.proof->L.size() != in.rs.size() || in.proof->R.size() != in.rs.size() || in.points.size() != in.weights.size()) return false;
            for (const auto &p : in.points) {
                pts[i].push_back(p.data());
                vars[i].push_back(p.size());
            }
            proofs[i] = reef_ipa_proof{&in.comm, &in.c, &in.q, in.proof->L.data(), in.proof->R.data(), in.rs.data(), &in.proof->a_hat, pts[i].data(),
                                       vars[i].data(), in.weights.data(), in.points.size(), in.h, in.blind};
        }
        uint32_t all = 0;
        std::vector<uint32_t> acc(each ? m : 0);
        check(reef_ipa_check_batch(gens_v, n, proofs.data(), m, rho.data(), true, &all, each && m ? acc.data() : nullptr, nullptr, nullptr, REEF_HOST, nullptr,
                                   nullptr), "reef_ipa_check_batch");
        if (each) each->assign(acc.begin(), acc.end());
        return all == 1;
    }
};

}  // namespace reef_provider
