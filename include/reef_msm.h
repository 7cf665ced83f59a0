/* libreef_msm.so -- MI355X (gfx950) backend for the Pasta-curve MSM hot path of eniac/Reef.
 *
 * C ABI only: plain pointers and sizes, no C++ / torch types.  Every entry point names the
 * reference interface it replaces (paths relative to the Reef repository).  Symbols marked
 * [R] belong to crates that are NOT vendored in the reference tree (nova-snark @ sga001/Nova,
 * fil_pasta_curves 0.5.2, pasta-msm; Cargo.toml:12,14) -- their layouts are isolated in this
 * header so they can be corrected in one place.
 *
 * Data layouts (fil_pasta_curves `repr-c`, Cargo.toml:14) [R]:
 *   reef_fe        4 x u64 little-endian limbs, Montgomery form (R = 2^256), fully reduced
 *   reef_affine    {x, y}      64 B, identity = (0, 0)                 (EpAffine / EqAffine)
 *   reef_jacobian  {x, y, z}   96 B, identity has z = 0                (Ep / Eq)
 * Scalars of Pallas are Fq elements, scalars of Vesta are Fp elements (the cycle).
 *
 * Error behaviour: the reference treats every failure as a panic (framework.rs:683,702).  The
 * pasta-msm compatible symbols return void and abort() with a message on any error; the handle
 * API returns a reef_status and records a message retrievable with reef_last_error().  There is
 * no CPU fallback: without a usable gfx950 device every call fails loudly.
 *
 * Threading: all entry points are re-entrant.  A reef_msm_ctx serialises the calls made on it
 * (it owns one HIP stream and one workspace); use one ctx (or clone) per concurrent caller.
 *
 * ABI changelog (reef_abi_version()):
 *   7  the NIFS fold of a folding step on the device (reef_nifs_*, section 3f): R1CS cross term T, comm_T, the folds of W, E, u, X,
 *      and the relaxed-R1CS check.  Nothing else changed.
 *      Later, still 7 (symbols added, none changed): the sum-checks of the final SNARK on a NIFS ctx's running instance
 *      (reef_spartan_*, section 3g).  A caller that needs them checks for the symbol, not the version.
 *      Later, still 7 (symbols added, none changed): the batched IPA opening of the final SNARK on the same ctx
 *      (reef_spartan_open_*, section 3h).
 *      Later, still 7 (symbols added, none changed): the Hyrax consistency argument on a resident document (reef_hyrax_*, section 3i).
 *      Later, still 7 (symbols added, none changed): K4's inverse, reef_decompress, and reef_hyrax_eval_comm_compressed on top of it.
 *      Later, still 7 (symbols added, none changed): the verifier's IPA check on a key ctx (reef_ipa_check, reef_ipa_check_eq, section 3j).
 *      Later, still 7 (symbols added, none changed): the verifier's matrix evaluations on a NIFS ctx (reef_spartan_eval_matrices, section 3k).
 *      Later, still 7 (symbols added, none changed): the sum-check table set from parts -- field elements, a fill, document symbols
 *      (reef_sc_set_table_parts, section 3b).
 *      Later, still 7 (symbols added, none changed): the row commitments of a resident Hyrax document from its own ctx
 *      (reef_hyrax_commit, reef_hyrax_eval_comm_own, section 3i).
 *      Later, still 7 (symbols added, none changed): a document's bytes turned into alphabet symbols on the device
 *      (reef_doc_transform, section 3l).
 *      Later, still 7 (symbols added, none changed): entries of the sum-check table as last set, by index (reef_sc_lookup, section 3b).
 *      Later, still 7 (symbols added, none changed): a batch of IPA openings checked against one key in a single pass
 *      (reef_ipa_check_batch, reef_ipa_check_batch_last_timing, section 3m).
 *      Later, still 7 (symbols added, none changed): a verifier's key of a committed document and comm_LZ for many points in one pass
 *      (reef_hyrax_vk_create, reef_hyrax_vk_destroy, reef_hyrax_vk_comm_lz, section 3n).
 *      Later, still 7 (symbols added, none changed): the verifier's matrix evaluations at many points in one pass
 *      (reef_spartan_eval_matrices_batch, reef_nifs_set_eval_workspace, reef_spartan_eval_matrices_batch_last_info, section 3o).
 *      Later, still 7 (symbols added, none changed): the Hyrax consistency arguments of many proofs over one resident document in
 *      lock-step (reef_hyrax_batch_*, section 3p).
 *   6  round 6: the drop-in symbols build a returning key's resident copy on a builder thread (no call pays for it: reef_key_cache_wait,
 *      reef_key_cache_stats.spares in place of .reserved); REEF_SC_FENCE defaults to the release-ordered ticket; device groups report where a
 *      call's time went (reef_msm_group_enable_timing / _last_timing) and take REEF_SCALARS_FANOUT (reef_msm_group_opts.scalars, was reserved[0]).
 *   5  round 5: device groups (reef_msm_group_*: one MSM split by window or by points, or the rows of a Hyrax commitment dealt out
 *      whole, over several GPUs of ONE process, the partial sums exchanged inside the library: peer copies, host slots, or a
 *      single-process RCCL communicator loaded at run time); reef_merkle_commit_devices (the Merkle tree in blocks over several GPUs); reef_get_device;
 *      reef_key_cache_timing_get; reef_runtime_opts.hw_queues is the only way the library touches GPU_MAX_HW_QUEUES unless
 *      REEF_MSM_HW_QUEUES is exported (the load-time default of rounds 3-4 is gone); the drop-in symbols confirm a returning key's
 *      bytes on the host whatever its size (no key upload on a hit).
 *   4  round 4: reef_runtime_init / reef_abi_version / reef_msm_ctx_attach / reef_msm_multi / reef_key_cache_info added; the drop-in symbols' key cache is one table per process
 *      (clones per calling thread) instead of one cache per thread.
 *   3  round 3: reef_msm_opts.byte_tables = 0 changed meaning from "build the byte tables in the background" to "follow the
 *      process-wide policy: none unless REEF_MSM_WIDE=1" -- callers that pass zeroed opts no longer get the byte-table path
 *      for MSM / IPA unless they ask (1 or 3).  A performance difference only; results are identical.
 *   2  round 2: byte tables, nibble tables, reef_msm_folded, rows N1-N4.
 *   1  round 1.
 */
#ifndef REEF_MSM_H
#define REEF_MSM_H
#define REEF_ABI_VERSION 7

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint64_t l[4]; } reef_fe;
typedef struct { reef_fe x, y; } reef_affine;
typedef struct { reef_fe x, y, z; } reef_jacobian;

enum { REEF_PALLAS = 0, REEF_VESTA = 1 };
enum { REEF_HOST = 0, REEF_DEVICE = 1 }; /* where a buffer lives */

typedef enum {
    REEF_OK = 0,
    REEF_ERR_ARG = 1,    /* bad argument (null pointer, size mismatch, unknown curve) */
    REEF_ERR_HIP = 2,    /* HIP runtime error (message in reef_last_error) */
    REEF_ERR_NO_GPU = 3, /* no gfx950 device visible */
    REEF_ERR_OOM = 4
} reef_status;

/* ---------------------------------------------------------------------------------------------
 * (1) pasta-msm drop-in symbols [R].
 * Replaces: `extern "C" mult_pippenger_pallas/vesta` declared by the pasta-msm crate and reached
 * from nova-snark's `Group::vartime_multiscalar_mul` (provider/pasta.rs) for every commitment:
 * src/backend/framework.rs:668 (RecursiveSNARK::prove_step), :695 (CompressedSNARK::prove),
 * src/backend/commitment.rs:187,350,361,371,383,422,430.
 * Stateless: nothing is retained; bases are uploaded per call.  `is_mont` = scalars are in
 * Montgomery form (what the Rust wrapper passes).  abort()s on error.
 * ------------------------------------------------------------------------------------------- */
/* (A key that keeps coming back is nominated by a non-cryptographic hash of 64 sampled points (no pass over all of its bytes), CONFIRMED byte for byte
 * against a retained HOST copy while the GPU already works on the nominated key (helper threads share the comparison of
 * keys above 4 MiB), and served from a resident pre-shifted copy as soon as one exists; a hash collision
 * therefore costs time, never a wrong result, and nothing the caller can observe is retained.  The resident copy is built OFF the
 * caller's thread: the call that brings a key's second appearance is served like the first, keeps a copy of the key's bytes and
 * returns; one builder thread of the process uploads the copy, builds the tables and prepares a ready context for the first call
 * that finds the key published (typically the third or fourth).  A caller never waits for the builder.  The table of resident keys is
 * one per process (at most 16 keys, REEF_MSM_KEY_CACHE_MB of device memory, default 16384, and REEF_MSM_KEY_HOST_MB of host
 * memory, default 4096; a key stays charged while any thread's context is still attached to it): the key is built once, whichever threads call --
 * nova-snark reaches these symbols from the prover thread and from rayon workers, src/backend/framework.rs:110,
 * 668,695 -- and each calling thread serves it through its own stream and workspace on the shared tables.  On an
 * allocation failure the table is emptied and the call is served uncached.  REEF_MSM_KEY_CACHE=0 turns it off.) */
void mult_pippenger_pallas(reef_jacobian *out, const reef_affine *points, size_t npoints,
                           const reef_fe *scalars, bool is_mont);
void mult_pippenger_vesta(reef_jacobian *out, const reef_affine *points, size_t npoints,
                          const reef_fe *scalars, bool is_mont);
/* What the drop-in symbols' process-wide key table holds (tests, diagnostics): entries nominated, keys with a resident copy,
 * device bytes charged to the budget, and counters since the process started -- resident copies built, calls served from
 * one, per-thread contexts made by the calling threads themselves, speculative calls whose bytes turned out to be another key's (served again on the plain path), ready contexts the builder thread prepared.  reef_key_cache_clear drops every entry (threads let go of their clones at their next call). */
typedef struct {
    uint64_t entries, resident_keys, resident_bytes, builds, hits, clones, misspeculated, spares;
} reef_key_cache_stats;
void reef_key_cache_info(reef_key_cache_stats *out);
void reef_key_cache_clear(void);
/* Blocks until the builder thread has nothing left to do (tests and timing harnesses that want a deterministic "the key is resident
 * now"; a prover never needs it). */
void reef_key_cache_wait(void);
/* Where the calls served from a resident key spent their time on the HOST, summed over all calling threads since the last reset
 * (nanoseconds; diagnostics: tools/seam_bench): nominating the key (sampled hash + table lookup), enqueueing the MSM (includes the
 * staging of the caller's pageable scalars), confirming the caller's bytes (memcmp against the retained copy, beside the GPU), and
 * waiting for the result. */
typedef struct {
    uint64_t calls, nominate_ns, enqueue_ns, confirm_ns, wait_ns, reserved[3];
} reef_key_cache_timing;
void reef_key_cache_timing_get(reef_key_cache_timing *out, int reset);

/* ---------------------------------------------------------------------------------------------
 * (2) Resident-key handle API.
 * Replaces: nova-snark `CommitmentGens<G>` [R] as held inside PublicParams / HyraxPC for the
 * life of a proof (src/backend/framework.rs:45,134,297-303; src/backend/commitment.rs:176-186).
 * The bases are uploaded once; with `precompute` the key also stores 2^(c*G*j)-shifted copies so
 * that several Pippenger windows share one bucket set (HBM is 288 GB; a 2^20-point key with
 * 16 tables is 1 GiB).
 * ------------------------------------------------------------------------------------------- */
typedef struct reef_msm_ctx reef_msm_ctx;

typedef struct {
    uint32_t window_bits;   /* Pippenger window c; 0 = choose from n */
    uint32_t bucket_groups; /* G: 0 = one group per window (no precompute); 1 = full precompute
                               (all windows share one bucket set); otherwise windows w and w'
                               share buckets iff w % G == w' % G */
    uint32_t chunk;         /* sorted entries per accumulation thread (L0); 0 = default */
    uint32_t byte_tables;   /* bucket_groups = 1, 1024 < n <= 65536: the sort-free byte tables (256 KiB per point, 14-38 ms to
                               build).  OPT-IN: 0 = the process-wide policy (none, unless REEF_MSM_WIDE=1 is set: then as 3),
                               1 = built inside reef_msm_ctx_create, 2 = never, 3 = built in the background on a
                               low-priority stream of the key's own (the bucket pipeline serves the key until they are
                               ready; calls that run beside the build are slowed by it).  For keys that live long enough
                               to earn them (a prover service).  See reef_msm_ctx_byte_tables. */
    int32_t device;         /* HIP device ordinal; -1 = current device */
    uint32_t reserved[3];
} reef_msm_opts;

reef_status reef_msm_ctx_create(reef_msm_ctx **out, int curve, const reef_affine *bases, size_t n,
                                int bases_loc, const reef_msm_opts *opts /* may be NULL */);
/* 1 when MSMs on this key are served from its byte tables (a mid-size resident key: every signed byte multiple of every point
 * tabulated, an MSM is a plain sum of table entries: no sort, no buckets; 2^15 points 0.19 ms against 0.32 ms), else 0. */
int reef_msm_ctx_byte_tables(reef_msm_ctx *ctx);
/* Replace the key of a ctx in place (same options, workspace kept): what the IPA rounds need, where
 * the generators change every round (CommitmentGens::fold [R], framework.rs:695).  Fails on a ctx
 * whose key is shared with clones. */
reef_status reef_msm_ctx_set_bases(reef_msm_ctx *ctx, const reef_affine *bases, size_t n, int bases_loc);
/* A second handle on the same resident key with its own stream and workspace (for callers that
 * issue MSMs from several threads, e.g. nova's rayon workers inside ipa_pc). */
reef_status reef_msm_ctx_clone(reef_msm_ctx **out, reef_msm_ctx *src);
/* ctx becomes what a clone of src would be -- a handle on src's resident key -- but keeps its own stream and workspace (O(1);
 * waits for the work already enqueued on ctx; same curve and device).  For callers with more keys than threads: one ctx per
 * thread, attached to the key of the moment (what the drop-in symbols do per calling thread). */
reef_status reef_msm_ctx_attach(reef_msm_ctx *ctx, reef_msm_ctx *src);
void reef_msm_ctx_destroy(reef_msm_ctx *ctx);
/* Block until everything enqueued on the ctx's stream has finished. */
reef_status reef_msm_ctx_sync(reef_msm_ctx *ctx);
/* The ctx's hipStream_t (as void*), e.g. to order work of a torch/RCCL stream after it: from here on the ctx stays on this stream of the
 * library's pool.  NULL on failure (no stream could be had; reef_last_error() says why) -- never a stand-in for the default stream. */
void *reef_msm_ctx_stream(reef_msm_ctx *ctx);

/* K1: out = sum_{i<n} scalars[i] * bases[i], n <= key length.
 * Replaces Group::vartime_multiscalar_mul / CE::commit without blind [R] (call sites above).
 * With out_loc == REEF_DEVICE the call only enqueues work (no host sync). */
reef_status reef_msm(reef_msm_ctx *ctx, const reef_fe *scalars, size_t n, int scalars_loc,
                     bool is_mont, reef_jacobian *out, int out_loc);

/* `count` independent MSMs issued at once, MSM i on ctxs[i] with scalars[i][0 .. n[i]): all are enqueued before any is waited
 * for, each on the stream its context takes from the library's pool, so their latency-bound stages overlap on the GPU.  The
 * contexts must be distinct (clone a key that commits twice); they may belong to different curves.  out: `count` commitments in
 * host memory.  For the two commitments of ONE curve inside RecursiveSNARK::prove_step (comm_W of the fresh witness and the
 * cross term comm_T of NIFS::prove [R]: both are absorbed before the folding challenge is drawn, neither needs the other;
 * src/backend/framework.rs:668-675) -- the commitments of the two curves are NOT independent of each other: the secondary
 * step circuit hashes the primary's folded instance, which contains them.  reef_msm_rows(rows = 2) is the other way to issue
 * such a pair (one pass of the pipeline over both; same key, equal lengths). */
reef_status reef_msm_multi(size_t count, reef_msm_ctx *const *ctxs, const reef_fe *const *scalars, const size_t *n, int scalars_loc,
                           bool is_mont, reef_jacobian *out);

/* K2: rows independent MSMs over the same first row_len bases, plus an optional Pedersen blind:
 *   out[r] = sum_j scalars[r*row_len + j] * bases[j]  (+ blinds[r] * h   if blinds != NULL)
 * Replaces HyraxPC::commit(&poly) [R] at src/backend/commitment.rs:187 (L = 2^(l/2) rows of
 * R = 2^(l - l/2) symbols each, src/backend/commitment.rs:173-174) and CE::commit with blind
 * (commitment.rs:350,361,422,430) when rows == 1.  `max_scalar_bits` bounds the canonical
 * scalars (e.g. 8 for ASCII symbols, 3 for DNA; framework.rs:978-1011); 0 = measure on device.
 * blinds/h live where scalars live. */
reef_status reef_msm_rows(reef_msm_ctx *ctx, const reef_fe *scalars, size_t rows, size_t row_len,
                          int scalars_loc, bool is_mont, uint32_t max_scalar_bits,
                          const reef_fe *blinds, const reef_affine *h, reef_jacobian *out,
                          int out_loc);

/* The same commitments from the document's own symbols: one unsigned byte per entry (< 2^symbol_bits,
 * symbol_bits in 1..8), as Reef holds the document before turning it into field elements
 * (src/backend/framework.rs:978-1011 -> NLDocCommitment::new, src/backend/commitment.rs:133-212).
 * Tiny scalars need no bucket method: the generators are taken k at a time (2^(symbol_bits*k) <= 512),
 * every combination is tabulated once per (ctx, row_len, symbol_bits), and a row is the plain sum of
 * row_len/k table entries.  reef_msm_rows takes the same path on its own when max_scalar_bits <= 8 and
 * the batch is large enough to pay for the tables.  blinds/h live where the symbols live; blinds are
 * field elements (Montgomery form if blinds_are_mont). */
reef_status reef_msm_rows_symbols(reef_msm_ctx *ctx, const uint8_t *symbols, size_t rows, size_t row_len, int symbols_loc,
                                  uint32_t symbol_bits, const reef_fe *blinds, const reef_affine *h, bool blinds_are_mont,
                                  reef_jacobian *out, int out_loc);

/* The same from symbols wider than a byte: elem_bytes = 2 (uint16_t) or 4 (uint32_t), little-endian, symbol_bits in
 * 1..8*elem_bytes (an alphabet of 254 characters already needs 9 bits: EPSILON and EOF are |ab| + 1 and |ab| + 2,
 * framework.rs:978-1011).  Only the low symbol_bits bits of a symbol are used.  A symbol is the sum of its bytes times powers of
 * 256, so a row is the plain sum of P * row_len entries (P = ceil(symbol_bits / 8)) of byte-multiple tables over the plane
 * generators 256^p * G_j, cached per (ctx, row_len, symbol_bits) like the byte entry's tables (one set at a time: a byte call
 * after a wide call rebuilds its own, and the reverse).  Everything else is the contract of reef_msm_rows_symbols.
 * REEF_ERR_ARG before any device work: elem_bytes not 2 or 4, symbol_bits out of range, row_len above the key length, blinds
 * without h, more than 2^26 table points, rows * row_len * P >= 2^31 entries. */
reef_status reef_msm_rows_symbols_wide(reef_msm_ctx *ctx, const void *symbols, uint32_t elem_bytes, size_t rows, size_t row_len,
                                       int symbols_loc, uint32_t symbol_bits, const reef_fe *blinds, const reef_affine *h,
                                       bool blinds_are_mont, reef_jacobian *out, int out_loc);

/* IPA round WITHOUT generator folding.  After k rounds of G'_i = w1*G_i + w2*G_{i+half} the
 * generators are fixed linear combinations of the original ones, so the cross terms of round k
 *     L = <a_lo, G^(k)_hi>,   R = <a_hi, G^(k)_lo>        (a = a_lo || a_hi, n_k = n / 2^k scalars)
 * are two MSMs over the ORIGINAL resident key with scalars a[.] * prod(challenges): this replaces
 * CommitmentGens::fold + the two commits of ipa_pc::InnerProductArgument::prove [R]
 * (CompressedSNARK::prove, src/backend/framework.rs:695; HyraxPC::prove_eval, commitment.rs:371,383)
 * and yields bit-identical L, R.  w1s/w2s: the k challenges so far, canonical integers on the host
 * (same convention as reef_fold); n_k * 2^k must equal the key length.  L and R go to the host. */
reef_status reef_ipa_cross_terms(reef_msm_ctx *ctx, const reef_fe *a, size_t n_k, int a_loc, bool is_mont,
                                 const reef_fe *w1s, const reef_fe *w2s, size_t k, reef_jacobian *out_l,
                                 reef_jacobian *out_r);

/* A commitment over FOLDED generators without folding them: what CE::commit(&gens.fold(..).fold(..), v) [R] returns when
 * `gens` is the resident key of ctx.  With n_k = n / 2^k generators after k folds (challenges w1s[m], w2s[m], canonical
 * integers on the host, same convention as reef_fold),
 *     out = sum_{j < len} v[j] * G^(k)_{off + j},     off + len <= n_k,
 * computed as one MSM over the original key with scalars v[j] * prod(challenges).  `off`/`len` select a slice, so the halves
 * of CommitmentGens::split_at and the last remaining generator (len = 1 after log2(n) folds, v = [1]) are the same call:
 * a CommitmentGens that records its folds instead of performing them (reef_amd/provider.py FoldedGens,
 * host/reef_provider.hpp) serves nova-snark's ipa_pc unchanged -- no 255-bit scalar multiplication per generator, no
 * re-keying.  k = 0 is a commitment over a slice of the key.  The key length must be a multiple of 2^k. */
reef_status reef_msm_folded(reef_msm_ctx *ctx, const reef_fe *v, size_t len, size_t off, int v_loc, bool is_mont,
                            const reef_fe *w1s, const reef_fe *w2s, size_t k, reef_jacobian *out, int out_loc);

/* K3, deep: the generators k folds away from the resident key of src, in ONE pass instead of k folds.  After k rounds of
 * G'_i = w1*G_i + w2*G_{i+half},
 *     G^(k)_j = sum_{t < 2^k} s_t * G_{t*n_k + j},    n_k = n / 2^k,    s_t = prod_m (bit_{k-1-m}(t) ? w2s[m] : w1s[m]),
 * so the n_k outputs all use the SAME 2^k scalars: one bucket pass whose digit is the same for every output (no sort, no
 * divergence), then one window combine per output.  out[j] = G^(k)_j for j < n_k: the points k successive reef_fold calls
 * produce, affine in ABI form, the identity as (0, 0).  w1s, w2s: canonical integers on the host, in the convention and order
 * of reef_ipa_cross_terms and reef_msm_folded; any scalar below the modulus is legal, 0 included.  k = 0 copies the key,
 * k = log2(n) gives one point.  Works on a plain, a pre-shifted, a byte-table and a nibble-table key alike (table 0 is read).
 * REEF_ERR_ARG, with nothing written: a key length that is not a multiple of 2^k, k > 31, a scalar not below the modulus, a
 * ctx with a window split.  The call waits for its work. */
reef_status reef_fold_deep(reef_msm_ctx *src, const reef_fe *w1s, const reef_fe *w2s, size_t k, reef_affine *out, int out_loc);

/* The same points as a resident key of their own: reef_fold_deep into a device buffer, then reef_msm_ctx_create from it;
 * nothing visits the host.  Same curve and device as src (opts->device is ignored); the other opts as in reef_msm_ctx_create:
 * with bucket_groups = 1 and at most 1024 points the key gets its nibble tables, as any small key does.  The late rounds of
 * an IPA then run over n_k points with only the challenges drawn since (reef_ipa_cross_terms on the new key). */
reef_status reef_msm_ctx_create_folded(reef_msm_ctx **out, reef_msm_ctx *src, const reef_fe *w1s, const reef_fe *w2s, size_t k,
                                       const reef_msm_opts *opts);

/* ---------------------------------------------------------------------------------------------
 * (3) Stateless helpers around the MSMs.
 * ------------------------------------------------------------------------------------------- */
/* K3: out[i] = w1*gens[i] + w2*gens[half+i], i < half, affine out.
 * Replaces CommitmentGens::fold [R] as used by ipa_pc::InnerProductArgument::prove inside
 * CompressedSNARK::prove (src/backend/framework.rs:695).  w1, w2: canonical (non-Montgomery)
 * 32-byte little-endian scalars on the host. */
reef_status reef_fold(int curve, const reef_affine *gens, size_t half, int loc, const reef_fe *w1,
                      const reef_fe *w2, reef_affine *out);

/* K4: batch Jacobian -> affine and/or 32-byte compressed encoding (LE canonical x, y parity in
 * bit 255, identity = zeros).  Replaces Commitment::compress / to_affine [R]
 * (src/backend/commitment.rs:195,351,365,425,427,431).  Either output may be NULL. */
reef_status reef_normalize(int curve, const reef_jacobian *in, size_t n, int loc, reef_affine *out_affine,
                           uint8_t *out_compressed);

/* K4 inverse: n 32-byte encodings -> affine (ABI form).  Replaces CompressedCommitment::decompress [R] over PolyCommit.comm
 * (src/backend/commitment.rs:60,192-197; HyraxPC::prove_eval).  The rule is pasta_curves' from_bytes [R]: 32 zero bytes are the
 * identity, (0, 0); otherwise bit 255 is the parity of y and the low 255 bits are x, little-endian; x >= p or x^3 + 5 a non-residue
 * (00..00 80 among them: x = 0) is invalid.  Invalid entries give (0,0); *invalid (host, may be NULL) = how many,
 * *first_invalid (host, may be NULL) = the lowest such index (n when none).  REEF_OK whenever the batch was decoded.
 * loc names the memory of both `in` and out_affine; device buffers are 16-byte aligned (as reef_normalize's out_compressed). */
reef_status reef_decompress(int curve, const uint8_t *in, size_t n, int loc, reef_affine *out_affine,
                            uint64_t *invalid, uint64_t *first_invalid);

/* Sum of n Jacobian points (multi-GPU: combine the per-rank partial MSMs after an all-gather). */
reef_status reef_sum_points(int curve, const reef_jacobian *in, size_t n, int loc, reef_jacobian *out);

/* Deterministic synthetic inputs, generated on the device (bench / tests; no file I/O):
 * bases B_i = (k0 + i*d)*G with G = (-1, 2); scalars from a SplitMix64 stream
 * (kind 0 uniform, 1 witness-like 70/20/10 mix, 2 uniform below small_bound). */
reef_status reef_gen_bases(int curve, uint64_t k0, uint64_t d, size_t n, reef_affine *out, int loc);
reef_status reef_gen_scalars(int curve, uint64_t seed, int kind, uint64_t small_bound, size_t n,
                             bool to_mont, reef_fe *out, int loc);

/* ---------------------------------------------------------------------------------------------
 * (3b) Row N2 ("next" in SURVEY.md 8f): the host sum-check of nlookup witness generation as
 * vector kernels over the scalar field of `curve` (Reef: REEF_PALLAS, i.e. Fq, the CirC modulus of
 * src/backend/r1cs_helper.rs:37-38).  All values cross the ABI as canonical integers, 32 bytes
 * little-endian -- what the reference's rug::Integer tables hold -- NOT in Montgomery form.
 * Replaces, per folding step (src/backend/r1cs.rs:2318-2385):
 *   gen_eq_table              r1cs_helper.rs:508-544  -> reef_sc_gen_eq_table
 *   linear_mle_product        r1cs_helper.rs:441-506  -> reef_sc_round_coeffs (sums, :455-476), then
 *                                                        reef_sc_fold (both tables, :491-503) with the
 *                                                        Poseidon challenge the host derived (:478-489)
 *   prover_mle_partial_eval(table, sc_rs)  :551-634   -> after the last round the folded table holds
 *                                                        the value in entry 0: reef_sc_read(ctx, 0, 1, ..)
 * The results are the reference's whatever happens inside; what happens inside when the calls come in the reference's
 * order (reset, gen_eq_table, rounds with halving pow): the EQ table of gen_eq_table is a rank-one table (two factor
 * tables) plus the lookup points and is kept as that while the rounds fold its high index bits -- nothing of 2^ell
 * entries is written for it, a round streams T only; and the first round of a step reads T through the row structure
 * reef_sc_set_table found (constant rows, rows of small entries such as document symbols).  A caller-given EQ
 * (which = 1), reef_sc_read(ctx, 1, ..) between rounds, or a round out of order: dense tables from there on.
 * ------------------------------------------------------------------------------------------- */
typedef struct reef_sc_ctx reef_sc_ctx;
/* Two resident tables (T = lookup table or document, EQ) of table_len = 2^ell entries each. */
reef_status reef_sc_create(reef_sc_ctx **out, int curve, size_t table_len);
void reef_sc_destroy(reef_sc_ctx *ctx);
/* which: 0 = T, 1 = EQ.  n <= table_len values; the rest is zero-padded (r1cs.rs:2323-2330). */
reef_status reef_sc_set_table(reef_sc_ctx *ctx, int which, const reef_fe *values, size_t n, int loc);
/* T from what the caller knows it to be: runs of field elements, of one repeated value, of document symbols.  Reef's tables
 * are such runs -- "nldoc" (r1cs.rs:2322-2329): [SYMBOLS doc]; "nlhybrid" (r1cs.rs:2101-2112, :481-484): [FE table,
 * FILL calc_fill x (half - |table|), SYMBOLS proj_doc] -- and a host symbol part uploads count * elem_bytes bytes, not 32 per entry. */
enum { REEF_SC_PART_FE = 0, REEF_SC_PART_SYMBOLS = 1, REEF_SC_PART_FILL = 2 };
#define REEF_SC_MAX_PARTS 8
typedef struct {
    uint32_t kind;        /* REEF_SC_PART_*                                                         */
    uint32_t elem_bytes;  /* SYMBOLS: 1, 2 or 4 (unsigned little-endian); otherwise 0               */
    const void *data;     /* FE: count canonical 32-byte integers; SYMBOLS: count symbols;          */
                          /* FILL: ONE canonical 32-byte integer, always host memory                */
    size_t count;         /* entries of T this part covers (FILL: repetitions); 0 = part is skipped */
    int loc;              /* REEF_HOST / REEF_DEVICE for data (FE, SYMBOLS)                         */
} reef_sc_part;
/* T <- the parts laid end to end from entry 0, zero beyond their total (<= table_len).  Same effect on the ctx as
 * reef_sc_set_table(ctx, 0, ..) on the table written out as integers: same coefficients, folds, reads and reset.
 * nparts <= REEF_SC_MAX_PARTS (0: the all-zero table); device symbols are aligned to elem_bytes.  An argument error
 * (REEF_ERR_ARG) is found before anything of the ctx is touched: the table set before stays usable. */
reef_status reef_sc_set_table_parts(reef_sc_ctx *ctx, const reef_sc_part *parts, size_t nparts);
/* EQ[i] = sum_{k: qs[k] = i} rs[k] + rs[nq] * prod_j (bit_j(i) ? last_q[j] : 1 - last_q[j]);
 * rs has nq + 1 entries, last_q has ell entries (host arrays). */
reef_status reef_sc_gen_eq_table(reef_sc_ctx *ctx, const reef_fe *rs, const uint32_t *qs, size_t nq,
                                 const reef_fe *last_q, size_t ell);
/* Round with pow = 2^(ell - i): out = { xsq, x, con } (host). */
reef_status reef_sc_round_coeffs(reef_sc_ctx *ctx, size_t pow, reef_fe out[3]);
/* X[b] <- X[b]*(1 - r) + X[b + pow]*r for b < pow, both tables (asynchronous).  Only entries [0, pow) are
 * written: after a fold the tables hold `pow` live entries each, and reads or rounds that reach beyond them
 * are rejected with REEF_ERR_ARG until the table is set / reset (T) or generated (EQ) again. */
reef_status reef_sc_fold(reef_sc_ctx *ctx, size_t pow, const reef_fe *r);
/* reef_sc_fold(pow, r) and reef_sc_round_coeffs(pow / 2) in ONE pass over the tables (pow >= 2):
 * the fold of round i feeds the sums of round i+1 from registers. */
reef_status reef_sc_fold_and_next_coeffs(reef_sc_ctx *ctx, size_t pow, const reef_fe *r, reef_fe out[3]);
/* Read back the first `count` entries of a table as canonical integers (host). */
reef_status reef_sc_read(reef_sc_ctx *ctx, int which, size_t count, reef_fe *out);
/* out[j] = T[idx[j]] of the table AS LAST SET (what reef_sc_reset_table restores), canonical integers: the v_i of a step's
 * lookups (r1cs.rs:2066-2077) when the document's symbols live on the device only.  idx is a host array of k indices (repeats
 * allowed), out has k entries in host or device memory (out_loc); k = 0 is REEF_OK.  In no call order: legal before, between and
 * after rounds, the answer does not depend on how far T has been folded, and the rounds that follow run the kernels they would
 * have run without it.  An index >= table_len, or a ctx no table was set on: REEF_ERR_ARG (reef_last_error names the first such
 * index), nothing written. */
reef_status reef_sc_lookup(reef_sc_ctx *ctx, const uint64_t *idx, size_t k, reef_fe *out, int out_loc);
/* T <- the values last given to reef_sc_set_table(ctx, 0, ..): every folding step starts from the
 * unfolded table (the reference clones it per step, r1cs.rs:2320); device-to-device, asynchronous. */
reef_status reef_sc_reset_table(reef_sc_ctx *ctx);
reef_status reef_sc_sync(reef_sc_ctx *ctx);

/* ---------------------------------------------------------------------------------------------
 * (3c) Row N3: the O(N) field passes over the committed document at proof end, over the SCALAR
 *      field of `curve`.
 *
 * Replaces, in NLDocCommitment::proof_dot_prod_prover (src/backend/commitment.rs:287-405):
 *   doc_poly.evaluate(&running_q)                               commitment.rs:357
 *   the bound rows LZ = L^T Z inside hyrax_gen.prove_eval(..)   commitment.rs:371-379, :383-391
 *   (the dot-product IPA over LZ that follows runs on reef_msm / reef_ipa_cross_terms)
 * and verifier_mle_eval(table, q') of prove_consistency (commitment.rs:236; r1cs_helper.rs:637-641).
 *
 * z: the table, n entries (n <= 2^num_vars; the rest is zero padding), row-major as the
 * 2^left_vars x 2^(num_vars-left_vars) matrix Hyrax commits to (compute_factored_lens,
 * commitment.rs:173-174).  elem_bytes = 32: field elements in the same form as `point`
 * (is_mont: pasta ABI Montgomery form, else canonical integers); elem_bytes = 1, 2 or 4: unsigned
 * little-endian document symbols (framework.rs:978-1011).  point[0] pairs with the most
 * significant index bit (r1cs_helper.rs:577-592).
 *
 *   lz_out[j]  = sum_i eq(point[..left_vars], i) * z[i * 2^(num_vars-left_vars) + j]
 *   *eval_out  = sum_j lz[j] * eq(point[left_vars..], j)     (= the multilinear extension at point)
 *
 * Either output may be NULL.  Outputs are in the form `is_mont` names; eval_out is host memory.
 * Blind combination sum_i L_i * blind_i: the same call with the blinds as a one-column table
 * (num_vars = left_vars). */
reef_status reef_mle_bound_rows(int curve, const void *z, size_t n, int elem_bytes, int z_loc, bool is_mont,
                                const reef_fe *point, size_t num_vars, size_t left_vars, reef_fe *lz_out, int out_loc,
                                reef_fe *eval_out);

/* ---------------------------------------------------------------------------------------------
 * (3d) Row N4: the Poseidon Merkle commitment of the document (`--merkle`).
 *
 * Replaces MerkleCommitment::new(&doc, &pc) (src/backend/merkle_tree.rs:25-80, new_parent :82-114; built at
 * src/backend/commitment.rs:94-100) over the SCALAR field of `curve` (Reef: REEF_PALLAS, G1::Scalar):
 *   level 0, node i = H4(2i, doc[2i], 2i+1, doc[2i+1])      an odd last symbol hashes (2i, doc[2i], 0, 0)
 *   level h, node i = H2(below[2i], below[2i+1])             an odd last node hashes (below[2i], 0)
 *   H_k(x_1..x_k)   = P([tag_k, x_1, .., x_k, 0, ..])[1]     P = the Poseidon permutation of width 5 (x^5 S-box,
 *                     full_rounds/2 full rounds, partial_rounds partial rounds, full_rounds/2 full rounds; a round adds
 *                     the round constants, applies the S-box and multiplies by the MDS matrix)
 * which is what neptune's Sponge<F, U4> in Mode::Simplex computes for IOPattern [Absorb(k), Squeeze(1)] [R].  The
 * constants are the CALLER'S: round_constants, mds and the two tags are neptune's PoseidonConstants fields and the
 * domain tags its sponge API derives from the two IO patterns -- that crate is not in the reference tree, so nothing
 * here restates it.  All field elements (constants in, tree out) are canonical integers, or in the pasta Montgomery
 * form when is_mont.  `doc`: one 32-bit value per document symbol (the indices of framework.rs:978-1011).
 * tree_out (may be NULL): all levels, level 0 first, reef_merkle_nodes(n) elements; root_out (host, may be NULL). */
typedef struct {
    uint32_t width;              /* state width t = arity + 1; only 5 (Reef's U4) is built */
    uint32_t full_rounds;        /* R_F, even */
    uint32_t partial_rounds;     /* R_P */
    uint32_t reserved;
    const reef_fe *round_constants; /* host: width * (R_F + R_P) elements, round-major */
    const reef_fe *mds;          /* host: width * width; new[j] = sum_i state[i] * mds[i*width + j] */
    reef_fe tag_leaf;            /* state[0] of the 4-input leaf hash */
    reef_fe tag_node;            /* state[0] of the 2-input node hash */
} reef_poseidon_params;
uint64_t reef_merkle_nodes(uint64_t n);
reef_status reef_merkle_commit(int curve, const reef_poseidon_params *params, const uint32_t *doc, size_t n, int doc_loc,
                               bool is_mont, reef_fe *tree_out, int tree_loc, reef_fe *root_out);
/* The same tree built by several GPUs of ONE process (BASELINE configs[4]: the 64 MiB --merkle document on 8 GPUs; SURVEY.md 8e.1:
 * independent units).  The bottom level is cut into blocks of 2^L nodes -- the smallest L that leaves at most ndev blocks -- and block b is
 * hashed by devices[b] on a host thread of its own: a block is a subtree of the whole tree (its leaf hashes take the symbols' positions in
 * the whole document; a ragged last block keeps hashing (node, 0) up to level L as the whole tree does), so the devices exchange nothing
 * but their block's root, 32 bytes each, through the host; the levels above L are hashed from those roots on devices[0].  doc, tree_out
 * (may be NULL) and root_out (may be NULL, not both) are HOST memory: every device reads its slice of the document and writes its slices of
 * the levels over its own PCIe link.  Node for node the tree of reef_merkle_commit.  *blocks_out (may be NULL): how many blocks, hence
 * devices, the call used (a power-of-two cut: 3 devices and 2^26 bottom nodes give 2 blocks).  devices[] may repeat an ordinal. */
reef_status reef_merkle_commit_devices(int curve, const reef_poseidon_params *params, const uint32_t *doc, size_t n, bool is_mont,
                                       const int *devices, size_t ndev, reef_fe *tree_out, reef_fe *root_out, uint32_t *blocks_out);

/* (3d, continued) The same tree KEPT on one device, and the openings Reef takes from it.
 *
 * The only reader of MerkleCommitment.tree is make_wits(&merkle_lookups) (src/backend/merkle_tree.rs:116-190), once per folding step: a few
 * openings of `levels` siblings each.  A prover that holds the document rebuilds the tree on the device instead of loading it from the
 * .cmt file and never has it on the host.  reef_merkle_create builds it with reef_merkle_commit's kernels and keeps, on `device`, for the
 * life of the ctx: the document (32 bits a symbol), every level in the library's table form, the Poseidon constants and tags.  No copy
 * of the tree in the caller's form is made: 2^27 symbols hold 0.5 GiB + 4 GiB.  Argument errors are reef_merkle_commit's, and an unknown
 * device.  is_mont is remembered: it is the form of every field element the ctx hands out or takes in.
 * reef_merkle_info: the document length, L = the number of levels, reef_merkle_nodes(n), the root; each may be NULL.
 * reef_merkle_open: make_wits as arrays.  idx, symbols, opposite_idx: HOST, k entries; opposite, path: HOST, k * L entries.
 *   symbols[j]          = doc[idx[j]]
 *   opposite_idx[j]     = the document index of the leaf's sibling symbol; 0 when idx[j] is even and idx[j] + 1 >= n (:134-139)
 *   opposite[j*L]       = that symbol as a field element; 0 when missing
 *   opposite[j*L+1+h]   = tree[h][quo ^ 1], quo = idx[j] >> (h + 1), h = 0 .. L-2; 0 when quo is even and quo + 1 >= len(tree[h])
 *   path[j*L+h]         = tree[h][idx[j] >> (h + 1)], h = 0 .. L-1: the digests on the way up, the root last -- what the step circuit's
 *                         Merkle gadget recomputes as witness values (src/backend/nova.rs:392-511)
 *   l_or_r at depth h is "bit h of idx[j] is clear" and is not returned.  symbols, opposite_idx and path may be NULL; k = 0 is REEF_OK.
 *   An idx[j] >= n is REEF_ERR_ARG naming the first such j, and nothing is written.  One gather kernel, one copy back, one wait.
 * reef_merkle_read_level: nodes [first, first + count) of level `level`, to the host or the device (out_loc), in the caller's form; a
 *   range past the level's end is REEF_ERR_ARG.
 * reef_merkle_check_paths: the root recomputed from CLAIMED openings (opposite: k * L entries in reef_merkle_open's layout; all HOST),
 *   without a look at the stored tree but for its root: the loop of the reference's make_mt test (:220-256).  Depth 0 hashes
 *   H4(idx, sym, opp_idx, opp), or H4(opp_idx, opp, idx, sym) when bit 0 of idx is set; depth h >= 1 hashes H2(hash, opp), or H2(opp, hash)
 *   when bit h is set.  accept[j] = 1 when the result is the ctx's root, else 0: a failing path is REEF_OK.  REEF_ERR_ARG only for an index
 *   out of range or an opposite[] not below the modulus.  k paths up to 12 a wave cost one chain of L hashes whatever k is.
 * A ctx serialises its calls; different ctxs run concurrently. */
typedef struct reef_merkle_ctx reef_merkle_ctx;
reef_status reef_merkle_create(reef_merkle_ctx **out, int curve, const reef_poseidon_params *params, const uint32_t *doc, size_t n,
                               int doc_loc, bool is_mont, int device);
void        reef_merkle_destroy(reef_merkle_ctx *ctx);
reef_status reef_merkle_info(reef_merkle_ctx *ctx, uint64_t *n, uint32_t *levels, uint64_t *nodes, reef_fe *root);
reef_status reef_merkle_open(reef_merkle_ctx *ctx, const uint64_t *idx, size_t k, uint32_t *symbols, uint64_t *opposite_idx,
                             reef_fe *opposite, reef_fe *path);
reef_status reef_merkle_read_level(reef_merkle_ctx *ctx, uint32_t level, uint64_t first, uint64_t count, reef_fe *out, int out_loc);
reef_status reef_merkle_check_paths(reef_merkle_ctx *ctx, const uint64_t *idx, const uint32_t *symbols, const uint64_t *opposite_idx,
                                    const reef_fe *opposite, size_t k, uint32_t *accept);

/* ---------------------------------------------------------------------------------------------
 * (3e) Row N1: derivation of a commitment key from a label.
 *
 * Replaces nova-snark's CommitmentGens::new(label, n) -> from_label [R] (called at PublicParams::setup,
 * src/backend/framework.rs:297-303, and at SpartanSNARK::setup / HyraxPC::setup, src/backend/commitment.rs:146-149,
 * 176-180; once per --prove and once per --verify):
 *   stream  = SHAKE256(label), squeezed into n strings of 32 bytes                    (host: the XOF is sequential)
 *   out[i]  = hash_to_curve(stream[32 i .. 32 i + 32))                                (GPU: one generator per thread)
 * hash_to_curve is RFC 9380's: u0, u1 = hash_to_field(msg, 2) with expand_message_xmd over BLAKE2b-512 and 64-byte
 * strings per element; Q_j = iso_map(map_to_curve_simple_swu(u_j)) through the curve E': y^2 = x^3 + a x + b that is
 * 3-isogenous to y^2 = x^3 + 5; out = Q_0 + Q_1 (the Pasta curves have cofactor 1).  Everything pasta_curves fixes
 * and this repository cannot confirm from the reference tree [R] is DATA of the call: a, b, Z of the SWU map, the 13
 * coefficients of the isogeny (x_num[4], x_den[2], y_num[4], y_den[3]: highest degree first, the monic leading terms
 * of the denominators left out), the domain separation string and the byte order hash_to_field reads its 64-byte
 * strings in.  Field elements of the parameters are canonical integers of the curve's BASE field, or pasta
 * Montgomery form when is_mont; in either form each of the 16 is below that field's modulus, and a call with one that
 * is not is refused with REEF_ERR_ARG.  out: n affine points in the ABI form (identity = (0, 0)), host or device. */
typedef struct {
    reef_fe a, b, z;             /* E' and the SWU constant Z (a non-square with g(b/(Z a)) square, RFC 9380 6.6.2) */
    reef_fe iso[13];             /* x_num[4], x_den[2], y_num[4], y_den[3] */
    const uint8_t *dst;          /* host: domain separation string, at most 255 bytes */
    uint32_t dst_len;
    uint32_t little_endian;      /* 0: OS2IP big-endian strings (RFC 9380 5.2); 1: little-endian */
} reef_keygen_params;
reef_status reef_derive_generators(int curve, const uint8_t *label, size_t label_len, size_t n, const reef_keygen_params *params,
                                   bool is_mont, reef_affine *out, int out_loc);
/* SHAKE256(in) -> out_len bytes: the host half of the derivation, exported for tests and for callers that want the stream. */
void reef_shake256(const uint8_t *in, size_t in_len, uint8_t *out, size_t out_len);

/* ---------------------------------------------------------------------------------------------
 * (3f) Row N6: the vector work of one folding step, nova-snark's NIFS::prove [R] (Reef: RecursiveSNARK::prove_step,
 * src/backend/framework.rs:668-675), over the SCALAR field of the curve (Pallas: Fq, Vesta: Fp).  Per step and curve:
 *   T      = AZ1 o BZ2 + AZ2 o BZ1 - u1 CZ2 - CZ1          (o: entry-wise; the fresh instance has u2 = 1, E2 = 0)
 *   comm_T = MSM(T, key)                                   (the existing MSM path, T never leaves the device)
 *   W = W1 + r W2,  E = E1 + r T,  u = u1 + r,  X = X1 + r X2
 * Recalled layouts [R]: z = W || u || X (num_vars + 1 + num_io entries; column num_vars is u), and the matrices as
 * (row, col, value) triples, duplicates summed (R1CSShape::multiply_vec).  The points comm_W, comm_E of the folded
 * instance (two scalar multiplications) stay with the caller.
 *
 * reef_nifs_create      one context per curve and R1CS shape, on `device`; every vector stays resident there.
 * reef_nifs_set_matrix  which: 0 A, 1 B, 2 C.  Host triples in any order, row < num_cons, col < num_vars + 1 + num_io
 *                       (REEF_ERR_ARG otherwise).  The device form (CSR, coefficient classes) is built once per call.
 * reef_nifs_set_running the running relaxed instance: W (num_vars), E (num_cons; NULL: zeros), u (1), X (num_io), all
 *                       in `loc` memory.  nova's first step: E = 0, u = 1.
 * reef_nifs_commit_T    the fresh W2, X2 (loc memory): T on the device, kept resident with z2; *comm_T (HOST) = MSM of T
 *                       over `key`: a reef_msm_ctx of the same curve and device holding at least num_cons points.  The
 *                       MSM runs on the key ctx's stream (reef_msm_ctx_stream: the key ctx stays on that stream).
 * reef_nifs_fold        the four folds with the host's challenge r; valid once after every commit_T (REEF_ERR_ARG else).
 * reef_nifs_read        which: 0 W, 1 E, 2 T, 3 u, 4 X; the first `count` entries to the host, Montgomery form if to_mont.
 * reef_nifs_check_relaxed  AZ o BZ == u CZ + E on the running instance (nova's is_sat_relaxed without the commitment
 *                       check): *violations = rows that fail, *first_bad_row = the lowest of them (UINT64_MAX: none).
 * reef_nifs_commit_step  reef_nifs_commit_T and the fresh witness's commitment from ONE upload: also *comm_W2 (HOST, Jacobian) =
 *                       MSM(W2, key[0 .. num_vars)).  A host W2 crosses PCIe once, a device W2 is read once: one pass writes z2 and
 *                       the integers of W2 next to T, and the key commits the two rows as one batch of its row pipeline (a small key
 *                       that serves single rows from nibble tables takes each row that way); one host wait.  State, T, z2, the fold that
 *                       may follow and reef_nifs_read(.., 2, ..) are exactly commit_T's.  The key: same curve and device, at least
 *                       max(num_cons, num_vars) points, no window split -- REEF_ERR_ARG otherwise, naming the key's length and both
 *                       lengths it must cover, and the ctx is left as it was (no prove voided, the previous T readable).  NO BLINDS:
 *                       a CE::commit that adds blind * h adds it to the two points itself.
 * reef_nifs_commit_running  *comm_W = MSM(W, key), *comm_E = MSM(E, key) of the running instance as it stands (HOST, Jacobian; E = 0
 *                       gives the identity).  Either output may be NULL, not both.  The key rule of commit_step; no blinds.  With
 *                       check_relaxed this is nova's is_sat_relaxed.  The call READS ONLY: it is legal at any time after set_running,
 *                       between commit_T / commit_step and fold, and between any two calls of a 3g prove or a 3h opening, which go on
 *                       unchanged (the rule of reef_spartan_eval_matrices, 3k).
 * reef_nifs_check_fresh AZ2 o BZ2 == CZ2 on the fresh instance (W2, 1, X2) the ctx last took (commit_T or commit_step; before the
 *                       first, REEF_ERR_ARG), reported as check_relaxed reports; both outputs may be NULL.  Reads only, as
 *                       commit_running: it tells which step's witness is bad before the fold hides it.
 * is_mont: inputs in pasta Montgomery form, else canonical integers.  Calls on one context are serialised and return
 * with their work done. */
typedef struct reef_nifs_ctx reef_nifs_ctx;
reef_status reef_nifs_create(reef_nifs_ctx **out, int curve, size_t num_cons, size_t num_vars, size_t num_io, int device);
void reef_nifs_destroy(reef_nifs_ctx *ctx);
reef_status reef_nifs_set_matrix(reef_nifs_ctx *ctx, int which, const uint32_t *row, const uint32_t *col, const reef_fe *val, size_t nnz,
                                 bool is_mont);
reef_status reef_nifs_set_running(reef_nifs_ctx *ctx, const reef_fe *W, const reef_fe *E, const reef_fe *u, const reef_fe *X, int loc,
                                  bool is_mont);
reef_status reef_nifs_commit_T(reef_nifs_ctx *ctx, reef_msm_ctx *key, const reef_fe *W2, const reef_fe *X2, int loc, bool is_mont,
                               reef_jacobian *comm_T);
reef_status reef_nifs_fold(reef_nifs_ctx *ctx, const reef_fe *r, bool is_mont);
reef_status reef_nifs_read(reef_nifs_ctx *ctx, int which, size_t count, reef_fe *out, bool to_mont);
reef_status reef_nifs_check_relaxed(reef_nifs_ctx *ctx, uint64_t *violations, uint64_t *first_bad_row);
reef_status reef_nifs_commit_step(reef_nifs_ctx *ctx, reef_msm_ctx *key, const reef_fe *W2, const reef_fe *X2, int loc, bool is_mont,
                                  reef_jacobian *comm_W2, reef_jacobian *comm_T);
reef_status reef_nifs_commit_running(reef_nifs_ctx *ctx, reef_msm_ctx *key, reef_jacobian *comm_W, reef_jacobian *comm_E);
reef_status reef_nifs_check_fresh(reef_nifs_ctx *ctx, uint64_t *violations, uint64_t *first_bad_row);

/* ---------------------------------------------------------------------------------------------
 * (3g) Row N5: the two sum-checks of the final SNARK, nova-snark's RelaxedR1CSSNARK::prove [R] (Reef: S1 / S2,
 * src/backend/framework.rs:7-8, called from CompressedSNARK::prove :695-698), run on the running relaxed instance (W, E, u, X)
 * and the matrices of a reef_nifs_ctx as they stand at reef_spartan_begin.  Same field as 3f (the curve's SCALAR field).
 * The Keccak transcript stays with the caller: every call takes the challenge the caller squeezed after the previous one.
 *
 * Recalled facts [R], in one place (spartan/snark.rs, spartan/sumcheck.rs, r1cs.rs; correct them here if they are wrong):
 *   padding    R1CSShape::pad / RelaxedR1CSWitness::pad: the caller passes pk.S's num_cons_pad, num_vars_pad (powers of two);
 *              matrix column c >= num_vars becomes c + num_vars_pad - num_vars (u lands at num_vars_pad); rows >= num_cons
 *              are empty; W and E are zero-padded; z = W || 0 || u || X || 0 has 2 num_vars_pad entries.
 *   eq         eq(t)[i] = prod_j (bit_j(i) ? t_j : 1 - t_j), t_0 pairing with the MOST significant bit of i (EqPolynomial::evals).
 *   binding    a round binds the top variable: X[i] <- X[i] + r (X[i + n] - X[i]), i < n, n = half the table (bound_poly_var_top);
 *              r_x, r_y list the challenges in call order, so r_x[0] is the most significant bit.
 *   outer      prove_cubic_with_additive_term over eq(tau), AZ, BZ, D = u CZ + E with comb eq (AZ BZ - D), log2(num_cons_pad)
 *              rounds; a round's evaluations are {e0, e2, e3}: the sums at t = 0, 2, 3 of lo + t (hi - lo); the verifier's
 *              e1 = claim - e0; the CompressedUniPoly absorbed is the cubic through (0, e0), (1, e1), (2, e2), (3, e3) without
 *              its linear coefficient.  claims_outer = {AZ(r_x), BZ(r_x), CZ(r_x), E(r_x)}.
 *   inner      the joint claim AZ(r_x) + r BZ(r_x) + r^2 CZ(r_x); ABC[col] = sum_row eq(r_x)[row] (A + r B + r^2 C)[row][col] on
 *              the renumbered columns (compute_eval_table_sparse); prove_quad over ABC and z, log2(2 num_vars_pad) rounds, each
 *              {e0, e2} (t = 0, 2); then eval_W = W~(r_y[1..]) over num_vars_pad entries.
 *
 * reef_spartan_begin        num_cons_pad, num_vars_pad: powers of two in [2, 2^24], num_cons_pad >= num_cons, num_vars_pad >= num_vars,
 *                           num_io < num_vars_pad; tau: log2(num_cons_pad) entries.  AZ, BZ, CZ, D and eq(tau) on the device;
 *                           evals = round 0 of the outer sum-check.  May be called at any time: it starts a new prove.
 * reef_spartan_outer_round  binds with r, evals = the next round; exactly log2(num_cons_pad) - 1 calls.
 * reef_spartan_outer_claims binds with r_last; claims = {AZ(r_x), BZ(r_x), CZ(r_x), E(r_x)}.
 * reef_spartan_inner_begin  r: the joint-claim challenge; builds ABC and z; evals = round 0 of the inner sum-check.
 * reef_spartan_inner_round  binds with r, evals = the next round; exactly log2(num_vars_pad) calls.
 * reef_spartan_inner_claims binds with r_last; claims = {ABC(r_y), z(r_y), eval_W}.
 * Every challenge and tau entry must be below the modulus.  is_mont: inputs and outputs in pasta Montgomery form, else canonical
 * integers.  Outputs are HOST memory.  A call out of order -- a round before begin, one round too many or too few, any call after
 * reef_nifs_set_matrix / set_running / commit_T / fold changed the ctx since begin -- is REEF_ERR_ARG naming the call expected, and
 * changes nothing.  The calls never modify W, E, u, X, T or the NIFS state: commit_T and fold stay valid.  The workspace (five
 * tables of num_cons_pad entries, two of 2 num_vars_pad) is allocated by the first begin, grows, and is freed with the ctx. */
reef_status reef_spartan_begin(reef_nifs_ctx *ctx, size_t num_cons_pad, size_t num_vars_pad, const reef_fe *tau, bool is_mont,
                               reef_fe evals[3]);
reef_status reef_spartan_outer_round(reef_nifs_ctx *ctx, const reef_fe *r, bool is_mont, reef_fe evals[3]);
reef_status reef_spartan_outer_claims(reef_nifs_ctx *ctx, const reef_fe *r_last, bool is_mont, reef_fe claims[4]);
reef_status reef_spartan_inner_begin(reef_nifs_ctx *ctx, const reef_fe *r, bool is_mont, reef_fe evals[2]);
reef_status reef_spartan_inner_round(reef_nifs_ctx *ctx, const reef_fe *r, bool is_mont, reef_fe evals[2]);
reef_status reef_spartan_inner_claims(reef_nifs_ctx *ctx, const reef_fe *r_last, bool is_mont, reef_fe claims[3]);

/* ---------------------------------------------------------------------------------------------
 * (3h) The batched IPA opening of the final SNARK: what RelaxedR1CSSNARK::prove [R] does after the sum-checks of 3g,
 * EE::prove_batch(&[comm_E, comm_W], &[E, W], &[r_x, r_y[1..]], &[eval_E, eval_W]) in ipa_pc -- NIFSForInnerProduct's fold of
 * the two instances, then InnerProductArgument::prove -- on the vectors of the same reef_nifs_ctx, after reef_spartan_inner_claims.
 * The Keccak transcript and every point operation on commitments (comm_a = comm_E + r comm_W, q = gens_c.scale(r)) stay
 * with the caller; only challenges go in, and only points and single scalars come out.  Same field as 3f and 3g.
 *
 * Recalled facts [R], in one place (provider/ipa_pc.rs; correct them here if they are wrong):
 *   batch      the order is [E, W]: instance 1 is a1 = E with b1 = eq(r_x), instance 2 is a2 = W with b2 = eq(r_y[1..]);
 *              both are zero-padded to n = max(num_cons_pad, num_vars_pad) (InnerProductInstance / Witness ::pad).
 *   fold       cross = <a1, b2> + <a2, b1>; a = a1 + r a2, b = b1 + r b2, c = c1 + r^2 c2 + r cross (= <a, b>).
 *   labels     the NIFS challenge r (after absorbing cross), then the IPA's r (q = gens_s.scale(r)), then one challenge_r
 *              per round (after absorbing L and R).  b_vec is not absorbed by the IPA; if it is, open_read(.., 1, ..) serves.
 *   rounds     L = <a_lo, G_hi> + c_L q, R = <a_hi, G_lo> + c_R q with c_L = <a_lo, b_hi>, c_R = <a_hi, b_lo>; then
 *              a' = a_lo r + a_hi r^-1, b' = b_lo r^-1 + b_hi r, G' = r^-1 G_lo + r G_hi (gens.fold(r^-1, r)); a_hat = a[0]
 *              after log2(n) folds.
 *   gens_v     holds exactly n generators: the key of these calls.
 *
 * reef_spartan_open_begin     key: gens_v, a reef_msm_ctx of the same curve and device holding exactly n points, used until
 *                             finish.  Builds eq(r_x) and eq(r_y[1..]); *cross_term = cross.  May restart an opening.
 * reef_spartan_open_fold      the NIFS challenge r: a and b on the device; *c = <a, b>.
 * reef_spartan_open_ipa_begin q = gens_c.scale(r_ipa), affine, pasta Montgomery coordinates; round 0's L and R.
 * reef_spartan_open_ipa_round folds a and b with the round's challenge r; the next round's L and R; exactly log2(n) - 1 calls.
 * reef_spartan_open_finish    the last fold with r_last; *a_hat = a[0].
 * reef_spartan_open_read      which: 0 a, 1 b, as they stand now (n, n/2, ... entries); the first `count` to the host.
 * L and R are computed over the ORIGINAL resident key (the fold challenges go into the scalars, as reef_ipa_cross_terms does),
 * on the key ctx's stream, with c_L q and c_R q added on the device; one host wait per round, no vector crosses PCIe.
 * Every challenge must be below the modulus, the IPA's non-zero (REEF_ERR_ARG); r^-1 is computed in the library.  is_mont:
 * scalar inputs and outputs in pasta Montgomery form, else canonical integers.  Outputs are HOST memory.  A call out of order --
 * an opening call before reef_spartan_inner_claims, a round before ipa_begin, one round too many, any call after
 * reef_nifs_set_matrix / set_running / commit_T / fold changed the ctx -- is REEF_ERR_ARG naming the call expected, and changes
 * nothing; so is a key of another curve, device or length (the message names both lengths).  The calls never modify W, E, u, X,
 * T or the NIFS state: commit_T, fold and a new reef_spartan_begin stay valid.  The workspace (two eq tables, a and b) grows
 * with the first open_begin and is freed with the ctx. */
reef_status reef_spartan_open_begin(reef_nifs_ctx *ctx, reef_msm_ctx *key, bool is_mont, reef_fe *cross_term);
reef_status reef_spartan_open_fold(reef_nifs_ctx *ctx, const reef_fe *r, bool is_mont, reef_fe *c);
reef_status reef_spartan_open_ipa_begin(reef_nifs_ctx *ctx, const reef_affine *q, reef_jacobian *L, reef_jacobian *R);
reef_status reef_spartan_open_ipa_round(reef_nifs_ctx *ctx, const reef_fe *r, bool is_mont, reef_jacobian *L, reef_jacobian *R);
reef_status reef_spartan_open_finish(reef_nifs_ctx *ctx, const reef_fe *r_last, bool is_mont, reef_fe *a_hat);
reef_status reef_spartan_open_read(reef_nifs_ctx *ctx, int which, size_t count, reef_fe *out, bool to_mont);
/* The late rounds on a small key (opt-in; 0 = never, the default).  n_small: a power of two.  In the openings begun
 * (reef_spartan_open_begin) after the call, the round at which a and b reach n_small entries makes the n_small folded
 * generators a resident key of the run's own (reef_msm_ctx_create_folded from the challenges so far, bucket_groups = 1) and
 * every later L, R is computed over it with the challenges drawn since.  L and R are the same points, a_hat, c and the reads
 * the same values; an opening of n <= n_small entries never switches.  REEF_ERR_ARG: n_small not a power of two. */
reef_status reef_spartan_open_set_small_key(reef_nifs_ctx *ctx, size_t n_small);

/* ---------------------------------------------------------------------------------------------
 * (3i) The Hyrax consistency argument: NLDocCommitment::proof_dot_prod_prover -> HyraxPC::prove_eval [R]
 * (src/backend/commitment.rs:287-405, :371-391) over a document kept resident on the device, the IPA rounds run as 3h's (same
 * kernels, same cross-term MSMs over the original key).  Replaces the 3c calls of that argument (LZ back to the host, a second
 * reef_mle_bound_rows for the blinds, a third pass for doc_poly.evaluate in hybrid mode, :357) and the per-round host fold and
 * upload of a for reef_ipa_cross_terms.  The transcript and every point operation on commitments stay with the caller; only
 * challenges and blinds go in, only points and single scalars come out.  Over the SCALAR field of `curve`, as 3c.
 *
 * Recalled facts [R], in one place (HyraxPC::prove_eval, nova-snark's ipa_pc / dot-product proofs; correct them here if wrong):
 *   factoring  compute_factored_lens(num_vars) = (left, right) = (num_vars / 2, num_vars - num_vars / 2) (commitment.rs:173-174):
 *              Z is the row-major 2^left x 2^right matrix of the zero-padded document; row i was committed as C_i = <Z_i, gens_v>
 *              (+ blind_i h, HyraxPC::commit's row blinds).
 *   L and R    point[0] pairs with the most significant index bit; L = eq(point[..left]) weighs the ROWS, R = eq(point[left..])
 *              the columns.  The argument proves <LZ, R> = eval with LZ = L^T Z (2^right entries): a = LZ, b = R.
 *   comm_LZ    the prover forms comm_LZ = sum_i L_i C_i itself (the verifier can too) and its blind sum_i L_i blind_i;
 *              reef_hyrax_eval_comm / lz_blind serve it when the fork does, and cost nothing when it does not.
 *   rounds     as 3h: L = <a_lo, G_hi> + c_L q, R = <a_hi, G_lo> + c_R q, c_L = <a_lo, b_hi>, c_R = <a_hi, b_lo>; a' = a_lo r +
 *              a_hi r^-1, b' = b_lo r^-1 + b_hi r; a_hat = a[0] after right folds.  q = gens_1.scale(challenge) is the caller's.
 *   blinding   plain ipa_pc rounds have no blinding term (h NULL).  A bullet-style reading (Reef's verifier takes a hiding
 *              v_commit, commitment.rs:477-492) adds bl h to L and br h to R with fresh blinds per round: pass h and the blinds.
 *
 * reef_hyrax_create     z: n <= 2^num_vars entries (the rest is zero padding), elem_bytes 1 / 2 / 4 (unsigned document symbols) or
 *                       32 (field elements in the form is_mont names), on the host or the device (z_loc); copied, kept resident
 *                       for the life of the ctx.  1 <= left_vars < num_vars <= 28, and the matrix must fit one pass of 3c's
 *                       bound-rows kernel (at most 65535 row chunks: every left_vars <= 15 does; REEF_ERR_ARG otherwise).
 *                       row_blinds: 2^left_vars entries (is_mont form; then left_vars <= 25), or NULL (zeros).  device: the
 *                       ordinal of everything on this ctx.
 * reef_hyrax_eval_begin point: num_vars entries.  key: gens_v, a reef_msm_ctx of the same curve and device holding exactly
 *                       2^(num_vars - left_vars) points, used until finish.  a = LZ and b = R on the device; *eval = <LZ, R>
 *                       (= doc_poly.evaluate(point)), *lz_blind = sum_i L_i blind_i (either may be NULL).  May be called at any
 *                       time: it starts the argument over (a second eval_begin mid-argument is a restart, not an error).
 * reef_hyrax_eval_comm  optional, any time after eval_begin: *comm_lz = sum_i L_i row_comms[i] over the 2^left_vars row commitments
 *                       (affine, host or device per loc), one MSM on the device on a plain key of this ctx's device.  The
 *                       key is rebuilt from row_comms (one upload of 2^left_vars points) unless they are the host bytes of the
 *                       previous call; device row_comms are uploaded every time.
 * reef_hyrax_eval_comm_compressed  the same from the rows as Reef holds them (PolyCommit.comm, what a .cmt file holds): 2^left_vars x 32
 *                       bytes, host or device (16-byte aligned).  Decoded on the ctx's device (reef_decompress's kernel) straight into the
 *                       buffer the key is built from: no affine point visits the host.  The same host bytes as the previous call skip the
 *                       decode and the re-key.  An invalid row is REEF_ERR_ARG naming the first such row; the ctx stays usable and keeps
 *                       the row commitments it had.
 * reef_hyrax_commit     HyraxPC::commit (commitment.rs:187) of the resident document: C_i = <Z_i, key> (+ blind_i h) for every row i < 2^left_vars
 *                       of the zero-padded matrix.  key: gens_v as eval_begin takes it (same curve and device, exactly 2^(num_vars - left_vars)
 *                       points, any kind; no window split).  h: host, affine, pasta Montgomery coordinates; given exactly when create took
 *                       row_blinds.  comms32: 2^left_vars x 32 bytes in reef_normalize's encoding (the identity: 32 zero bytes);
 *                       comms_affine: the same rows as affine points (the identity: (0, 0)); both where out_loc says (device buffers
 *                       16-byte aligned), either or both NULL.  The rows stay on the device as the ctx's own row commitments (the
 *                       plain key of eval_comm, made or re-keyed device to device).  The symbol width is no argument: for elem_bytes
 *                       1 / 2 / 4 the bit length of the largest resident symbol is measured on the device, once per ctx, and the rows
 *                       take reef_msm_rows_symbols[_wide]'s route at that width; elem_bytes 32 takes reef_msm_rows' with
 *                       max_scalar_bits = 0.  A row wholly beyond n is blind_i h, or the identity.  In no call order: legal any time
 *                       after create, also between two IPA rounds, and it changes nothing of an argument in flight.  Any error
 *                       (REEF_ERR_ARG: a key of another curve, device or length -- the message names both lengths --, a window split, h
 *                       without blinds or blinds without h, a misaligned device output, a limit of the row route in its own words)
 *                       leaves the ctx usable with the row commitments it had.
 * reef_hyrax_eval_comm_own  reef_hyrax_eval_comm over the ctx's own rows: no argument, no upload.  After eval_begin, as eval_comm.
 *                       REEF_ERR_ARG naming reef_hyrax_commit when the ctx has never committed, or when a later
 *                       reef_hyrax_eval_comm[_compressed] replaced the rows.
 * reef_hyrax_ipa_begin  q: affine, pasta Montgomery coordinates; h: the optional blinding point, blinds[2]: its blinds for round 0
 *                       (the term is on when both are given, for the whole argument); round 0's L and R.
 * reef_hyrax_ipa_round  folds a and b with r; the next round's L and R; blinds: that round's two blinds (NULL = zeros; an error
 *                       when ipa_begin took no h); exactly right - 1 calls.
 * reef_hyrax_finish     the last fold with r_last; *a_hat = a[0], *b_hat = b[0] (b_hat may be NULL).
 * reef_hyrax_read       which: 0 a, 1 b, as they stand now (2^right, 2^(right-1), ... entries); the first `count` to the host.
 * Every challenge, blind and point entry must be below the modulus, the IPA's challenges non-zero (REEF_ERR_ARG).  is_mont: scalar
 * inputs and outputs in pasta Montgomery form, else canonical integers.  Outputs are HOST memory.  A call out of order -- a round
 * before ipa_begin, one round too many, finish too early, anything but eval_begin or commit before the first eval_begin -- is REEF_ERR_ARG
 * naming the call expected, and changes nothing; so is a key of another curve, device or length (the message names both lengths).
 * L and R are computed on the key ctx's stream with c_L q, c_R q (and bl h, br h) added on the device: one host wait per round. */
typedef struct reef_hyrax_ctx reef_hyrax_ctx;
reef_status reef_hyrax_create(reef_hyrax_ctx **out, int curve, const void *z, size_t n, int elem_bytes, int z_loc, bool is_mont, size_t num_vars,
                              size_t left_vars, const reef_fe *row_blinds, int device);
void reef_hyrax_destroy(reef_hyrax_ctx *ctx);
reef_status reef_hyrax_eval_begin(reef_hyrax_ctx *ctx, reef_msm_ctx *key, const reef_fe *point, bool is_mont, reef_fe *eval, reef_fe *lz_blind);
reef_status reef_hyrax_eval_comm(reef_hyrax_ctx *ctx, const reef_affine *row_comms, int loc, reef_jacobian *comm_lz);
/* reef_hyrax_eval_comm from the rows as Reef holds them (PolyCommit.comm): 2^left_vars x 32 bytes, host or device. */
reef_status reef_hyrax_eval_comm_compressed(reef_hyrax_ctx *ctx, const uint8_t *row_comms32, int loc, reef_jacobian *comm_lz);
/* The row commitments of the resident document, kept on the ctx and handed out; comm_LZ over them. */
reef_status reef_hyrax_commit(reef_hyrax_ctx *ctx, reef_msm_ctx *key, const reef_affine *h, uint8_t *comms32, reef_affine *comms_affine, int out_loc);
reef_status reef_hyrax_eval_comm_own(reef_hyrax_ctx *ctx, reef_jacobian *comm_lz);
reef_status reef_hyrax_ipa_begin(reef_hyrax_ctx *ctx, const reef_affine *q, const reef_affine *h, const reef_fe *blinds, bool is_mont,
                                 reef_jacobian *L, reef_jacobian *R);
reef_status reef_hyrax_ipa_round(reef_hyrax_ctx *ctx, const reef_fe *r, const reef_fe *blinds, bool is_mont, reef_jacobian *L, reef_jacobian *R);
reef_status reef_hyrax_finish(reef_hyrax_ctx *ctx, const reef_fe *r_last, bool is_mont, reef_fe *a_hat, reef_fe *b_hat);
reef_status reef_hyrax_read(reef_hyrax_ctx *ctx, int which, size_t count, reef_fe *out, bool to_mont);
/* The same switch as reef_spartan_open_set_small_key for the arguments begun (reef_hyrax_eval_begin) after the call. */
reef_status reef_hyrax_set_small_key(reef_hyrax_ctx *ctx, size_t n_small);

/* ---------------------------------------------------------------------------------------------
 * (3p) The Hyrax consistency arguments (3i) of many proofs over ONE resident document, advanced in lock-step: a prover that keeps a
 * committed document resident and proves m regexes over it runs m arguments whose rounds are independent given their own challenges.
 * A batch advances all of them one round per call, with one host wait per call for the whole batch: the folds of all proofs are one
 * launch (the proof index in the grid), the 2 m cross terms L_i, R_i one pass of the row pipeline (reef_msm_rows' route for the key's
 * kind, rows = 2 m over the original key), the blind terms one launch.
 *
 * Proof i of a batch is, output for output, what 3i returns for points[i] alone with the same q, h, blinds and challenges: evals,
 * lz_blinds, a_hat, b_hat and read bit for bit, L and R as points (their 32-byte encodings).  All conventions are 3i's.
 *
 * reef_hyrax_batch_create      borrows doc's resident document -- z, the row blinds, the factoring, the device -- and copies none of
 *                              it: doc must outlive the batch.  The batch keeps buffers of its own (a and b as m_max x 2^right
 *                              entries, the expanded scalars, the block sums, the per-proof tables; they only grow) and never touches
 *                              doc's single-argument state: an argument in flight through reef_hyrax_* on the same ctx continues bit
 *                              for bit, reef_hyrax_commit stays legal at any time, and calls on a batch and on its doc serialise.
 *                              REEF_ERR_ARG: m_max > 4096; m_max 2^right > 2^24 entries (the message names both numbers).
 * reef_hyrax_batch_eval_begin  points: m x num_vars entries, point after point; key as reef_hyrax_eval_begin takes it (same curve and
 *                              device, exactly 2^right points, any kind, no window split).  evals[i] = <LZ_i, R_i>, lz_blinds[i] =
 *                              sum_j L_ij blind_j (either may be NULL).  One upload, the document pass of one point after the other
 *                              on the stream, one wait.  May come at any time: it starts the batch over, with any m <= m_max.
 * reef_hyrax_batch_ipa_begin   q: one point per proof (each proof's own transcript challenge); h: ONE point for the whole batch (the
 *                              key's blinding generator) or NULL; with h, blinds holds 2 m entries (blinds[2 i], blinds[2 i + 1]:
 *                              proof i's for L and R), here and in every round call (NULL there: zeros).  L[i], R[i]: round 0's.
 * reef_hyrax_batch_ipa_round   r: one non-zero challenge per proof; exactly right - 1 calls.
 * reef_hyrax_batch_finish      the last fold with r_last[i]; a_hat[i] = a_i[0], b_hat[i] = b_i[0] (b_hat may be NULL).
 * reef_hyrax_batch_read        which: 0 a, 1 b of proof `proof` as they stand; the first `count` to the host.  From eval_begin on.
 *
 * m = 0: REEF_OK with no device work and nothing written.  REEF_ERR_ARG writes nothing, leaves the batch usable and names the proof
 * index where there is one: everything 3i rejects, per proof; m > m_max; a key of another curve, device or length; a window split on
 * the key; h without blinds.  A call out of order is REEF_ERR_ARG naming the next call, and changes nothing.
 * Out of scope: the folded small key (reef_hyrax_set_small_key: folded keys differ per proof); comm_LZ of the batch (the prover holds
 * the rows: reef_hyrax_vk_comm_lz serves it); points, q or challenges in device memory; batches over several documents or devices. */
typedef struct reef_hyrax_batch reef_hyrax_batch;
reef_status reef_hyrax_batch_create(reef_hyrax_batch **out, reef_hyrax_ctx *doc, size_t m_max);
void reef_hyrax_batch_destroy(reef_hyrax_batch *b);
reef_status reef_hyrax_batch_eval_begin(reef_hyrax_batch *b, reef_msm_ctx *key, const reef_fe *points /* m x num_vars */, size_t m, bool is_mont,
                                        reef_fe *evals /* m */, reef_fe *lz_blinds /* m, may be NULL */);
reef_status reef_hyrax_batch_ipa_begin(reef_hyrax_batch *b, const reef_affine *q /* m */, const reef_affine *h /* one, may be NULL */,
                                       const reef_fe *blinds /* 2 m, with h */, bool is_mont, reef_jacobian *L /* m */, reef_jacobian *R /* m */);
reef_status reef_hyrax_batch_ipa_round(reef_hyrax_batch *b, const reef_fe *r /* m */, const reef_fe *blinds /* 2 m or NULL */, bool is_mont,
                                       reef_jacobian *L /* m */, reef_jacobian *R /* m */);
reef_status reef_hyrax_batch_finish(reef_hyrax_batch *b, const reef_fe *r_last /* m */, bool is_mont, reef_fe *a_hat /* m */,
                                    reef_fe *b_hat /* m, may be NULL */);
reef_status reef_hyrax_batch_read(reef_hyrax_batch *b, size_t proof, int which, size_t count, reef_fe *out, bool to_mont);

/* ---------------------------------------------------------------------------------------------
 * (3j) The verifier's half of an inner-product argument: the check EE::verify_batch ends CompressedSNARK::verify with [R] and
 * HyraxPC::verify_eval makes inside verify_consistency (src/backend/commitment.rs:446-492).  Two stateless calls on a reef_msm_ctx
 * that holds gens_v: no handle of their own, no call order.  The transcript, the sum-check verification and the matrix evaluations
 * stay with the caller; the proof's points and scalars go in, a verdict comes out, and no n-entry vector crosses PCIe.
 *
 * With k = log2(n), round 0 pairing with the MOST significant index bit (3h's folds):
 *   s_j    = prod_i (bit_{k-1-i}(j) ? rs[i] : rs[i]^-1)
 *   P_hat  = comm + c q + sum_i rs[i]^2 L[i] + sum_i rs[i]^-2 R[i]
 *   G_hat  = sum_{j<n} s_j key[j]            (the first n points of the key; n <= key length)
 *   b_hat  = sum_{j<b_len} s_j b[j]          (b zero-padded to n)
 *   accept = [ P_hat == a_hat G_hat + (a_hat b_hat) q (+ blind h) ]   as group elements
 *
 * reef_ipa_check     b: b_len <= n entries in the form is_mont names, host or device (b_loc).  comm, L, R (k each): Jacobian, pasta
 *                    Montgomery coordinates, any Z; q, h: affine.  c, rs (k), a_hat, blind: host scalars.  h and blind: both NULL (no
 *                    blind term) or both given.  *accept: 1 or 0.  p_hat, g_hat, b_hat: the intermediates, each may be NULL.
 * reef_ipa_check_eq  the same with b built on the device: b = sum_t weights[t] pad(eq(points[t])), npoints 1 or 2, eq(p) of 2^vars[t]
 *                    <= n entries with p[0] pairing with the most significant bit.  b = eq(r_x) + r eq(r_y[1..]) is 3h's opening,
 *                    b = eq(point[left..]) 3i's.  points, vars, weights: host.
 * A proof that does not verify is REEF_OK with *accept = 0, not an error.  REEF_ERR_ARG, with nothing written: a challenge that is
 * zero or not below the modulus, any HOST scalar not below the modulus, n not a power of two >= 2 or beyond the key length, h without
 * blind or blind without h, a device b that is not 16-byte aligned, a key ctx with a window split set
 * (reef_msm_ctx_set_window_split: its MSMs are partial sums).  The calls take no curve: the key's curve is the call's, so scalars of
 * the other curve's field are caught only where they are not below this one's modulus.  A b in DEVICE memory is not checked: its
 * entries are reduced modulo the field's modulus as they are read.  Outputs are HOST memory, scalars in the form is_mont names.
 * The s vector, b_hat and the G_hat MSM (whatever kind of key: plain, pre-shifted, byte tables, small) run on the key ctx's stream.
 * The 2k + 4 one-off points run beside them on a second stream: made affine on the device, imported into a small plain key the key
 * ctx keeps for this (made by the first call), one MSM over it -- two when p_hat is asked for.  With g_hat asked for, a_hat G_hat is
 * a 255-step chain after the MSM (~2 ms more); otherwise a_hat rides in s.  The comparison needs no inversion; one host wait. */
reef_status reef_ipa_check(reef_msm_ctx *key, size_t n, const reef_jacobian *comm, const reef_fe *c, const reef_affine *q, const reef_jacobian *L,
                           const reef_jacobian *R, const reef_fe *rs, const reef_fe *a_hat, const reef_fe *b, size_t b_len, int b_loc,
                           const reef_affine *h, const reef_fe *blind, bool is_mont, uint32_t *accept, reef_jacobian *p_hat, reef_jacobian *g_hat,
                           reef_fe *b_hat);
reef_status reef_ipa_check_eq(reef_msm_ctx *key, size_t n, const reef_jacobian *comm, const reef_fe *c, const reef_affine *q, const reef_jacobian *L,
                              const reef_jacobian *R, const reef_fe *rs, const reef_fe *a_hat, const reef_fe *const *points, const size_t *vars,
                              const reef_fe *weights, size_t npoints, const reef_affine *h, const reef_fe *blind, bool is_mont, uint32_t *accept,
                              reef_jacobian *p_hat, reef_jacobian *g_hat, reef_fe *b_hat);

/* ---------------------------------------------------------------------------------------------
 * (3k) The verifier's matrix evaluations: what RelaxedR1CSSNARK::verify [R] ends with, A~(r_x, r_y), B~(r_x, r_y), C~(r_x, r_y), on the
 * matrices a reef_nifs_ctx holds.  With 3j this is the verifier's device work; the transcript and the O(log n) sum-check verification stay
 * with the caller.  For M = A, B, C as given to reef_nifs_set_matrix (duplicates summed), ell_x = log2(num_cons_pad), ell_y =
 * log2(2 num_vars_pad) and col' = col for col < num_vars, col + num_vars_pad - num_vars otherwise (R1CSShape::pad [R], 3g):
 *
 *   M~(r_x, r_y) = sum_entries val eq(r_x)[row] eq(r_y)[col']        (eq as 3g: index 0 of a point pairs with the most significant bit)
 *
 * r_x: ell_x entries, r_y: ell_y entries, evals = {A~, B~, C~}: HOST memory, in the form is_mont names.  num_cons_pad, num_vars_pad:
 * reef_spartan_begin's rule.  Every entry must be below the modulus; 0 and 1 are legal.  REEF_ERR_ARG, with nothing written and the ctx
 * usable: a null pointer, an illegal pad, an entry not below the modulus, a matrix not yet set.
 * The call needs the three matrices only: no reef_nifs_set_running (a verifier has no witness).  It may come at any time, between any
 * two calls of a 3g prove or a 3h opening on the same ctx: it reads no table of theirs and changes neither their phase nor the NIFS
 * state, and is in no call order.  After a reef_nifs_set_matrix the next call sees the new matrix.  Its workspace (num_cons + num_vars
 * + 1 + num_io field elements and the block sums -- none of 3g's tables) is made by the first call, grows, and is freed with the ctx.
 * One pass over the entries: a row's three dot products with eq(r_y)[col'] (the row pass of 3f: +-1 coefficients are additions), three
 * products with eq(r_x)[row], a sum over the rows.  One host wait; three field elements cross PCIe. */
reef_status reef_spartan_eval_matrices(reef_nifs_ctx *ctx, size_t num_cons_pad, size_t num_vars_pad, const reef_fe *r_x, const reef_fe *r_y,
                                       bool is_mont, reef_fe evals[3]);

/* ---------------------------------------------------------------------------------------------
 * (3l) A document's bytes -> alphabet symbols: Reef's doc_transform [R] (src/backend/framework.rs:978-1011) over the characters
 * read_doc / BaseParser::read_file hand it (src/main.rs:162-174, src/config.rs:216-284, transforms :290-420), on the device.  The file's
 * bytes cross PCIe once, as they are; the symbols are written in device memory in the width the next call wants (reef_hyrax_create:
 * 1 / 2 / 4; reef_merkle_create, the SYMBOLS part of reef_sc_set_table_parts: 4).  Stateless, on the calling thread's current device.
 *
 *   out[0 .. kept)        map[c] for every kept character c, in document order
 *   out[kept]             eof_symbol         (EOF first, then EPSILON: framework.rs:997-1003)
 *   out[kept + 1]         epsilon_symbol
 *   out[kept + 2 .. padded)   0
 *
 * Elements are elem_bytes (1, 2 or 4) wide.  text: nbytes bytes at text_loc; out: room for out_cap elements at out_loc; device buffers
 * 16-byte aligned.  map (HOST memory, map_len entries) is indexed by the byte value (REEF_DOC_BYTES) or by the code point
 * (REEF_DOC_UTF8); an entry is a symbol, REEF_DOC_DROP (the character is filtered out) or REEF_DOC_BAD (not in the alphabet); a
 * character beyond map_len is BAD.  map == NULL is the encoding's own alphabet, and no table is read: BYTES is the identity on 0..127
 * and BAD above (AsciiParser); UTF8 is Utf8Parser's alphabet order, cp below 0xD800 and cp - 0x800 from 0xE000 up.  In both, character
 * 0x1A gives eof_symbol (framework.rs:986 inserts it last and the insert overrides the alphabet's own entry).
 * padded is the plain next power of two of kept + 2.  The reference's logmn goes through f32 (costs.rs:10-15): for kept + 2 just above
 * 2^24 (16 777 217, for one) it rounds down and doc_transform then underflows, so the reference cannot run those lengths; that quirk is
 * NOT reproduced here.
 * UTF-8 follows Rust's rule (read_to_string): overlong forms, surrogates (ED A0..BF ..), values above U+10FFFF, the bytes C0, C1 and
 * F5..FF as lead bytes, truncated sequences and stray continuation bytes are malformed; malformed_at is Utf8Error::valid_up_to().
 *
 * REEF_OK whenever the text was examined.  If malformed_at < nbytes or bad > 0 nothing is written to out and info says why (bad and
 * first_bad are defined only for well-formed text).  out == NULL measures only: info is filled, nothing is written.  info may be NULL.
 * REEF_ERR_ARG: a null text with nbytes > 0; an unknown encoding or location; elem_bytes outside {1, 2, 4}; a device buffer that is not
 * 16-byte aligned; nbytes >= 2^32; a map entry, eof_symbol or epsilon_symbol that does not fit elem_bytes (a given map is checked on
 * the host; for a NULL map the limit follows from the encoding: 1 byte holds BYTES, UTF8 needs 4) -- all found before the device is
 * touched -- and out_cap < padded, with info filled first and both numbers in the message.
 * Three launches (count the kept characters per 4096-byte tile; scan the counts; decode again, map, write) and the tail; two host waits
 * (info before anything is written; the end).  No workgroup waits for another. */
enum { REEF_DOC_BYTES = 0,   /* one character per byte: AsciiParser / DnaParser, `i as char` (config.rs:229-284) */
       REEF_DOC_UTF8  = 1 }; /* Utf8Parser: read_to_string + chars() (config.rs:252-264) */
#define REEF_DOC_DROP 0xFFFFFFFEu   /* map entry: the character is filtered out (a transform whose apply() gives None) */
#define REEF_DOC_BAD  0xFFFFFFFFu   /* map entry: not in the alphabet (Reef panics, framework.rs:990-992) */
typedef struct {
    uint64_t chars;         /* characters decoded */
    uint64_t kept;          /* characters not dropped */
    uint64_t padded;        /* the smallest power of two >= kept + 2 */
    uint64_t bad;           /* characters whose map entry is BAD or lies beyond map_len */
    uint64_t first_bad;     /* byte offset of the first such character; nbytes when none */
    uint64_t malformed_at;  /* UTF-8 only: length of the longest well-formed prefix; nbytes when all of it is */
} reef_doc_info;
reef_status reef_doc_transform(const uint8_t *text, size_t nbytes, int text_loc, int encoding,
                               const uint32_t *map, size_t map_len,        /* host; NULL = the encoding's own alphabet */
                               uint32_t eof_symbol, uint32_t epsilon_symbol,
                               void *out, uint32_t elem_bytes, size_t out_cap, int out_loc, reef_doc_info *info);

/* ---------------------------------------------------------------------------------------------
 * (3m) A batch of IPA openings checked against one key in a single pass: a verifier that holds one set of public parameters and
 * checks a stream of proofs (all proofs for the same regex and document size share gens_v).  With weights rho_i the m checks of 3j
 * collapse into one equation -- the standard batch verification of inner-product arguments; nothing of the protocol changes and
 * nothing of what a single call of 3j does:
 *
 *   sum_i rho_i (comm_i + c_i q_i + sum_t rs_it^2 L_it + sum_t rs_it^-2 R_it - (a_hat_i b_hat_i) q_i - blind_i h_i)  ==  < S, key >
 *   S_j = sum_i rho_i a_hat_i s^(i)_j        (s^(i): 3j's s vector of proof i)
 *
 * One MSM over the key whatever m is, one MSM over the m (2k + 2) one-off points and the h_i of the blinded proofs, and an O(m n)
 * field pass that builds S (one launch for any m).  b_hat_i = <s^(i), b^(i)> has a closed form of O(k) products for the eq form and
 * is formed on the host, so every scalar is known before anything is enqueued.
 *
 * A reef_ipa_proof holds what reef_ipa_check_eq takes for one proof, field for field; every pointer in it is HOST memory.
 * Conventions are 3j's: round 0 pairs with the most significant index bit, is_mont names the form of every scalar (rho included),
 * points are in pasta Montgomery coordinates, any Z is legal, the identity is legal.  All m proofs are over the same n; the key must
 * hold at least n points; any kind of key is accepted (plain, pre-shifted, byte tables, small).
 *
 * rho: m HOST scalars, each non-zero and below the modulus.  They are the CALLER'S randomness, to be drawn after all m proofs are
 * fixed (from a transcript over them, or from a random source the provers cannot predict): the library draws no randomness.  An
 * accepted batch vouches for each proof only up to the usual 1/|F| over that choice; with weights a prover could foresee, errors
 * of two proofs can cancel (rho = [1, 1] accepts comm_0 + X beside comm_1 - X: that is what the equation says).
 *
 * *accept_all   1 iff the combined equation holds.  A batch that does not verify is REEF_OK with *accept_all = 0, not an error.
 * accept_each   m entries, may be NULL.  The batch accepts: every entry is 1.  The batch rejects: the call then runs the single check
 *               of 3j on each proof -- m MSMs over the key, paid ONLY on failure -- and fills the array.  NULL: nothing beyond the
 *               batch runs.
 * b_hats        m entries, may be NULL: b_hat_i, bit for bit what reef_ipa_check_eq returns for proof i alone (the form is_mont names).
 * s_comb        n entries, may be NULL: S as canonical integers, in host or device memory (s_loc; a device buffer 16-byte aligned).
 * d_comb, g_comb   may be NULL: the left and the right side of the combined equation (Jacobian, HOST memory).
 * Asking for the intermediates changes neither the verdict nor what is launched.
 *
 * m = 0: REEF_OK with *accept_all = 1, whatever the key, and no device work.  REEF_ERR_ARG, with no output touched and the key
 * usable, the message naming the proof's index where there is one: everything 3j rejects, per proof; a rho that is zero or not
 * below the modulus; a null field of a proof (h and blind excepted: both NULL or both given); npoints outside {1, 2}; a batch beyond
 * the limits m <= 4096 and m (2k + 3) <= 2^16 one-off points (the message names both numbers); a window split on the key ctx.
 * S and the MSM over the key run on the key ctx's stream.  The one-off points take 3j's route beside them on a second stream --
 * made affine, imported into a plain key of the key ctx's own, one MSM -- but on a second side key, sized to the largest batch
 * seen (grow-only, freed with the ctx); the 64-slot side key of the single calls is not touched.  The comparison needs no
 * inversion; one host wait, and accept_each's fallback comes after it.
 * reef_ipa_check_batch_last_timing: how the last batch on the key ctx divided, in device milliseconds, when it ran with the key's
 * timing on (reef_msm_ctx_enable_timing): the tables and the S pass, the MSM over the key, the one-off points (normalise, import,
 * MSM).  Each pointer may be NULL.  REEF_ERR_ARG when there was no such batch.
 * Out of scope: an explicit b vector per proof; proofs of different n in one batch; any change to the replay (its two openings are on
 * different curves and cannot share a key).  (The matrix evaluations of a batch of proofs: 3o.) */
typedef struct {
    const reef_jacobian *comm;          /* 1 */
    const reef_fe *c;                   /* 1 */
    const reef_affine *q;               /* 1 */
    const reef_jacobian *L, *R;         /* k = log2(n) each */
    const reef_fe *rs;                  /* k */
    const reef_fe *a_hat;               /* 1 */
    const reef_fe *const *points;       /* b = sum_t weights[t] pad(eq(points[t])): reef_ipa_check_eq's form, npoints 1 or 2 */
    const size_t *vars;
    const reef_fe *weights;
    size_t npoints;
    const reef_affine *h;               /* both NULL or both given, per proof */
    const reef_fe *blind;
} reef_ipa_proof;                       /* 13 pointers/sizes: 104 bytes */

reef_status reef_ipa_check_batch(reef_msm_ctx *key, size_t n, const reef_ipa_proof *proofs, size_t m, const reef_fe *rho, bool is_mont,
                                 uint32_t *accept_all, uint32_t *accept_each /* m, may be NULL */, reef_fe *b_hats /* m, may be NULL */,
                                 reef_fe *s_comb /* n, may be NULL */, int s_loc, reef_jacobian *d_comb /* may be NULL */,
                                 reef_jacobian *g_comb /* may be NULL */);
reef_status reef_ipa_check_batch_last_timing(reef_msm_ctx *key, float *s_pass_ms, float *key_msm_ms, float *side_ms);

/* ---------------------------------------------------------------------------------------------
 * (3n) The verifier's key of a committed document: comm_LZ = sum_i eq(point[..left])_i C_i of HyraxPC::verify_eval [R]
 * (commitment.rs:446-492) over the 2^left row commitments a .cmt file holds, WITHOUT a document.  3i forms the same point on a
 * reef_hyrax_ctx, which is made from z; a verifier has no z.  The rows are decoded and keyed once; every call then serves any number
 * of points -- the proofs of a batch (3m) against one document commitment -- in one pass:
 *
 *   one launch writes the m x 2^left weights eq(points[t])_i as canonical integers (3i's convention: point[0] pairs with the most
 *   significant row bit), the m MSMs go through the row pipeline (reef_msm_rows: rows = m, row_len = 2^left) over the resident key
 *   as one batch of full-width scalars, one launch encodes the m results; one host wait per call.
 *
 * row_comms32   2^left_vars x 32 bytes in reef_normalize's encoding, host or device memory (loc; a device buffer 16-byte aligned).
 *               Decoded on `device` (-1: the calling thread's current device) straight into the buffer the key is built from: no
 *               affine point visits the host.  Identity rows (32 zero bytes) are legal, as in 3i; so is a key that is all identities.
 * key_opts      as reef_msm_ctx_create's opts (NULL: the library's default key; .device is ignored).  The key is the vk's own: a
 *               window split cannot be set on it.
 * points        m x left_vars scalars, row-major, HOST memory, in the form is_mont names.  Entries 0 and 1 (weights of exactly 0
 *               and 1) are legal.
 * comm_lz       m Jacobian points, comm_lz32 their 32-byte encodings (the identity: 32 zero bytes); HOST memory, either may be NULL,
 *               not both.  The points are the same whatever route the row pipeline takes for a shape.
 *
 * m = 0: REEF_OK with nothing written.  REEF_ERR_ARG, the message naming the cause, with nothing written and the vk (if any) still
 * usable: left_vars outside 1 .. 25; a row that is not the encoding of a point (the message names the first such row and their
 * count; *out is not written); a point entry not below the modulus; a misaligned device buffer; m 2^left_vars >= 2^31; both outputs
 * NULL.  The weights and the key's workspace stay on the vk and grow on demand.  A vk serialises the calls made on it; different vks
 * are independent.  Out of scope: vks over several devices. */
typedef struct reef_hyrax_vk reef_hyrax_vk;
reef_status reef_hyrax_vk_create(reef_hyrax_vk **out, int curve, const uint8_t *row_comms32, size_t left_vars, int loc, int device,
                                 const reef_msm_opts *key_opts);
void        reef_hyrax_vk_destroy(reef_hyrax_vk *vk);
reef_status reef_hyrax_vk_comm_lz(reef_hyrax_vk *vk, const reef_fe *points, size_t m, bool is_mont, reef_jacobian *comm_lz /* m, may be NULL */,
                                  uint8_t *comm_lz32 /* 32 m bytes, may be NULL */);

/* ---------------------------------------------------------------------------------------------
 * (3o) The verifier's matrix evaluations (3k) at many points in one pass: a verifier that checks m proofs over one shape -- every
 * proof's secondary circuit; the primary circuit whenever one regex meets many documents -- needs A~, B~, C~ at m points (r_x, r_y) on
 * the same matrices.  With 3m and 3n this gives each of such a verifier's three device jobs a one-pass form.
 *
 * r_x: m x ell_x entries, point after point; r_y: m x ell_y; evals: m x {A~, B~, C~}: HOST memory, in the form is_mont names.
 * evals[3 t .. 3 t + 2] is bit for bit what reef_spartan_eval_matrices returns for point t alone.  All of 3k holds unchanged: the pad
 * rule, the matrices-only ctx (no running instance), "at any time, in no call order", no table of a prove or an opening read or
 * written, and the next call seeing a matrix replaced by reef_nifs_set_matrix.  The single call's results and launches are as before:
 * the batch keeps buffers of its own.
 *
 * m = 0: REEF_OK with no device work and nothing written.  REEF_ERR_ARG, with no output touched and the ctx usable: everything 3k
 * rejects; an entry not below the modulus (the message names the point's index and whether the entry is in r_x or r_y); m > 4096, 3m's
 * limit (the message names both numbers).
 *
 * One host wait per call, one copy up (every point's 2 (ell_x + ell_y) eq factors) and one copy down (3 m field elements).  The points
 * are taken two a thread: a matrix entry, its class and its general coefficient are read once for a pair of points (an odd last point
 * is walked alone, in the same launches).  The eq tables of one point take (num_cons + num_vars + 1 + num_io) x 32 bytes, so the call walks the points in
 * groups of G = max(1, floor(budget / bytes per point)), rounded down to an even number when above 1 and never more than m; the groups
 * follow each other on the stream with no host wait between them, each writes its results into one device array of 3 m values, and a
 * group is four launches -- six when the shape has rows of more than 128 entries -- however many points it holds.
 * reef_nifs_set_eval_workspace sets the budget in bytes; 0 restores the default of 1 GiB (a choice, not a measurement: whole batches at
 * Reef's usual shapes, 16 points a group at 2^20 rows).  A budget below one point's tables gives groups of one; it is never an error.
 * The tables' buffer grows to at most the budget, or one point's tables if that is larger (a buffer made under a larger budget is given
 * back by the next batch), and is freed with the ctx; beside it the batch keeps the eq factors, 216 bytes of block sums per 256 rows and
 * point, the long rows' segment sums and the 3 m results.
 * reef_spartan_eval_matrices_batch_last_info: the last batch on the ctx (m = 0 and failed calls do not count) -- the number of groups,
 * the points of a full group (G above), the bytes of the tables' buffer as it stands.  Each pointer may be NULL.  REEF_ERR_ARG when
 * there was no batch.
 * Out of scope: points in device memory; one batch over different shapes or ctxs; a batched prover. */
reef_status reef_spartan_eval_matrices_batch(reef_nifs_ctx *ctx, size_t num_cons_pad, size_t num_vars_pad, const reef_fe *r_x /* m ell_x */,
                                             const reef_fe *r_y /* m ell_y */, size_t m, bool is_mont, reef_fe *evals /* 3 m */);
reef_status reef_nifs_set_eval_workspace(reef_nifs_ctx *ctx, size_t bytes);
reef_status reef_spartan_eval_matrices_batch_last_info(reef_nifs_ctx *ctx, size_t *groups, size_t *points_per_group, size_t *workspace_bytes);

/* ---------------------------------------------------------------------------------------------
 * (4) Runtime plumbing.
 * ------------------------------------------------------------------------------------------- */
int reef_device_count(void);
reef_status reef_set_device(int ordinal);
reef_status reef_get_device(int *ordinal);              /* the calling thread's current device */
reef_status reef_device_sync(void);
void *reef_device_alloc(size_t bytes);                 /* hipMalloc; NULL on failure */
void reef_device_free(void *p);
reef_status reef_memcpy(void *dst, const void *src, size_t bytes, int dst_loc, int src_loc);
const char *reef_last_error(void);                     /* thread-local message of the last failure */
const char *reef_version(void);
uint32_t reef_abi_version(void);                       /* REEF_ABI_VERSION of the library that was loaded */
/* Process-wide runtime settings.  The HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware queues (4 unless set) and
 * streams that share a queue run in turn; concurrent callers of this library (the three arguments of the final SNARK, rayon workers:
 * src/backend/framework.rs:695-721) want 8.  The variable is read at the process's FIRST HIP call, so this must run before it.
 * OPT-IN (ABI 5): the library touches the environment only when asked -- hw_queues > 0 here, or REEF_MSM_HW_QUEUES=<n> exported when
 * the library is loaded; hw_queues < 0 withdraws a value the library set, 0 changes nothing.  A value the user exported as
 * GPU_MAX_HW_QUEUES is never overwritten.  info (may be NULL) reports what the environment holds and who put it there.
 *
 * warm (ABI 6): a process's first calls into HIP pay for the runtime, not for the work -- measured on a bare caller of mult_pippenger_pallas
 * (profiles/r06_seam_hip_first_use.txt): runtime initialisation 51 ms, the first stream 21 ms, the first launch of a code object 7 ms (this library
 * carries one per curve), the first copy in each direction 8 ms: ~100 ms before the first commitment of a proof whose commitments take 20-30 ms in
 * all.  Reef spends far longer than that on the host before its first MSM (regex -> SAFA, the step circuit: src/backend/framework.rs:81-166), so the
 * warm-up can hide behind it: REEF_WARM_BACKGROUND starts a thread of the library that initialises the runtime on the calling thread's CURRENT
 * device (device 0 for a thread that never chose one), creates the pool's first stream, launches one kernel of each curve's code object and moves a
 * few bytes host -> device -> host; the call returns at once, and a library call that arrives before the thread has finished simply runs beside it
 * (HIP's own locks order them).  REEF_WARM_NOW does the same before it returns.  REEF_MSM_WARM=1 in the environment asks for the background form
 * when the library is LOADED -- the zero-patch route, which has no init call.  info->warm reports 0 (never asked), 1 (running), 2 (done), 3 (failed:
 * no usable device -- the first real call will say why). */
enum { REEF_WARM_NONE = 0, REEF_WARM_NOW = 1, REEF_WARM_BACKGROUND = 2 };
typedef struct {
    int32_t hw_queues;
    uint32_t warm;                     /* REEF_WARM_* */
    uint32_t reserved[6];
} reef_runtime_opts;
typedef struct {
    int32_t hw_queues_env;             /* GPU_MAX_HW_QUEUES as the environment holds it now (0: unset) */
    int32_t hw_queues_set_by_library;  /* the value this library put there (0: it did not) */
    uint32_t abi_version;
    uint32_t warm;                     /* 0 never asked, 1 running, 2 done, 3 failed */
} reef_runtime_info;
reef_status reef_runtime_init(const reef_runtime_opts *opts /* may be NULL */, reef_runtime_info *info /* may be NULL */);

/* One MSM split by Pippenger window across `world` GPUs (north_star): every GPU holds
 * the whole key and receives all scalars, but accumulates only the windows w = rank (mod world), so
 * reef_msm / reef_msm_rows on this ctx return a PARTIAL sum; the N partial sums (96 B each) are
 * exchanged (RCCL all-gather) and added (reef_msm_ctx_sum_points).  world = 1 restores whole MSMs.
 * A Pedersen blind term is added by rank 0 only, and row commitments that go through the symbol tables
 * (no windows to split) are computed whole by rank 0, the other ranks returning the identity.
 * Clones made afterwards inherit the setting. */
reef_status reef_msm_ctx_set_window_split(reef_msm_ctx *ctx, uint32_t rank, uint32_t world);
/* Per-MSM HIP-event timing is opt-in (each event record costs ~6 us of stream time). */
reef_status reef_msm_ctx_enable_timing(reef_msm_ctx *ctx, int on);
/* Timing of the last reef_msm / reef_msm_rows on this ctx, measured with HIP events on the ctx's
 * stream (valid after a sync): total and the accumulation kernel alone, in milliseconds. */
reef_status reef_msm_ctx_last_timing(reef_msm_ctx *ctx, float *total_ms, float *accumulate_ms);
/* The same, summed over every MSM issued on this ctx since the last reset: number of calls, total
 * milliseconds and milliseconds inside the bucket-accumulation kernel (HIP events recorded on the
 * ctx's stream around each launch; the call waits for MSMs still in flight). */
reef_status reef_msm_ctx_timing_stats(reef_msm_ctx *ctx, int reset, uint64_t *calls, double *total_ms,
                                      double *accumulate_ms);
/* Which form the row / column sums of the bucket reduction took, counted over the bucket-pipeline MSMs
 * issued on this ctx since the last reset: four waves per sum (the shortest chain: what a lone MSM
 * gets), or several sums per wave (fewer instructions: taken by MSMs with a bucket matrix of 2^16 or
 * more buckets while another caller is at work on the device).  Diagnostics; both give the same point. */
reef_status reef_msm_ctx_rowcol_forms(reef_msm_ctx *ctx, int reset, uint64_t *latency_calls,
                                      uint64_t *throughput_calls);
/* Sum of n Jacobian points, enqueued on the ctx's stream (device buffers only): combines the
 * per-rank partial MSMs after an RCCL all-gather ordered on the same stream. */
reef_status reef_msm_ctx_sum_points(reef_msm_ctx *ctx, const reef_jacobian *in, size_t n, reef_jacobian *out);
/* Plan actually used by the ctx: window bits, windows, bucket groups, tables. */
reef_status reef_msm_ctx_plan(reef_msm_ctx *ctx, uint32_t *c, uint32_t *windows, uint32_t *groups,
                              uint32_t *tables);

/* Plan the engine would choose for an n-point key with the given options (pure host logic; works
 * without a GPU): window bits c, windows W = ceil(256/c), bucket groups G, tables T = ceil(W/G). */
reef_status reef_msm_plan_for(size_t n, uint32_t window_bits, uint32_t bucket_groups, uint32_t *c,
                              uint32_t *windows, uint32_t *groups, uint32_t *tables);

/* Device self-tests used by the parity suite (element-wise kernels over n inputs, HOST buffers).
 * field: 0 Fp, 1 Fq.  op: 0 mul 1 add 2 sub 3 inv 4 to_mont 5 from_mont 6 neg 7 sqr; 8 sqrt: out[i] = the root of a[i] whose canonical
 * integer is even, in the form the other ops use, or 32 bytes of 0xff when a[i] is a non-residue -- by the root reef_decompress ships
 * (fixed trip count, 4-bit windows); 9 the same by Tonelli-Shanks, the root of reef_derive_generators (same bytes; for comparison
 * and timing). */
reef_status reef_test_field_op(int field, int op, const reef_fe *a, const reef_fe *b, reef_fe *out, size_t n);
/* op: 0 mixed add P+Q, 1 general add, 2 double P, 3 k*P (k canonical in kbuf); the four-wave forms of the tail
 * kernels: 4 general add, 5 double, 6 the chain 4*(P + Q) + P, 7-10 latency probes, 11-19 every back-to-back order
 * of additions and doublings, 20 a doubling followed by an addition that falls into its own doubling (4P), 21 an addition
 * of Z = 1 operands, 22 a step machine with one addition site and one doubling site (7*(P + Q)). */
reef_status reef_test_ec_op(int curve, int op, const reef_affine *p, const reef_affine *q, const reef_fe *k,
                            reef_jacobian *out, size_t n);
/* Field-multiplication throughput probe: returns Montgomery products per second. */
reef_status reef_bench_fmul(int field, uint32_t iters, double *products_per_s);

/* ---------------------------------------------------------------------------------------------
 * (5) Device groups: the multi-GPU split behind the C ABI, in ONE process.
 *
 * Reef's prover is one Rust process (src/backend/main.rs:82; src/backend/framework.rs:81-166: two OS threads, no process
 * boundary), so what BASELINE's north_star asks for -- "large MSMs are split by Pippenger window across the 8 GPUs of one node
 * with a reduce of the partial sums over xGMI" -- has to be reachable from one address space: a group owns one resident-key
 * context per member device, issues a call on every member before it waits for any (one host thread per member: eight PCIe links
 * carry the scalars at once), brings the 96-byte partial sums together on member 0's device and adds them there.
 *
 *   REEF_SPLIT_WINDOWS  every member holds the WHOLE key (members that share a device share one copy) and receives all the
 *                       scalars; member i accumulates the Pippenger windows w = i (mod ndev) (reef_msm_ctx_set_window_split):
 *                       the split north_star names.  The rows of reef_msm_group_rows are dealt out whole on such a group.
 *   REEF_SPLIT_POINTS   member i holds points [i*n/ndev, (i+1)*n/ndev) of the key and receives that slice of every scalar
 *                       vector: 1/ndev of the key memory and of the upload per device (SURVEY.md 8e.2 "by points").
 *
 * Exchange (reef_msm_group_info.exchange): REEF_EXCHANGE_PEER -- a member on another device than member 0 sends its partial sum
 * with hipMemcpyPeerAsync on its own stream (xGMI between the GPUs of one node; peer access is enabled where the devices allow
 * it), a member on member 0's device writes it in place; member 0's stream waits for the members' events and runs the sum
 * kernel (RCCL has no elliptic-curve reduction and the payload is 96 bytes per member: latency, not bandwidth).
 * REEF_EXCHANGE_HOST -- the labelled fallback: every member's last kernel stores into its slot of host-mapped pinned memory,
 * the host waits for all members and the slots are summed on member 0's device.  gopts->exchange = 0 takes PEER.
 * REEF_EXCHANGE_RCCL -- the exchange north_star words ("an RCCL reduce of the partial sums over xGMI"), from one process: a
 * single-process communicator over the group's DISTINCT devices (ncclCommInitAll at reef_msm_group_create; RCCL is loaded at
 * run time -- librccl.so.1, or the file REEF_RCCL_LIB names -- so the library carries no link-time dependency on it, and the
 * creation FAILS, with the loader's message, where it cannot be loaded: no silent fallback).  Per call: one ncclGroup of
 * ncclSend (member i's 96 bytes, on its device's stream) / ncclRecv (member 0's device, into slot i) pairs, then the same sum
 * kernel.  RCCL offers no reduction over curve points, so the "reduce" is a gather plus k_sum_points whichever exchange is
 * chosen.  Every member but member 0 goes through a send/receive pair, also a member that shares member 0's device (a rank
 * sending to itself): a one-GPU box runs the calls an eight-GPU node runs, with other peers.
 *
 * STATUS: everything in this section has run on ONE physical device only -- groups whose members repeat ordinal 0.  The
 * branches that need two devices (hipMemcpyPeerAsync between different devices, peer-access enablement, events waited for across devices,
 * RCCL send/recv between different ranks) are HIP's and RCCL's documented calls and have never executed here: treat the section as
 * EXPERIMENTAL until it has met a multi-GPU node; reef_msm_group_enable_timing exists so that the first such run explains itself.
 *
 * devices[] may REPEAT an ordinal: a group of 2 / 3 / 8 members on device 0 runs every code path on a one-GPU box (that is how
 * tests/test_gpu_group.py covers it); members that share a device share the resident key (clones).  Results are identical to
 * reef_msm / reef_msm_rows on one context, whatever the split.  A group serialises the calls made on it.
 * Replaces, as (2) does on one device: nova-snark's CommitmentGens<G> + CE::commit [R] at src/backend/framework.rs:668-721 and
 * HyraxPC::commit at src/backend/commitment.rs:187.
 * ------------------------------------------------------------------------------------------- */
typedef struct reef_msm_group reef_msm_group;
enum { REEF_SPLIT_WINDOWS = 0, REEF_SPLIT_POINTS = 1 };
enum { REEF_EXCHANGE_DEFAULT = 0, REEF_EXCHANGE_PEER = 1, REEF_EXCHANGE_HOST = 2, REEF_EXCHANGE_RCCL = 3 };
/* How HOST scalars reach the members of a REEF_SPLIT_WINDOWS group (every member needs ALL of them: 8 x 32 MiB at 2^20 points).
 * REEF_SCALARS_EACH (default): every member uploads them from the caller's memory over its own PCIe link, all links at once.
 * REEF_SCALARS_FANOUT: ONE upload to devices[0], then every other member fetches them from there (hipMemcpyPeerAsync on its own stream, after
 * the upload's event: xGMI, 7 links x ~153 GB/s per GPU against one PCIe link per GPU shared with nothing) -- every member but member 0 goes
 * through the copy, also one that shares devices[0], so a one-GPU box runs the calls a node runs.  Which of the two wins depends on the host's
 * PCIe topology and on how much of the caller's memory is pageable; bench.py --single-process reports both.  Ignored for device scalars
 * (already a fan-out from devices[0]) and for points groups (every member uploads its own slice only). */
enum { REEF_SCALARS_EACH = 0, REEF_SCALARS_FANOUT = 1 };
typedef struct {
    uint32_t split;        /* REEF_SPLIT_* */
    uint32_t exchange;     /* REEF_EXCHANGE_* */
    uint32_t scalars;      /* REEF_SCALARS_* */
    uint32_t reserved[5];
} reef_msm_group_opts;
typedef struct {
    uint32_t members;          /* ndev */
    uint32_t distinct_devices; /* how many different ordinals devices[] named */
    uint32_t split, exchange;  /* as resolved */
    uint32_t peer_members;     /* members on another device than member 0 whose device has direct peer access to it (xGMI) */
    uint32_t reserved[3];
    uint64_t key_points[16];   /* points of the key resident on each of the first 16 members */
} reef_msm_group_info;
/* bases: the whole key, n points, on the host or on devices[0] (bases_loc).  key_opts as for reef_msm_ctx_create (its `device`
 * field is ignored: devices[] decides); 1 <= ndev <= 64. */
reef_status reef_msm_group_create(reef_msm_group **out, int curve, const reef_affine *bases, size_t n, int bases_loc,
                                  const reef_msm_opts *key_opts /* may be NULL */, const int *devices, size_t ndev,
                                  const reef_msm_group_opts *gopts /* may be NULL: windows, peer */);
void reef_msm_group_destroy(reef_msm_group *grp);
reef_status reef_msm_group_info_get(reef_msm_group *grp, reef_msm_group_info *info);
/* Where the time of a group call goes (diagnostics; round 6: the first run on several physical devices cannot be rehearsed on a one-GPU box, so
 * one call must be able to say which term is off).  With timing enabled a split call (reef_msm_group_msm, reef_msm_group_rows with rows == 1)
 * waits for every member separately before the partial sums are added -- a few microseconds of lost overlap -- and records, for the LAST call
 * (milliseconds, host clock unless said otherwise):
 *   total_ms         call entry -> result on the host
 *   distribute_ms    call entry -> every member's share enqueued (the slowest member's issue call: staging of the caller's pageable scalars,
 *                    peer fetches of device scalars, kernel launches)
 *   members_done_ms  call entry -> every member's last kernel and the send of its partial sum finished
 *   combine_ms       from there -> the sum of the partial sums on the host (k_sum_points on devices[0], one wait)
 *   member_issue_ms[i]   member i's issue call alone
 *   member_stream_ms[i]  member i's time on its stream, first enqueue to the send of its partial sum (HIP events): its share of the scalars'
 *                        way to the device, its MSM, its send
 * members beyond the 16th are not itemised. */
typedef struct {
    uint32_t members, reserved;
    double total_ms, distribute_ms, members_done_ms, combine_ms;
    double member_issue_ms[16], member_stream_ms[16];
} reef_msm_group_timing;
reef_status reef_msm_group_enable_timing(reef_msm_group *grp, int on);
reef_status reef_msm_group_last_timing(reef_msm_group *grp, reef_msm_group_timing *out);
/* K1 over the group: out (HOST) = sum_{i<n} scalars[i] * key[i], n <= key length.  scalars: host memory, or device memory of
 * devices[0] (the other devices fetch their share with peer copies). */
reef_status reef_msm_group_msm(reef_msm_group *grp, const reef_fe *scalars, size_t n, int scalars_loc, bool is_mont, reef_jacobian *out);
/* K2 over the group (REEF_SPLIT_WINDOWS groups: every member needs the first row_len points): reef_msm_rows with the rows dealt
 * out in contiguous blocks, member i computing rows [i*rows/ndev, (i+1)*rows/ndev) whole and writing them straight into out
 * (HOST): independent units, no exchange.  rows == 1 -- CE::commit with a blind -- is split by window like
 * reef_msm_group_msm, the blind term added by member 0 only.  Arguments as reef_msm_rows; scalars / blinds / h on the host or on
 * devices[0]. */
reef_status reef_msm_group_rows(reef_msm_group *grp, const reef_fe *scalars, size_t rows, size_t row_len, int scalars_loc, bool is_mont,
                                uint32_t max_scalar_bits, const reef_fe *blinds, const reef_affine *h, reef_jacobian *out);
/* The same from one-byte document symbols (reef_msm_rows_symbols). */
reef_status reef_msm_group_rows_symbols(reef_msm_group *grp, const uint8_t *symbols, size_t rows, size_t row_len, int symbols_loc,
                                        uint32_t symbol_bits, const reef_fe *blinds, const reef_affine *h, bool blinds_are_mont,
                                        reef_jacobian *out);

#ifdef __cplusplus
}
#endif
#endif /* REEF_MSM_H */
