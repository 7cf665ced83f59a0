// A document's bytes -> alphabet symbols (include/reef_msm.h 3l: reef_doc_transform): Reef's doc_transform [R] (src/backend/framework.rs:978-1011)
// over the characters read_doc hands it (src/config.rs:229-284), as a stream compaction in three launches.  No field arithmetic: compiled once
// (kernels_pallas.hip), reached through both curves' tables.
//
//   k_doc_count   a tile of DOC_TILE bytes per workgroup, 16 bytes per lane: decode, validate (UTF-8), look the characters up and count the ones
//                 kept -> counts[tile], the characters -> chars[tile]; bad / first_bad / malformed_at -> stats, one atomic per wave that
//                 saw something (no atomic at all on clean text: thousands of tiles adding to one word cost more than the pass)
//   k_doc_scan    one workgroup: counts -> exclusive prefix in place, its total and the sum of chars -> stats.  A launch of its own, so that
//                 no workgroup of the passes waits for another (no look-back, no flags, no spinning)
//   k_doc_write   decode and look up again, place the tile's symbols in LDS at the byte phase of their place in `out`, store whole dwords
//                 (the first and the last dword of a tile, shared with its neighbours, go out bytewise)
//   k_doc_tail    EOF, EPSILON and the zeros up to `padded`, once the host knows `kept`
//
// UTF-8 follows Rust's rule (core::str::from_utf8).  A lead byte decides alone whether its sequence is well formed: its length, its continuation
// bytes, the second-byte ranges after E0 / ED / F0 / F4.  A continuation byte is stray when the nearest non-continuation byte among the three
// before it does not cover it.  malformed_at (Utf8Error::valid_up_to) is the minimum over those local findings.  A lane therefore needs the
// three bytes before and after its sixteen; they come from the tile in LDS, and a tile reads at most three bytes beyond either end of itself,
// never outside [0, nbytes): what lies outside the text reads as 0, which neither covers a continuation byte nor continues a sequence.
#include "../../include/reef_msm.h"

namespace reef {

static constexpr u32 DOC_THREADS = 256;
static constexpr u32 DOC_TILE = DOC_THREADS * 16;      // bytes of text per workgroup
static constexpr u32 DOC_SCAN_THREADS = 1024;          // tile counts per step of k_doc_scan
static constexpr u32 DOC_DROP = 0xFFFFFFFEu, DOC_BAD = 0xFFFFFFFFu;   // REEF_DOC_DROP, REEF_DOC_BAD

// stats words (u64): what reef_doc_info is filled from
enum { DOC_ST_CHARS = 0, DOC_ST_KEPT = 1, DOC_ST_BAD = 2, DOC_ST_FIRST_BAD = 3, DOC_ST_MALFORMED = 4, DOC_ST_WORDS = 5 };

// The tile at `tile` into lds[0 .. DOC_TILE + 8): four bytes before it (three are used), the tile, four bytes after; zeros outside the text.
// Sixteen bytes per lane; the last, partial sixteen of the text and the two margins are read byte by byte.
__device__ __forceinline__ void doc_load_tile(const uint8_t *__restrict__ text, u32 nbytes, u32 tile, u32 *lds) {
    const u32 t = threadIdx.x;
    const u64 pos = (u64)tile * DOC_TILE + (u64)t * 16;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (pos + 16 <= nbytes) {
        v = *reinterpret_cast<const uint4 *>(text + pos);
    } else if (pos < nbytes) {
        u32 w[4] = {0, 0, 0, 0};
        for (u32 k = 0; k < (u32)(nbytes - pos); ++k) w[k >> 2] |= (u32)text[pos + k] << (8 * (k & 3));
        v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    lds[1 + 4 * t + 0] = v.x;
    lds[1 + 4 * t + 1] = v.y;
    lds[1 + 4 * t + 2] = v.z;
    lds[1 + 4 * t + 3] = v.w;
    if (t < 2) {                                                          // t = 0: the bytes before the tile, t = 1: after it
        const u64 from = t == 0 ? (u64)tile * DOC_TILE : (u64)(tile + 1) * DOC_TILE + 4;   // one past the margin's last byte
        u32 w = 0;
        for (u32 k = 0; k < 4; ++k) {
            const u64 p = from - 4 + k;
            if (from >= 4 && p < nbytes && (t == 0 ? k >= 1 : k <= 2)) w |= (u32)text[p] << (8 * k);     // three bytes either side
        }
        lds[t == 0 ? 0 : 1 + DOC_TILE / 4] = w;
    }
    __syncthreads();
}

// the symbol of character c (a byte value or a code point): the caller's map, or the encoding's own alphabet
template <int ENC> __device__ __forceinline__ u32 doc_symbol(u32 c, const u32 *__restrict__ map, u32 map_len, u32 eof) {
    if (map) return c < map_len ? map[c] : DOC_BAD;
    if (c == 0x1A) return eof;                                            // framework.rs:986: inserted last, overrides the alphabet's entry
    if (ENC == REEF_DOC_BYTES) return c < 128 ? c : DOC_BAD;              // AsciiParser
    return c < 0xD800 ? c : c - 0x800;                                    // Utf8Parser: every scalar value in order
}

// One lane's sixteen bytes: sym[i] for every byte i that starts a character (bit i of the result), its symbol looked up; *bad_at the lowest
// byte offset within the lane (16: none) that Rust's rule rejects.  w: the lane's six dwords of the tile, byte 4 of them its first.
template <int ENC>
__device__ __forceinline__ u32 doc_decode_lane(const u32 (&w)[6], u32 live, const u32 *__restrict__ map, u32 map_len, u32 eof, u32 (&sym)[16], u32 *bad_at) {
    u32 starts = 0;
    *bad_at = 16;
    const bool ascii = ((w[1] | w[2] | w[3] | w[4]) & 0x80808080u) == 0;
    if (ENC == REEF_DOC_BYTES || ascii) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const u32 b = (w[1 + (i >> 2)] >> (8 * (i & 3))) & 0xff;
            sym[i] = (u32)i < live ? doc_symbol<ENC>(b, map, map_len, eof) : DOC_DROP;
        }
        return live >= 16 ? 0xffffu : (1u << live) - 1;
    }
#define DOC_B(k) ((w[((k) + 4) >> 2] >> (8 * (((k) + 4) & 3))) & 0xff)
#pragma unroll
    for (int i = 15; i >= 0; --i) {                                       // downwards: *bad_at ends as the lowest offset
        const u32 b = DOC_B(i);
        sym[i] = DOC_DROP;
        if ((u32)i >= live) continue;
        if (b < 0x80) {
            starts |= 1u << i;
            sym[i] = doc_symbol<ENC>(b, map, map_len, eof);
        } else if (b < 0xC0) {
            const u32 b1 = DOC_B(i - 1), b2 = DOC_B(i - 2), b3 = DOC_B(i - 3);
            const bool c1 = (b1 & 0xC0) == 0x80, c2 = (b2 & 0xC0) == 0x80;
            const bool covered = !c1 ? b1 >= 0xC0 : !c2 ? b2 >= 0xE0 : b3 >= 0xF0;
            if (!covered) *bad_at = i;
        } else {
            const u32 n1 = DOC_B(i + 1), n2 = DOC_B(i + 2), n3 = DOC_B(i + 3);
            const u32 lo = b == 0xE0 ? 0xA0 : b == 0xF0 ? 0x90 : 0x80, hi = b == 0xED ? 0x9F : b == 0xF4 ? 0x8F : 0xBF;
            bool ok = b >= 0xC2 && b <= 0xF4 && n1 >= lo && n1 <= hi;
            u32 cp;
            if (b < 0xE0) {
                cp = (b & 0x1F) << 6 | (n1 & 0x3F);
            } else if (b < 0xF0) {
                ok = ok && (n2 & 0xC0) == 0x80;
                cp = (b & 0x0F) << 12 | (n1 & 0x3F) << 6 | (n2 & 0x3F);
            } else {
                ok = ok && (n2 & 0xC0) == 0x80 && (n3 & 0xC0) == 0x80;
                cp = (b & 0x07) << 18 | (n1 & 0x3F) << 12 | (n2 & 0x3F) << 6 | (n3 & 0x3F);
            }
            if (ok) {
                starts |= 1u << i;
                sym[i] = doc_symbol<ENC>(cp, map, map_len, eof);
            } else {
                *bad_at = i;
            }
        }
    }
#undef DOC_B
    return starts;
}

// the lane's window of the tile and how many of its sixteen bytes lie in the text
__device__ __forceinline__ u32 doc_lane_window(const u32 *lds, u32 nbytes, u32 tile, u32 (&w)[6], u64 *pos) {
    *pos = (u64)tile * DOC_TILE + (u64)threadIdx.x * 16;
#pragma unroll
    for (int k = 0; k < 6; ++k) w[k] = lds[4 * threadIdx.x + k];
    return *pos >= nbytes ? 0u : (u32)std::min<u64>(16, nbytes - *pos);
}

template <int ENC>
static __global__ void __launch_bounds__(DOC_THREADS) k_doc_count(const uint8_t *__restrict__ text, u32 nbytes, const u32 *__restrict__ map, u32 map_len,
                                                                  u32 eof, u32 *__restrict__ counts, u32 *__restrict__ chars_out,
                                                                  unsigned long long *__restrict__ stats) {
    __shared__ u32 lds[DOC_TILE / 4 + 2];
    __shared__ u32 wave_sums[DOC_THREADS / WAVE][2];
    const u32 tile = blockIdx.x;
    doc_load_tile(text, nbytes, tile, lds);
    u32 w[6], sym[16], mal;
    u64 pos;
    const u32 live = doc_lane_window(lds, nbytes, tile, w, &pos);
    const u32 starts = doc_decode_lane<ENC>(w, live, map, map_len, eof, sym, &mal);
    u32 kept = 0, bad = 0, first_bad = 16;
#pragma unroll
    for (int i = 15; i >= 0; --i) {
        const bool st = (starts >> i) & 1;
        kept += st && sym[i] != DOC_DROP;
        if (st && sym[i] == DOC_BAD) { ++bad; first_bad = i; }
    }
    u32 chars = __popc(starts);
    u64 fb = first_bad < 16 ? pos + first_bad : ~0ull, ma = mal < 16 ? pos + mal : ~0ull;
    for (int d = 32; d > 0; d >>= 1) {
        chars += __shfl_xor(chars, d, WAVE);
        kept += __shfl_xor(kept, d, WAVE);
        bad += __shfl_xor(bad, d, WAVE);
        fb = std::min<u64>(fb, (u64)__shfl_xor((unsigned long long)fb, d, WAVE));
        ma = std::min<u64>(ma, (u64)__shfl_xor((unsigned long long)ma, d, WAVE));
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        wave_sums[threadIdx.x / WAVE][0] = chars;
        wave_sums[threadIdx.x / WAVE][1] = kept;
        if (bad) {
            atomicAdd(stats + DOC_ST_BAD, (unsigned long long)bad);
            atomicMin(stats + DOC_ST_FIRST_BAD, (unsigned long long)fb);
        }
        if (ma != ~0ull) atomicMin(stats + DOC_ST_MALFORMED, (unsigned long long)ma);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        u32 c = 0, k = 0;
        for (u32 v = 0; v < DOC_THREADS / WAVE; ++v) { c += wave_sums[v][0]; k += wave_sums[v][1]; }
        counts[tile] = k;
        chars_out[tile] = c;
    }
}

// counts[0 .. n) -> their exclusive prefix sums in place, the total -> stats[DOC_ST_KEPT], the sum of chars[0 .. n) -> stats[DOC_ST_CHARS]; one
// workgroup, DOC_SCAN_THREADS counts per step
static __global__ void __launch_bounds__(DOC_SCAN_THREADS) k_doc_scan(u32 *__restrict__ counts, const u32 *__restrict__ chars, u32 n,
                                                                      unsigned long long *__restrict__ stats) {
    __shared__ u32 wave_total[DOC_SCAN_THREADS / WAVE];
    __shared__ unsigned long long wave_chars[DOC_SCAN_THREADS / WAVE];
    const u32 lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    u64 carry = 0, nchars = 0;
    for (u32 base = 0; base < n; base += DOC_SCAN_THREADS) {              // (n, and with it the trip count, is the same for every lane)
        const u32 i = base + threadIdx.x;
        const u32 v = i < n ? counts[i] : 0;
        nchars += i < n ? chars[i] : 0;
        u32 inc = v;
        for (int d = 1; d < WAVE; d <<= 1) {
            const u32 o = __shfl_up(inc, d, WAVE);
            if ((int)lane >= d) inc += o;
        }
        if (lane == WAVE - 1) wave_total[wv] = inc;
        __syncthreads();
        u32 before = 0, all = 0;
        for (u32 k = 0; k < DOC_SCAN_THREADS / WAVE; ++k) {
            const u32 t = wave_total[k];
            before += k < wv ? t : 0;
            all += t;
        }
        if (i < n) counts[i] = (u32)carry + before + inc - v;            // kept < nbytes < 2^32
        carry += all;
        __syncthreads();
    }
    for (int d = 32; d > 0; d >>= 1) nchars += (u64)__shfl_xor((unsigned long long)nchars, d, WAVE);
    if (lane == 0) wave_chars[wv] = nchars;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 all = 0;
        for (u32 k = 0; k < DOC_SCAN_THREADS / WAVE; ++k) all += wave_chars[k];
        stats[DOC_ST_KEPT] = carry;
        stats[DOC_ST_CHARS] = all;
    }
}

// out[offsets[tile] ..) = the symbols of the tile's kept characters, EB bytes each.  Only run on text that k_doc_count found well formed and
// without a BAD character.
template <int ENC, int EB>
static __global__ void __launch_bounds__(DOC_THREADS) k_doc_write(const uint8_t *__restrict__ text, u32 nbytes, const u32 *__restrict__ map, u32 map_len,
                                                                  u32 eof, const u32 *__restrict__ offsets, uint8_t *__restrict__ out) {
    __shared__ u32 lds[DOC_TILE / 4 + 2];
    __shared__ u32 stage[DOC_TILE * EB / 4 + 1];                          // the tile's symbols at the byte phase of their place in out
    __shared__ u32 wave_total[DOC_THREADS / WAVE];
    const u32 tile = blockIdx.x;
    doc_load_tile(text, nbytes, tile, lds);
    u32 w[6], sym[16], mal;
    u64 pos;
    const u32 live = doc_lane_window(lds, nbytes, tile, w, &pos);
    const u32 starts = doc_decode_lane<ENC>(w, live, map, map_len, eof, sym, &mal);
    u32 mine = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) mine += ((starts >> i) & 1) && sym[i] != DOC_DROP;
    const u32 lane = threadIdx.x & (WAVE - 1), wv = threadIdx.x / WAVE;
    u32 inc = mine;
    for (int d = 1; d < WAVE; d <<= 1) {
        const u32 o = __shfl_up(inc, d, WAVE);
        if ((int)lane >= d) inc += o;
    }
    if (lane == WAVE - 1) wave_total[wv] = inc;
    __syncthreads();
    u32 at = inc - mine, total = 0;
    for (u32 k = 0; k < DOC_THREADS / WAVE; ++k) {
        at += k < wv ? wave_total[k] : 0;
        total += wave_total[k];
    }
    const u64 g0 = (u64)offsets[tile] * EB;                               // byte offset of the tile's first symbol in out
    const u32 phase = (u32)(g0 & 3), end = phase + total * EB;            // the tile's bytes are stage bytes [phase, end)
    uint8_t *sb = reinterpret_cast<uint8_t *>(stage);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if (((starts >> i) & 1) && sym[i] != DOC_DROP) {
            if (EB == 1) sb[phase + at] = (uint8_t)sym[i];
            else if (EB == 2) *reinterpret_cast<uint16_t *>(sb + phase + 2 * at) = (uint16_t)sym[i];     // phase is even when EB is 2
            else stage[at] = sym[i];                                                                     // and 0 when EB is 4
            ++at;
        }
    }
    __syncthreads();
    uint8_t *dst = out + (g0 - phase);                                    // dword aligned: out is
    for (u32 j = threadIdx.x; 4 * j < end; j += DOC_THREADS) {
        if (4 * j >= phase && 4 * j + 4 <= end) {
            reinterpret_cast<u32 *>(dst)[j] = stage[j];
        } else {
            for (u32 k = 4 * j; k < 4 * j + 4; ++k)
                if (k >= phase && k < end) dst[k] = sb[k];
        }
    }
}

// out[kept] = eof, out[kept + 1] = epsilon, out[kept + 2 .. padded) = 0, EB bytes each, as dwords; the dwords that out's ends cut go out bytewise
template <int EB>
static __global__ void __launch_bounds__(256) k_doc_tail(uint8_t *__restrict__ out, u64 kept, u64 padded, u32 eof, u32 epsilon) {
    const u64 b0 = kept * EB, b1 = padded * EB, d0 = b0 >> 2, d1 = (b1 + 3) >> 2;
    for (u64 d = d0 + (u64)blockIdx.x * blockDim.x + threadIdx.x; d < d1; d += (u64)gridDim.x * blockDim.x) {
        u32 v = 0;
        if (4 * d < b0 + 2 * EB) {
            for (u32 k = 0; k < 4; ++k) {
                const u64 a = 4 * d + k, e = a / EB;
                const u32 s = e == kept ? eof : e == kept + 1 ? epsilon : 0;
                v |= ((s >> (8 * (u32)(a % EB))) & 0xff) << (8 * k);
            }
        }
        if (4 * d >= b0 && 4 * d + 4 <= b1) {
            reinterpret_cast<u32 *>(out)[d] = v;
        } else {
            for (u32 k = 0; k < 4; ++k)
                if (4 * d + k >= b0 && 4 * d + k < b1) out[4 * d + k] = (uint8_t)(v >> (8 * k));
        }
    }
}

}  // namespace reef
