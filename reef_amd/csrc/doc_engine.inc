// Host side of reef_doc_transform (doc_kernels.inc; include/reef_msm.h 3l); included after engine.inc (ScratchStream), once: the kernels
// know no curve, and both curves' tables point here (common.h: doc_check, doc_transform).

namespace reef {

// The argument errors that do not depend on the text: found before the device is touched (api.cpp asks for the GPU after this).
reef_status doc_check(const uint8_t *text, size_t nbytes, int text_loc, int encoding, const uint32_t *map, size_t map_len, uint32_t eof_symbol,
                      uint32_t epsilon_symbol, void *out, uint32_t elem_bytes, int out_loc) {
    if (!text && nbytes) { set_error("reef_doc_transform: null text with %zu bytes", nbytes); return REEF_ERR_ARG; }
    if (encoding != REEF_DOC_BYTES && encoding != REEF_DOC_UTF8) { set_error("reef_doc_transform: unknown encoding %d", encoding); return REEF_ERR_ARG; }
    if ((text_loc != REEF_HOST && text_loc != REEF_DEVICE) || (out_loc != REEF_HOST && out_loc != REEF_DEVICE)) {
        set_error("reef_doc_transform: unknown location (text %d, out %d)", text_loc, out_loc);
        return REEF_ERR_ARG;
    }
    if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4) { set_error("reef_doc_transform: elem_bytes %u, not 1, 2 or 4", elem_bytes); return REEF_ERR_ARG; }
    if (nbytes >= (1ull << 32)) { set_error("reef_doc_transform: %zu bytes, the limit is 2^32 - 1", nbytes); return REEF_ERR_ARG; }
    if ((text_loc == REEF_DEVICE && ((uintptr_t)text & 15)) || (out && out_loc == REEF_DEVICE && ((uintptr_t)out & 15))) {
        set_error("reef_doc_transform: device buffers must be 16-byte aligned");
        return REEF_ERR_ARG;
    }
    if (map && !map_len) { set_error("reef_doc_transform: a map without entries"); return REEF_ERR_ARG; }
    if (map_len >= (1ull << 32)) { set_error("reef_doc_transform: a map of %zu entries", map_len); return REEF_ERR_ARG; }
    const u64 limit = elem_bytes == 4 ? (1ull << 32) : 1ull << (8 * elem_bytes);      // symbols are below this
    if (eof_symbol >= limit || epsilon_symbol >= limit) {
        set_error("reef_doc_transform: eof_symbol %u / epsilon_symbol %u do not fit %u byte(s)", eof_symbol, epsilon_symbol, elem_bytes);
        return REEF_ERR_ARG;
    }
    if (!map && encoding == REEF_DOC_UTF8 && elem_bytes != 4) {
        set_error("reef_doc_transform: the UTF-8 alphabet has symbols up to 0x10F7FF: elem_bytes must be 4, not %u", elem_bytes);
        return REEF_ERR_ARG;
    }
    if (map && elem_bytes != 4)
        for (size_t i = 0; i < map_len; ++i)
            if (map[i] >= limit && map[i] != REEF_DOC_DROP && map[i] != REEF_DOC_BAD) {
                set_error("reef_doc_transform: map[%zu] = %u does not fit %u byte(s)", i, map[i], elem_bytes);
                return REEF_ERR_ARG;
            }
    return REEF_OK;
}

template <int ENC>
static void doc_launch_write(hipStream_t s, u32 tiles, const uint8_t *d_text, u32 nbytes, const u32 *d_map, u32 map_len, u32 eof, const u32 *d_counts,
                             uint8_t *d_out, u32 eb) {
    if (eb == 1) hipLaunchKernelGGL((k_doc_write<ENC, 1>), dim3(tiles), dim3(DOC_THREADS), 0, s, d_text, nbytes, d_map, map_len, eof, d_counts, d_out);
    else if (eb == 2) hipLaunchKernelGGL((k_doc_write<ENC, 2>), dim3(tiles), dim3(DOC_THREADS), 0, s, d_text, nbytes, d_map, map_len, eof, d_counts, d_out);
    else hipLaunchKernelGGL((k_doc_write<ENC, 4>), dim3(tiles), dim3(DOC_THREADS), 0, s, d_text, nbytes, d_map, map_len, eof, d_counts, d_out);
}

// arguments as doc_check left them
reef_status doc_transform(const uint8_t *text, size_t nbytes, int text_loc, int encoding, const uint32_t *map, size_t map_len, uint32_t eof_symbol,
                          uint32_t epsilon_symbol, void *out, uint32_t elem_bytes, size_t out_cap, int out_loc, reef_doc_info *info) {
    const bool utf8 = encoding == REEF_DOC_UTF8;
    const u32 tiles = (u32)ceil_div((u64)nbytes, (u64)DOC_TILE);
    ScratchStream ss;
    REEF_TRY(ss.init());
    u64 stats[DOC_ST_WORDS] = {0, 0, 0, ~0ull, ~0ull};
    const uint8_t *d_text = nullptr;
    const u32 *d_map = nullptr;
    void *d_counts = nullptr, *d_stats = nullptr;
    if (nbytes) {
        REEF_TRY(stage_in<uint8_t>(ss, &d_text, text, nbytes, text_loc));
        if (map) REEF_TRY(stage_in<u32>(ss, &d_map, map, map_len, REEF_HOST));
        REEF_TRY(ss.alloc(&d_counts, 2 * (size_t)tiles * sizeof(u32)));            // the kept characters per tile, then the characters per tile
        REEF_TRY(ss.alloc(&d_stats, sizeof stats));
        REEF_HIP_TRY(hipMemsetAsync(d_stats, 0, 3 * sizeof(u64), ss.s));
        REEF_HIP_TRY(hipMemsetAsync((u64 *)d_stats + 3, 0xff, 2 * sizeof(u64), ss.s));
        if (utf8) hipLaunchKernelGGL(k_doc_count<REEF_DOC_UTF8>, dim3(tiles), dim3(DOC_THREADS), 0, ss.s, d_text, (u32)nbytes, d_map, (u32)map_len, eof_symbol, (u32 *)d_counts, (u32 *)d_counts + tiles, (unsigned long long *)d_stats);
        else hipLaunchKernelGGL(k_doc_count<REEF_DOC_BYTES>, dim3(tiles), dim3(DOC_THREADS), 0, ss.s, d_text, (u32)nbytes, d_map, (u32)map_len, eof_symbol, (u32 *)d_counts, (u32 *)d_counts + tiles, (unsigned long long *)d_stats);
        hipLaunchKernelGGL(k_doc_scan, dim3(1), dim3(DOC_SCAN_THREADS), 0, ss.s, (u32 *)d_counts, (const u32 *)d_counts + tiles, tiles, (unsigned long long *)d_stats);
        REEF_HIP_TRY(hipGetLastError());
        REEF_HIP_TRY(hipMemcpyAsync(stats, d_stats, sizeof stats, hipMemcpyDeviceToHost, ss.s));
        REEF_HIP_TRY(hipStreamSynchronize(ss.s));                          // the first host wait: kept decides padded, and whether anything is written
    }
    const u64 kept = stats[DOC_ST_KEPT];
    u64 padded = 2;
    while (padded < kept + 2) padded <<= 1;
    const bool malformed = stats[DOC_ST_MALFORMED] < nbytes, has_bad = !malformed && stats[DOC_ST_BAD] > 0;
    if (info) {
        info->chars = stats[DOC_ST_CHARS];
        info->kept = kept;
        info->padded = padded;
        info->bad = stats[DOC_ST_BAD];
        info->first_bad = has_bad ? stats[DOC_ST_FIRST_BAD] : nbytes;
        info->malformed_at = malformed ? stats[DOC_ST_MALFORMED] : nbytes;
    }
    if (malformed || has_bad || !out) return REEF_OK;
    if (out_cap < padded) {
        set_error("reef_doc_transform: out_cap %zu, the padded document has %llu symbols", out_cap, (unsigned long long)padded);
        return REEF_ERR_ARG;
    }
    uint8_t *d_out;
    REEF_TRY(stage_out<uint8_t>(ss, &d_out, out, padded * elem_bytes, out_loc));
    if (kept) {
        if (utf8) doc_launch_write<REEF_DOC_UTF8>(ss.s, tiles, d_text, (u32)nbytes, d_map, (u32)map_len, eof_symbol, (const u32 *)d_counts, d_out, elem_bytes);
        else doc_launch_write<REEF_DOC_BYTES>(ss.s, tiles, d_text, (u32)nbytes, d_map, (u32)map_len, eof_symbol, (const u32 *)d_counts, d_out, elem_bytes);
    }
    const u64 tail_dwords = (padded * elem_bytes + 3) / 4 - kept * elem_bytes / 4;
    const dim3 tail_grid((u32)std::min<u64>(4096, (tail_dwords + 255) / 256));
    if (elem_bytes == 1) hipLaunchKernelGGL(k_doc_tail<1>, tail_grid, dim3(256), 0, ss.s, d_out, kept, padded, eof_symbol, epsilon_symbol);
    else if (elem_bytes == 2) hipLaunchKernelGGL(k_doc_tail<2>, tail_grid, dim3(256), 0, ss.s, d_out, kept, padded, eof_symbol, epsilon_symbol);
    else hipLaunchKernelGGL(k_doc_tail<4>, tail_grid, dim3(256), 0, ss.s, d_out, kept, padded, eof_symbol, epsilon_symbol);
    return finish_out<uint8_t>(ss, d_out, out, padded * elem_bytes, out_loc);
}

}  // namespace reef
