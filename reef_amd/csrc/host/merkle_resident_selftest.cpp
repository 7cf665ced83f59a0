// Exercises MerkleCommitmentResident (reef_provider.hpp) on a seeded document and prints one JSON object: the root, the level count, the
// openings of a few lookups, the digests on their way up, and the accept flags of reef_merkle_check_paths for the honest openings and for
// two altered ones.  tests/test_gpu_merkle_resident.py recomputes every entry with the oracle and compares bit for bit.
// usage: merkle_resident_selftest [symbols]      (default 1001; doc[i] = (31 i + 7) mod 131)
// Exit codes: 0 ok, 1 a library failure, 2 a bad argument, 3 no GPU.
#include <cstdio>
#include <cstdlib>
#include <string>

#include "reef_provider.hpp"
#include "replay_standins.h"   // stand-in Poseidon constants (generated from the oracle's; NOT neptune's)

using namespace reef_provider;

static std::string fhex(const reef_fe &f) {
    static const char *d = "0123456789abcdef";
    const uint8_t *p = (const uint8_t *)&f;
    std::string s;
    for (size_t i = 0; i < 32; ++i) { s += d[p[i] >> 4]; s += d[p[i] & 15]; }
    return s;
}
static std::string flags(const std::vector<uint32_t> &a) {
    std::string j = "[";
    for (size_t i = 0; i < a.size(); ++i) j += std::string(i ? ", " : "") + std::to_string(a[i]);
    return j + "]";
}

int main(int argc, char **argv) {
    size_t n = 1001;
    if (argc > 2) { fprintf(stderr, "usage: %s [symbols]\n", argv[0]); return 2; }
    if (argc == 2) {
        char *end = nullptr;
        const unsigned long long v = strtoull(argv[1], &end, 10);
        if (!*argv[1] || *end || v < 1 || v > (1ull << 24)) { fprintf(stderr, "%s: symbols is a number from 1 to 2^24, not '%s'\n", argv[0], argv[1]); return 2; }
        n = (size_t)v;
    }
    try {
        // argument errors come before any device is looked for
        reef_merkle_ctx *none = nullptr;
        uint32_t one_doc[1] = {7};
        if (reef_merkle_create(nullptr, REEF_PALLAS, nullptr, one_doc, 1, REEF_HOST, false, 0) != REEF_ERR_ARG ||
            reef_merkle_create(&none, 9, nullptr, one_doc, 1, REEF_HOST, false, 0) != REEF_ERR_ARG || none != nullptr ||
            reef_merkle_open(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr) != REEF_ERR_ARG ||
            reef_merkle_info(nullptr, nullptr, nullptr, nullptr, nullptr) != REEF_ERR_ARG)
            throw std::runtime_error("a null or unknown argument was not refused");
        reef_merkle_destroy(nullptr);                                   // a no-op
        if (reef_device_count() < 1) { fprintf(stderr, "merkle_resident_selftest: no GPU\n"); return 3; }
        reef_poseidon_params pp;
        pp.width = 5; pp.full_rounds = STANDIN_POSEIDON_RF; pp.partial_rounds = STANDIN_POSEIDON_RP; pp.reserved = 0;
        pp.round_constants = STANDIN_POSEIDON_RC; pp.mds = STANDIN_POSEIDON_MDS;
        pp.tag_leaf = STANDIN_POSEIDON_TAGS[0]; pp.tag_node = STANDIN_POSEIDON_TAGS[1];
        std::vector<uint32_t> doc(n);
        for (size_t i = 0; i < n; ++i) doc[i] = (uint32_t)((31 * i + 7) % 131);
        MerkleCommitmentResident<REEF_PALLAS> mc(doc, pp);
        std::vector<size_t> lookups = {0, 1 % n, n / 2, n >= 2 ? n - 2 : 0, n - 1};
        std::vector<reef_fe> path;
        const auto wits = mc.make_wits(lookups, &path);
        std::string out = "{\"n\": " + std::to_string(n) + ", \"root\": \"" + fhex(mc.commitment) + "\", \"levels\": " + std::to_string(mc.levels) + ", \"lookups\": [";
        for (size_t j = 0; j < lookups.size(); ++j) out += std::string(j ? ", " : "") + std::to_string(lookups[j]);
        out += "], \"wits\": [";
        for (size_t j = 0; j < wits.size(); ++j) {
            out += std::string(j ? ", " : "") + "[";
            for (size_t h = 0; h < wits[j].size(); ++h) {
                const MerkleWit &w = wits[j][h];
                out += std::string(h ? ", " : "") + "[" + (w.l_or_r ? "true" : "false") + ", " + (w.has_idx ? std::to_string(w.opposite_idx) : "null") + ", \"" + fhex(w.opposite) + "\"]";
            }
            out += "]";
        }
        out += "], \"path\": [";
        for (size_t i = 0; i < path.size(); ++i) out += std::string(i ? ", " : "") + "\"" + fhex(path[i]) + "\"";
        out += "], \"single\": \"" + fhex(mc.path_wits(lookups[2]).back().opposite) + "\", ";
        const std::vector<uint32_t> sym = mc.symbols(lookups);
        out += "\"symbols\": " + flags(sym) + ", \"accept\": " + flags(mc.check_paths(lookups, sym, wits)) + ", ";
        auto bad = wits;                                                // one limb of the top sibling of lookup 2; the symbol of the last lookup
        bad[2].back().opposite.l[0] ^= 1;
        std::vector<uint32_t> bad_sym = sym;
        bad_sym.back() += 1;
        out += "\"accept_altered\": " + flags(mc.check_paths(lookups, bad_sym, bad)) + ", ";
        bool oob = false;
        try { mc.path_wits(n); } catch (const std::out_of_range &) { oob = true; }
        out += std::string("\"oob_throws\": ") + (oob ? "true" : "false") + "}";
        printf("%s\n", out.c_str());
        return 0;
    } catch (const std::exception &e) {
        fprintf(stderr, "merkle_resident_selftest: %s\n", e.what());
        return 1;
    }
}
