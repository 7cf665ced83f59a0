// char_map of reef_provider.hpp against written-out expectations: pure host logic, no HIP, no library (this file's link line is the check
// that char_map calls nothing of it).  tests/test_doc_host.py runs it; exit status 0 = every expectation held.
#include <cstdio>

#include "reef_provider.hpp"

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);        \
            ++failures;                                                  \
        }                                                                \
    } while (0)

int main() {
    using reef_provider::char_map;
    {   // "abc": positions, EOF at 0x1A = len + 2, BAD elsewhere, as long as the largest code point asks
        const std::vector<uint32_t> m = char_map(U"abc");
        EXPECT(m.size() == 'c' + 1u);
        EXPECT(m['a'] == 0 && m['b'] == 1 && m['c'] == 2);
        EXPECT(m[0x1A] == 5);
        EXPECT(m[0] == REEF_DOC_BAD && m['A'] == REEF_DOC_BAD && m['`'] == REEF_DOC_BAD);
        size_t bad = 0;
        for (uint32_t v : m) bad += v == REEF_DOC_BAD;
        EXPECT(bad == m.size() - 4);
    }
    {   // the empty alphabet still has EOF
        const std::vector<uint32_t> m = char_map(U"");
        EXPECT(m.size() == 0x1B && m[0x1A] == 2 && m[0x19] == REEF_DOC_BAD);
    }
    {   // a later duplicate overrides an earlier one; the length counts every character
        const std::vector<uint32_t> m = char_map(U"abca");
        EXPECT(m['a'] == 3 && m['b'] == 1 && m['c'] == 2 && m[0x1A] == 6);
    }
    {   // 0x1A in the alphabet: the EOF insert comes last and wins
        const std::u32string ab = {U'x', char32_t(0x1A), U'y'};
        const std::vector<uint32_t> m = char_map(ab);
        EXPECT(m['x'] == 0 && m['y'] == 2 && m[0x1A] == 5);
    }
    {   // CaseInsensitive over "ABC": lowercase letters take the entry of what they become, also one that is not in the alphabet
        const std::vector<uint32_t> m = char_map(U"ABC", {{U'a', U'A'}, {U'b', U'B'}, {U'z', U'Z'}});
        EXPECT(m['A'] == 0 && m['a'] == 0 && m['b'] == 1 && m['c'] == REEF_DOC_BAD);
        EXPECT(m['z'] == REEF_DOC_BAD && m['Z'] == REEF_DOC_BAD && m.size() == 'z' + 1u);
    }
    {   // a swap is looked up before either side is written
        const std::vector<uint32_t> m = char_map(U"ab", {{U'a', U'b'}, {U'b', U'a'}});
        EXPECT(m['a'] == 1 && m['b'] == 0);
    }
    {   // IgnoreWhitespace: dropped characters, also one that the alphabet names and one that a remap targets
        const std::vector<uint32_t> m = char_map(U"a b", {{U'\t', U' '}}, U" \n");
        EXPECT(m['a'] == 0 && m['b'] == 2 && m[' '] == REEF_DOC_DROP && m['\n'] == REEF_DOC_DROP);
        EXPECT(m['\t'] == 1);                     // looked up before the drop: it becomes ' ', whose position is 1
        EXPECT(m[0x1A] == 5);
    }
    {   // beyond the BMP: the map is as long as the largest code point asks, surrogates stay BAD
        const std::u32string ab = {U'A', char32_t(0xE9), char32_t(0x20AC), char32_t(0x1F600)};
        const std::vector<uint32_t> m = char_map(ab);
        EXPECT(m.size() == 0x1F601 && m[0xE9] == 1 && m[0x20AC] == 2 && m[0x1F600] == 3 && m[0xD800] == REEF_DOC_BAD && m[0x1A] == 6);
    }
    if (failures) {
        std::printf("doc_map_selftest: %d expectation(s) failed\n", failures);
        return 1;
    }
    std::printf("doc_map_selftest ok\n");
    return 0;
}
