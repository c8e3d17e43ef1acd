// deflate_san_main.cpp -- the output compressor's core (flowgger_amd/csrc/fg_deflate.hpp) in a stand-alone program for
// -fsanitize=address,undefined: the length-by-content cases, each as a batch of its own whose input buffer ends with its last byte
// and whose output buffer holds exactly the bytes the sizing pass named, so that a read or a write one byte out is an error.  The
// program checks nothing but its own sanity (tests/test_deflate_cpu.py holds the bytes against zlib); prints the members and bytes
// it produced.  Test infrastructure.
#include <stdio.h>

#include <memory>
#include <string>
#include <vector>

#include "deflate_driver.hpp"

static std::vector<uint8_t> content(int kind, size_t n, uint32_t block) {
    std::vector<uint8_t> v(n);
    uint32_t x = 12345u + (uint32_t)n * 7u + (uint32_t)kind;
    const char* words[] = {"\"host\":\"h0123.dc4.example.com\",", "\"short_message\":\"", "pod ", "to ", "the ", "quote \\\" inside ", "\"_level\":", "net "};
    std::string text;
    while (text.size() < n + 64) {
        x = x * 1664525u + 1013904223u;
        text += words[(x >> 24) & 7u];
    }
    const std::string phrase = "the quick brown fox jumps over the lazy dog, 0123456789 times";
    for (size_t i = 0; i < n; ++i) {
        x = x * 1664525u + 1013904223u;
        switch (kind) {
            case 0: v[i] = 'a'; break;
            case 1: v[i] = 0xE9; break;
            case 2: v[i] = (uint8_t)(65 + i % 2); break;
            case 3: v[i] = (uint8_t)(65 + i % 3); break;
            case 4: v[i] = (uint8_t)(65 + i % 4); break;
            case 5: v[i] = (uint8_t)((7 * (i % 257) + 3) % 251); break;
            case 6: v[i] = (uint8_t)i; break;
            case 7: v[i] = (uint8_t)(x >> 24); break;
            case 8: v[i] = (uint8_t)text[i]; break;
            default: v[i] = '~'; break;
        }
    }
    if (kind >= 9 && n >= 2 * phrase.size()) {
        // 9: at 0 and at the end of the first block; 10: at 0 and across the block boundary
        size_t at = (n < block ? n : block) - phrase.size();
        if (kind == 10) at = n > block + phrase.size() ? block - phrase.size() / 2 + n % 5 - 2 : n - phrase.size();
        for (size_t i = 0; i < phrase.size(); ++i) v[i] = v[at + i] = (uint8_t)phrase[i];
    }
    return v;
}

int main() {
    fgd::lane_stack() = 32u << 10;  // (this process runs nothing else on the emulation; the core keeps a few dozen words on a lane's stack)
    const uint32_t B = fg::deflate::kBlock;
    const size_t lengths[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257, 258, 259, 260, 261, B - 1, B, B + 1, 2 * B - 1, 2 * B, 2 * B + 1};
    unsigned long long members = 0, bytes = 0;
    for (size_t n : lengths)
        for (int kind = 0; kind <= 10; ++kind) {
            // the member between an empty one and a short one: three cuts' worth of offsets, the input exactly as long as its bytes
            std::vector<uint8_t> in = content(kind, n, B);
            in.push_back('x');
            in.push_back('y');
            const uint64_t cuts[4] = {0, 0, n, n + 2};
            uint64_t zoff[4];
            const uint64_t total = fgd::deflate(in.data(), in.size(), cuts, 3, nullptr, 0, zoff);
            if (total == fgd::kBadArgs || total > fg::deflate::bound(in.size(), 3)) {
                fprintf(stderr, "length %zu kind %d: total %llu\n", n, kind, (unsigned long long)total);
                return 1;
            }
            std::unique_ptr<uint8_t[]> z(new uint8_t[total]);  // (exactly: the allocation ends with the last member)
            uint64_t zoff2[4];
            if (fgd::deflate(in.data(), in.size(), cuts, 3, z.get(), total, zoff2) != total || zoff2[3] != zoff[3] || zoff2[1] != 0) {
                fprintf(stderr, "length %zu kind %d: the second pass disagrees\n", n, kind);
                return 1;
            }
            members += 3;
            bytes += total;
        }
    printf("ok %llu members %llu bytes\n", members, bytes);
    return 0;
}
