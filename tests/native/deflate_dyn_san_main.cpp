// deflate_dyn_san_main.cpp -- FG_DEFLATE_DYNAMIC (compress_block_dyn, build_lengths of flowgger_amd/csrc/fg_deflate.hpp) in a stand-alone
// program for -fsanitize=address,undefined, as deflate_san_main.cpp runs the fixed mode: members of several contents and lengths, each
// a batch of its own whose input ends with its last byte and whose output holds exactly what the sizing pass named; then the code
// builder on histograms at its limits, its workspace exactly kWsBuild words.  The program checks nothing but its own sanity
// (tests/test_deflate_dynamic_cpu.py holds the bytes against zlib).  Test infrastructure.
#include <stdio.h>

#include <memory>
#include <vector>

#include "deflate_dyn_driver.hpp"

static std::vector<uint8_t> content(int kind, size_t n) {
    std::vector<uint8_t> v(n);
    uint32_t x = 99u + (uint32_t)n * 7u + (uint32_t)kind;
    const char* text = "{\"version\":\"1.1\",\"host\":\"h0123.dc4.example.com\",\"short_message\":\"pod to the net\",\"_level\":6}\n";
    for (size_t i = 0; i < n; ++i) {
        x = x * 1664525u + 1013904223u;
        switch (kind) {
            case 0: v[i] = 'a'; break;
            case 1: v[i] = (uint8_t)(65 + i % 3); break;
            case 2: v[i] = (uint8_t)i; break;
            case 3: v[i] = (uint8_t)(x >> 24); break;
            case 4: v[i] = (uint8_t)text[(i + (x >> 30)) % 94]; break;
            default: v[i] = (uint8_t)(33 + 3 * ((x >> 20) % 28) * ((x >> 8) % 3 == 0)); break;  // a skewed alphabet
        }
    }
    return v;
}

int main() {
    fgd::lane_stack() = 32u << 10;
    const uint32_t B = fg::deflate::kBlock;
    const size_t lengths[] = {0, 1, 2, 3, 4, 5, 63, 64, 65, 257, 258, 259, 2047, 2048, 2049, B - 1, B, B + 1, 2 * B + 1};
    unsigned long long members = 0, bytes = 0;
    for (size_t n : lengths)
        for (int kind = 0; kind <= 5; ++kind) {
            std::vector<uint8_t> in = content(kind, n);
            in.push_back('x');
            in.push_back('y');
            const uint64_t cuts[4] = {0, 0, n, n + 2};
            uint64_t zoff[4], zoff2[4];
            const uint64_t total = fgd::deflate_mode(in.data(), in.size(), cuts, 3, 1, nullptr, 0, zoff, nullptr);
            if (total == fgd::kBadArgs || total > fg::deflate::bound(in.size(), 3)) {
                fprintf(stderr, "length %zu kind %d: total %llu\n", n, kind, (unsigned long long)total);
                return 1;
            }
            std::unique_ptr<uint8_t[]> z(new uint8_t[total]);
            std::vector<uint32_t> info(fg::deflate::blocks_of(n) + 1u);
            if (fgd::deflate_mode(in.data(), in.size(), cuts, 3, 1, z.get(), total, zoff2, info.data()) != total || zoff2[3] != zoff[3] || zoff2[1] != 0) {
                fprintf(stderr, "length %zu kind %d: the second pass disagrees\n", n, kind);
                return 1;
            }
            members += 3;
            bytes += total;
        }
    // the builder: every symbol used, Fibonacci counts beyond both limits, one and no symbol
    unsigned long long builds = 0;
    for (uint32_t n : {286u, 30u, 19u})
        for (int kind = 0; kind < 4; ++kind) {
            std::vector<uint32_t> f(n, 0u), lens(n);
            uint32_t a = 1, b = 1;
            for (uint32_t k = 0; k < n; ++k) {
                if (kind == 0) f[k] = 57u;
                if (kind == 1 && k < 24u) {
                    f[n - 1u - k] = a;
                    const uint32_t c = a + b;
                    a = b;
                    b = c;
                }
                if (kind == 2 && k + 1u == n) f[k] = 5u;
            }
            uint32_t limited = 0;
            fgd::build(f.data(), n, n == 19u ? 7u : 15u, lens.data(), &limited);
            for (uint32_t k = 0; k < n; ++k)
                if ((lens[k] == 0u) != (f[k] == 0u) || lens[k] > 15u) {
                    fprintf(stderr, "builder n %u kind %d symbol %u: length %u\n", n, kind, k, lens[k]);
                    return 1;
                }
            ++builds;
        }
    printf("ok %llu members %llu bytes %llu builds\n", members, bytes, builds);
    return 0;
}
