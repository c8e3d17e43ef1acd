// tests/native/sparse_need_host.cpp -- fg_sparse_need.hpp against a byte-by-byte model (tests/test_sparse_need_cpu.py).
// A group = consecutive lines packed back to back from o[0] on, tile byte 0 at a0 = o[0] & ~15.  Model: byte b is wanted when
// o0 <= b < min(o0 + H, o1) or o1 - tail <= b < o1 (and b >= a0) for a line [o0, o1) of the group; a chunk is wanted when it holds a
// wanted byte.  The header marks chunks as the kernel does: need_head per line (first = the group's first line), need_tail for the
// last line.  Both directions are checked: every wanted chunk is marked, no other chunk is.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../flowgger_amd/csrc/fg_sparse_need.hpp"

static uint32_t rng_state = 2463534242u;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

static long check_group(uint64_t first, const std::vector<uint32_t>& lens, uint32_t H, uint32_t tail) {
    std::vector<uint64_t> o(lens.size() + 1);
    o[0] = first;
    for (size_t i = 0; i < lens.size(); ++i) o[i + 1] = o[i] + lens[i];
    const uint64_t a0 = o[0] & ~15ull;
    const size_t nchunk = (size_t)((o.back() - a0 + 15u) / 16u) + 1u;
    std::vector<char> model(nchunk, 0), marked(nchunk, 0);
    for (size_t i = 0; i < lens.size(); ++i) {
        const uint64_t o0 = o[i], o1 = o[i + 1];
        for (uint64_t b = a0; b < o1; ++b) {
            const bool head = b >= o0 && b < o0 + H;
            const bool end = b + tail >= o1;  // o1 - tail <= b, without the underflow
            if (head || end) model[(b - a0) / 16u] = 1;
        }
    }
    long errors = 0;
    auto mark = [&](fg::NeedRange r, size_t limit) {
        if (r.n > limit) ++errors;  // more consecutive chunks than the kernel's two words per lane hold
        for (uint32_t c = r.c0; c < r.c0 + r.n; ++c) {
            if (c >= nchunk) ++errors;
            else marked[c] = 1;
        }
    };
    const size_t limit = (H + tail + 14u) / 16u + 1u;
    for (size_t i = 0; i < lens.size(); ++i) mark(fg::need_head((uint32_t)(o[i] - a0), lens[i], H, tail, i == 0), limit);
    mark(fg::need_tail((uint32_t)(o.back() - a0), tail), 2);
    for (size_t c = 0; c < nchunk; ++c)
        if (model[c] != marked[c]) {
            if (errors < 5) fprintf(stderr, "H %u tail %u first %llu lines %zu: chunk %zu model %d marked %d\n", H, tail, (unsigned long long)first, lens.size(), c, model[c], marked[c]);
            ++errors;
        }
    return errors;
}

int main() {
    long errors = 0, groups = 0;
    const uint32_t heads[3] = {96, 112, 16};
    for (uint32_t H : heads)
        for (uint32_t tail = 1; tail <= 4; ++tail) {
            // edges: every alignment of the first line x every length of two lines around the head length
            for (uint64_t al = 0; al < 32; ++al)
                for (uint32_t l0 = 0; l0 <= H + 20; ++l0)
                    for (uint32_t l1 : {0u, 1u, 2u, 3u, 15u, 16u, 17u, H - 1u, H, H + 1u, H + 15u, H + 16u, H + 17u, 254u}) {
                        errors += check_group(4096u + al, {l0, l1}, H, tail), ++groups;
                        errors += check_group(al, {l1, l0, l1}, H, tail), ++groups;
                    }
            // runs of empty and one-byte lines: the last bytes of a line reach into the lines in front of it
            for (uint64_t al = 0; al < 16; ++al) {
                errors += check_group(al, {0, 0, 0, 0}, H, tail), ++groups;
                errors += check_group(64u + al, {300, 1, 1, 1, 0, 2, 0, 300}, H, tail), ++groups;
                errors += check_group(64u + al, {1}, H, tail), ++groups;
                errors += check_group(al, {0}, H, tail), ++groups;
            }
            // random groups of up to 64 lines: bench-shaped lengths, short ones, a mix
            for (int it = 0; it < 4000; ++it) {
                const uint32_t n = 1u + rnd() % 64u, kind = rnd() % 3u;
                std::vector<uint32_t> lens(n);
                for (auto& l : lens) l = kind == 0 ? 180u + rnd() % 150u : kind == 1 ? rnd() % 40u : (rnd() % 4u ? rnd() % 600u : rnd() % 4u);
                errors += check_group(((uint64_t)rnd() << 8) + rnd() % 4096u, lens, H, tail), ++groups;
            }
        }
    printf("%ld groups, %ld errors\n", groups, errors);
    return errors ? 1 : 0;
}
