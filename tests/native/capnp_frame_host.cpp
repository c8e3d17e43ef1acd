// capnp_frame_host.cpp -- the Cap'n Proto stream framer's device logic (flowgger_amd/csrc/fg_capnp_frame.hpp) on the CPU: every tile of
// every stage runs as one emulated wave (fg_wave_emu.hpp), stage after stage as the kernels are launched (test infrastructure).
// With -DFGC_STANDALONE the file has a main of its own: a seeded fuzz against the sequential walk, for sanitizer builds.
#include <string>
#include <vector>

#include "fg_capnp_frame.hpp"

using namespace fg::capnpf;
static std::string g_err;
extern "C" const char* fgcf_last_error() { return g_err.c_str(); }
extern "C" uint32_t fgcf_tile_words() { return kTileWords; }
extern "C" uint32_t fgcf_node_cap(uint64_t nbytes) { return node_cap_of(nbytes); }

// the sequential walk of fg_capnp_next.hpp: offsets (cap + 1 entries) -> stop reason
extern "C" uint32_t fgcf_walk(const uint8_t* bytes, uint64_t nbytes, uint64_t* offsets, uint64_t cap, uint64_t* n, uint64_t* consumed) {
    uint64_t k = 0;
    const uint32_t st = host_walk(bytes, nbytes, consumed, [&](uint64_t p) {
        if (k < cap) offsets[k] = p;
        ++k;
    });
    if (k <= cap) offsets[k] = *consumed;
    *n = k;
    return st;
}

// bytes: readable up to nbytes rounded up to 16.  hdr: H_WORDS words out.  Returns 0, or -1 on a wave divergence.
extern "C" int fgcf_frame(const uint8_t* bytes, uint64_t nbytes, uint64_t* offsets, uint64_t cap, uint32_t* hdr) {
    try {
        std::vector<uint32_t> scratch(scratch_words(nbytes) + 64, 0xA5A5A5A5u);  // (only what the launcher clears is cleared)
        for (uint64_t k = 0; k < scratch_zero_words(nbytes); ++k) scratch[k] = 0;
        const Scratch sc = carve(scratch.data(), nbytes);
        sc.bitmap[0] = 1u;
        std::vector<uint32_t> lds(kLdsWords);
        for (uint32_t t = 0; t < sc.tiles; ++t) fg::emu::run_wave([&] { mark_tile(bytes, nbytes, t, sc, lds.data()); });
        for (uint32_t t = sc.tiles; t-- > 0;) fg::emu::run_wave([&] { nodes_tile(bytes, nbytes, t, sc, lds.data()); });  // (any order)
        for (uint32_t u = 0; u < sc.node_cap; ++u) link_node(u, sc);
        for (uint32_t r = 1; r <= sc.rounds; ++r)
            for (uint32_t u = sc.node_cap; u-- > 0;) jump_round(u, r, sc);  // (any order inside a round)
        for (uint32_t t = 0; t < sc.tiles; ++t) fg::emu::run_wave([&] { emit_tile(bytes, nbytes, t, sc, offsets, cap, lds.data()); });
        for (uint32_t k = 0; k < H_WORDS; ++k) hdr[k] = sc.hdr[k];
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}

#if defined(FGC_STANDALONE)
#include <stdio.h>
int main() {
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto rnd = [&] { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
    for (int it = 0; it < 200; ++it) {
        std::vector<uint8_t> buf;
        const int msgs = (int)(rnd() % 60);
        for (int k = 0; k < msgs; ++k) {
            const uint32_t segs = 1u + (uint32_t)(rnd() % 3), table = segs / 2u + 1u;
            std::vector<uint32_t> t(table * 2u, 0u);
            t[0] = segs - 1u;
            uint32_t words = 0;
            for (uint32_t s = 0; s < segs; ++s) { t[1 + s] = (uint32_t)(rnd() % ((rnd() & 7) ? 40 : 1500)); words += t[1 + s]; }
            const uint8_t* tb = reinterpret_cast<const uint8_t*>(t.data());
            buf.insert(buf.end(), tb, tb + table * 8u);
            for (uint32_t w = 0; w < words * 8u; ++w) buf.push_back((rnd() & 3) ? 0 : (uint8_t)(rnd() % 5));
        }
        uint64_t nbytes = buf.size() ? rnd() % (buf.size() + 1) : 0;
        if (it & 1) nbytes = buf.size();
        buf.resize((buf.size() + 15) / 16 * 16 + 16, 0);
        const uint64_t cap = nbytes / 8 + 1;
        std::vector<uint64_t> a(cap + 1, ~0ull), b(cap + 1, ~0ull);
        uint64_t n = 0, consumed = 0;
        uint32_t hdr[H_WORDS];
        const uint32_t st = fgcf_walk(buf.data(), nbytes, a.data(), cap, &n, &consumed);
        if (fgcf_frame(buf.data(), nbytes, b.data(), cap, hdr) != 0) { printf("divergence: %s\n", g_err.c_str()); return 1; }
        if (hdr[H_DECLINE]) continue;
        if (!hdr[H_DONE] || hdr[H_STOP] != st || hdr[H_NFRAMES] != n || hdr[H_CONSUMED] * 8ull != consumed) { printf("mismatch at %d\n", it); return 1; }
        for (uint64_t k = 0; k <= n; ++k)
            if (a[k] != b[k]) { printf("offset %llu differs at %d\n", (unsigned long long)k, it); return 1; }
    }
    printf("ok\n");
    return 0;
}
#endif
