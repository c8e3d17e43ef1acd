// capnp_frame_multi_host.cpp -- the segmented Cap'n Proto framer's device logic (flowgger_amd/csrc/fg_capnp_frame_multi.hpp over
// fg_capnp_frame.hpp) on the CPU: every tile of every stage runs as one emulated wave (fg_wave_emu.hpp), stage after stage as the kernels
// are launched (test infrastructure).  With -DFGCM_STANDALONE the file has a main of its own: a boundary at every word of a three-tile
// stream against the sequential walk per segment, for sanitizer builds.
#include <string>
#include <vector>

#include "fg_capnp_frame_multi.hpp"

using namespace fg::capnpf;
static std::string g_err;
extern "C" const char* fgcm_last_error() { return g_err.c_str(); }
extern "C" uint32_t fgcm_tile_words() { return kTileWords; }
extern "C" uint32_t fgcm_node_cap(uint64_t nbytes, uint64_t n_segs) { return m_node_cap(nbytes, n_segs); }

// bytes: readable up to nbytes rounded up to 16.  raw_starts: n_segs + 1, clamped here as k_seg_clamp does.  hdr: H_WORDS words out.
// Returns 0, or -1 on a wave divergence.
extern "C" int fgcm_frame(const uint8_t* bytes, uint64_t nbytes, const uint64_t* raw_starts, uint64_t n_segs, uint64_t* offsets, uint8_t* kind,
                          uint64_t cap, uint64_t* seg_first, uint64_t* seg_consumed, uint8_t* seg_stop, uint32_t* hdr) {
    try {
        std::vector<uint32_t> scratch(m_scratch_words(nbytes, n_segs) + 64, 0xA5A5A5A5u);  // (only what the launcher clears is cleared)
        for (uint64_t k = 0; k < m_zero_words(nbytes, n_segs); ++k) scratch[k] = 0;
        const MScratch sc = m_carve(scratch.data(), nbytes, n_segs);
        for (uint64_t k = 0; k < n_segs; ++k) sc.sg_stop[k] = kNil;
        uint64_t run = 0;
        for (uint64_t k = 0; k <= n_segs; ++k) sc.raw[k] = run = fg::fmulti::clamp_start(raw_starts[k], run, nbytes, k, n_segs);
        const Segs sg = sc.segs();
        std::vector<uint32_t> lds(kLdsWords);
        for (uint64_t k = n_segs + 1; k-- > 0;) seg_root(k, sc);  // (any order inside a stage)
        for (uint32_t t = 0; t < sc.tiles; ++t) fg::emu::run_wave([&] { mark_tile(bytes, nbytes, t, sc, lds.data(), sg); });
        for (uint32_t t = sc.tiles; t-- > 0;) fg::emu::run_wave([&] { nodes_tile(bytes, nbytes, t, sc, lds.data(), sg); });
        for (uint32_t u = sc.node_cap; u-- > 0;) link_node(u, sc, sg);
        for (uint32_t r = 1; r <= sc.rounds; ++r)
            for (uint32_t u = sc.node_cap; u-- > 0;) jump_round(u, r, sc);
        for (uint32_t u = sc.node_cap; u-- > 0;) m_collect(u, sc);
        fg::emu::run_wave([&] { m_scan(sc, cap, offsets, kind, seg_first, seg_consumed, seg_stop); });
        for (uint32_t t = sc.tiles; t-- > 0;) fg::emu::run_wave([&] { m_emit_tile(bytes, nbytes, t, sc, offsets, kind, cap, lds.data()); });
        for (uint32_t k = 0; k < H_WORDS; ++k) hdr[k] = sc.hdr[k];
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}

#if defined(FGCM_STANDALONE)
#include <stdio.h>
static void put_msg(std::vector<uint8_t>& buf, uint32_t words, uint8_t fill) {
    const uint32_t t[2] = {0u, words};
    const uint8_t* tb = reinterpret_cast<const uint8_t*>(t);
    buf.insert(buf.end(), tb, tb + 8);
    buf.insert(buf.end(), (size_t)words * 8u, fill);
}
// one framer call against the sequential walk of every segment; 0 = equal
static int check(const std::vector<uint8_t>& padded, uint64_t nbytes, const std::vector<uint64_t>& starts) {
    const uint64_t n_segs = starts.size() - 1, cap = nbytes / 8 + n_segs;
    std::vector<uint64_t> off(cap + 2, ~0ull), first(n_segs + 2, ~0ull), cons(n_segs + 1, ~0ull), want_off;
    std::vector<uint8_t> kind(cap + 1, 0xEE), stop(n_segs + 1, 0xEE), want_kind;
    uint32_t hdr[H_WORDS];
    if (fgcm_frame(padded.data(), nbytes, starts.data(), n_segs, off.data(), kind.data(), cap, first.data(), cons.data(), stop.data(), hdr) != 0) {
        printf("divergence: %s\n", g_err.c_str());
        return 1;
    }
    if (hdr[H_DECLINE] || !hdr[H_DONE]) { printf("declined\n"); return 1; }
    std::vector<uint64_t> c(n_segs + 1);
    uint64_t run = 0;
    for (uint64_t k = 0; k <= n_segs; ++k) {
        run = fg::fmulti::clamp_start(starts[k], run, nbytes, k, n_segs);
        c[k] = k < n_segs ? run & ~7ull : run;
    }
    for (uint64_t k = 0; k < n_segs; ++k) {
        const uint64_t s = c[k], e = c[k + 1];
        if (first[k] != want_off.size()) { printf("seg_first[%llu]\n", (unsigned long long)k); return 1; }
        uint64_t consumed = 0;
        const uint32_t st = host_walk(padded.data() + s, e - s, &consumed, [&](uint64_t p) { want_off.push_back(s + p); want_kind.push_back(0); });
        if (consumed < e - s) { want_off.push_back(s + consumed); want_kind.push_back(2); }
        if (cons[k] != consumed || stop[k] != st) { printf("segment %llu: consumed / stop\n", (unsigned long long)k); return 1; }
    }
    want_off.push_back(nbytes);
    if (hdr[H_NFRAMES] != want_kind.size() || first[n_segs] != want_kind.size()) { printf("slot count\n"); return 1; }
    for (size_t i = 0; i < want_off.size(); ++i)
        if (off[i] != want_off[i] || (i < want_kind.size() && kind[i] != want_kind[i])) { printf("slot %zu\n", i); return 1; }
    if (off[want_off.size()] != ~0ull || kind[want_kind.size()] != 0xEE) { printf("a guard entry was written\n"); return 1; }
    return 0;
}
int main() {
    uint64_t seed = 0x9E3779B97F4A7C15ull;
    auto rnd = [&] { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return seed; };
    std::vector<uint8_t> buf;
    while (buf.size() < 3u * kTileBytes) put_msg(buf, (rnd() & 3) ? 0u : (uint32_t)(rnd() % 90), (rnd() & 1) ? 0 : (uint8_t)(rnd() % 3));
    buf.resize(3u * kTileBytes + 24);  // (the last message is cut: a TAIL; the chunk ends off a tile)
    const uint64_t nbytes = buf.size() - 3;  // ... and off a word
    buf.resize((buf.size() + 15) / 16 * 16 + 16, 0);
    for (uint64_t w = 1; w * 8 < nbytes; ++w) {
        if (check(buf, nbytes, {0, w * 8, nbytes})) { printf("boundary at word %llu\n", (unsigned long long)w); return 1; }
        if (check(buf, nbytes, {0, w * 8, w * 8, (w + 1) * 8 < nbytes ? (w + 1) * 8 : nbytes, nbytes})) {
            printf("boundaries at words %llu, %llu\n", (unsigned long long)w, (unsigned long long)w + 1);
            return 1;
        }
    }
    std::vector<uint64_t> every;  // a segment per word
    for (uint64_t w = 0; w * 8 < nbytes; ++w) every.push_back(w * 8);
    every.push_back(nbytes);
    if (check(buf, nbytes, every)) { printf("a segment per word\n"); return 1; }
    if (check(buf, nbytes, {0, 13, 5, 3, ~0ull, nbytes})) { printf("a list that needs clamping\n"); return 1; }
    printf("ok\n");
    return 0;
}
#endif
