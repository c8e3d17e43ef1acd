// syslen_host.cpp -- the octet-counted framer's device logic (flowgger_amd/csrc/fg_syslen.hpp) on the CPU: every tile of every stage
// runs as one emulated wave (fg_wave_emu.hpp), stage after stage as the kernels are launched (test infrastructure).
#include <string>
#include <vector>

#include "fg_syslen.hpp"

using namespace fg::syslen;
static std::string g_err;
extern "C" const char* fgs_last_error() { return g_err.c_str(); }
extern "C" uint32_t fgs_tile() { return kTile; }
extern "C" uint32_t fgs_max_prefix() { return kMaxPrefix; }

// out: status, prefix length, payload length
extern "C" void fgs_parse(const uint8_t* bytes, uint64_t nbytes, uint64_t p, uint64_t bound, uint64_t out[3]) {
    const Prefix pr = parse_prefix([&](uint64_t a) { return (uint32_t)bytes[a]; }, p, nbytes, bound);
    out[0] = pr.st; out[1] = pr.plen; out[2] = pr.len;
}
extern "C" int fgs_utf8_bad(const uint8_t* b, uint64_t n) { return fg::utf8::payload_bad(b, n) ? 1 : 0; }

// bytes: readable up to nbytes rounded up to 16.  hdr: H_WORDS words out.  Returns 0, or -1 on a wave divergence.
extern "C" int fgs_frame(const uint8_t* bytes, uint64_t nbytes, uint8_t* packed, uint64_t* offsets, uint64_t* starts, uint8_t* bad,
                         uint64_t cap, uint32_t* hdr) {
    try {
        std::vector<uint32_t> scratch(scratch_words(nbytes) + 64, 0xA5A5A5A5u);  // (only what the launcher clears is cleared)
        for (uint64_t k = 0; k < scratch_zero_words(nbytes); ++k) scratch[k] = 0;
        for (uint64_t k = 0; k < cap; ++k) bad[k] = 0;
        const Scratch sc = carve(scratch.data(), nbytes);
        std::vector<uint32_t> lds(kLdsWords + kEmitLdsWords);
        for (uint32_t t = 0; t < sc.tiles; ++t) fg::emu::run_wave([&] { resolve_route(bytes, nbytes, t, sc, lds.data()); });
        for (uint32_t t = 0; t < sc.tiles; ++t)
            for (uint32_t s = 0; s < kInbox; ++s) walk_node(bytes, nbytes, t, s, sc);
        for (uint32_t r = 1; r <= sc.rounds; ++r)
            for (uint32_t t = sc.tiles; t-- > 0;)  // (any order inside a round)
                for (uint32_t s = 0; s < kInbox; ++s) jump_round(t, s, r, sc);
        for (uint32_t t = 0; t < sc.tiles; ++t) fg::emu::run_wave([&] { emit_tile(bytes, nbytes, t, sc, packed, offsets, starts, bad, cap, lds.data()); });
        for (uint32_t k = 0; k < H_WORDS; ++k) hdr[k] = sc.hdr[k];
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}
