// syslen_multi_host.cpp -- the segmented octet-counted framer's device logic (flowgger_amd/csrc/fg_syslen_multi.hpp over fg_syslen.hpp) on
// the CPU: every tile of every stage runs as one emulated wave (fg_wave_emu.hpp), stage after stage as the kernels are launched (test
// infrastructure).
#include <string>
#include <vector>

#include "fg_syslen_multi.hpp"

using namespace fg::syslen;
static std::string g_err;
extern "C" const char* fgsm_last_error() { return g_err.c_str(); }
extern "C" uint32_t fgsm_tile() { return kTile; }
extern "C" uint32_t fgsm_max_prefix() { return kMaxPrefix; }
extern "C" uint32_t fgsm_inbox() { return kInbox; }

// bytes: readable up to nbytes rounded up to 16.  raw_starts: n_segs + 1, clamped here as k_seg_clamp does.  hdr: H_WORDS words out.
// Returns 0, or -1 on a wave divergence.
extern "C" int fgsm_frame(const uint8_t* bytes, uint64_t nbytes, const uint64_t* raw_starts, uint64_t n_segs, uint8_t* packed, uint64_t* offsets,
                          uint64_t* starts, uint8_t* bad, uint64_t cap, uint64_t* seg_first, uint64_t* seg_consumed, uint8_t* seg_stop,
                          uint32_t* hdr) {
    try {
        std::vector<uint32_t> scratch(m_scratch_words(nbytes, n_segs) + 64, 0xA5A5A5A5u);  // (only what the launcher clears is cleared)
        for (uint64_t k = 0; k < m_zero_words(nbytes, n_segs); ++k) scratch[k] = 0;
        for (uint64_t k = 0; k < cap; ++k) bad[k] = 0;
        const MScratch sc = m_carve(scratch.data(), nbytes, n_segs);
        for (uint64_t k = 0; k < n_segs; ++k) sc.sg_stop[k] = kNil;
        uint64_t run = 0;
        for (uint64_t k = 0; k <= n_segs; ++k) sc.c[k] = run = fg::fmulti::clamp_start(raw_starts[k], run, nbytes, k, n_segs);
        std::vector<uint32_t> lds(kLdsWords + kEmitLdsWords);
        for (uint32_t t = 0; t < sc.tiles; ++t) fg::emu::run_wave([&] { resolve_route(bytes, nbytes, t, sc, lds.data(), sc.segs()); });
        for (uint32_t u = sc.nodes; u-- > 0;) m_walk(bytes, u, sc);  // (any order inside a stage)
        for (uint32_t r = 1; r <= sc.rounds; ++r)
            for (uint32_t u = sc.nodes; u-- > 0;) m_jump(u, r, sc);
        for (uint32_t u = 0; u < sc.nodes; ++u) m_collect(u, sc);
        fg::emu::run_wave([&] { m_scan(sc, cap, offsets, seg_first, seg_consumed, seg_stop); });
        for (uint32_t t = sc.tiles; t-- > 0;) fg::emu::run_wave([&] { m_emit(bytes, t, sc, packed, offsets, starts, bad, cap, lds.data()); });
        for (uint32_t k = 0; k < H_WORDS; ++k) hdr[k] = sc.hdr[k];
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}
