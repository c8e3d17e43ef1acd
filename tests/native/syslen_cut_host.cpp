// syslen_cut_host.cpp -- the per-segment cut's device logic (flowgger_amd/csrc/fg_syslen_multi.hpp: cut_find, cut_mark) on the CPU: every
// workgroup of either pass runs as one emulated wave (fg_wave_emu.hpp), pass after pass as the kernels are launched, the workgroups of a
// pass in the order the caller asks for (test infrastructure).
#include <string>
#include <vector>

#include "fg_syslen_multi.hpp"

using namespace fg::syslen;
static std::string g_err;
extern "C" const char* fgsc_last_error() { return g_err.c_str(); }
extern "C" uint32_t fgsc_mark() { return kCutMark; }

// bad: n bytes, 0 / 1 going in; seg_first: n_segs + 1.  cut: cut_words(n_segs) + 2 words, the last two guards the caller checks.
// reverse: the workgroups of each pass run last to first.  Returns 0, or -1 on a wave divergence.
extern "C" int fgsc_cut(uint8_t* bad, uint64_t n, const uint64_t* seg_first, uint64_t n_segs, uint32_t* cut, int reverse) {
    try {
        if (n == 0 || n_segs == 0) return 0;  // (as the launcher)
        for (uint64_t k = 0; k < cut_words(n_segs); ++k) cut[k] = kCutNone;
        const uint64_t groups = (n + 63u) / 64u;
        for (int pass = 0; pass < 2; ++pass)
            for (uint64_t j = 0; j < groups; ++j) {
                const uint64_t g = reverse ? groups - 1u - j : j;
                fg::emu::run_wave([&] {
                    const uint64_t i = g * 64u + fg::emu::lane();
                    if (i >= n) return;
                    if (pass == 0) cut_find(bad, i, seg_first, n_segs, cut);
                    else cut_mark(bad, i, seg_first, n_segs, cut);
                });
            }
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return -1;
    }
}
