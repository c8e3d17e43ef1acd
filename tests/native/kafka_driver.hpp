// kafka_driver.hpp -- the passes of fg_kafka.hip as host loops over fg_kafka.hpp on the wave emulation: what a kernel does per wave or per
// lane, a loop does per iteration, with the kernels' arguments (test infrastructure, host only).
#pragma once
#include <functional>
#include <vector>

#include "fg_kafka.hpp"

namespace fgk {
namespace kf = fg::kafka;

constexpr uint64_t kBadArgs = ~0ull;

// bytes of stack per emulated lane (0 = the emulation's default), as deflate_driver.hpp's: a sanitized stand-alone program asks for
// small ones, AddressSanitizer's cost of a lane switch grows with them
inline size_t& lane_stack() {
    static size_t v = 0;
    return v;
}
inline void run_wave(const std::function<void()>& body) {
    if (lane_stack()) fg::emu::run_wave(body, lane_stack());
    else fg::emu::run_wave(body);
}

// k_kf_sizes and its scan: set_off[n + 1]; false for offsets the set refuses
inline bool sizes(const uint64_t* off, const uint8_t* skip, uint64_t n, uint64_t nbytes, uint64_t* set_off) {
    uint64_t o = 0;
    bool ok = true;
    for (uint64_t i = 0; i < n; ++i) {
        set_off[i] = o;
        if (kf::value_ok(off[i], off[i + 1], nbytes)) o += kf::wire_size(off[i + 1] - off[i], skip && skip[i]);
        else ok = false;
    }
    set_off[n] = o;
    return ok;
}
// k_kf_write: `waves` waves take the steps in turn (the bytes do not depend on it)
inline void write(const uint8_t* bytes, const uint64_t* off, const uint8_t* skip, uint64_t n, const uint64_t* set_off, uint8_t* set, uint64_t set_cap,
                  uint64_t waves = 3) {
    const uint64_t steps = kf::write_steps(n);
    for (uint64_t w = 0; w < waves && w < steps; ++w) {
        std::vector<uint32_t> lds(kf::kLdsWords);
        run_wave([&] {
            kf::build_tables(lds.data());
            const kf::Lds s = kf::lds_of(lds.data());
            for (uint64_t k = w; k < steps; k += waves) kf::write_step(bytes, off, skip, n, k * kf::kRowsPerWave, set_off, set, set_cap, s);
        });
    }
}
// k_kf_cuts
inline void cuts(const uint64_t* set_off, const uint64_t* member_first, uint64_t n, uint64_t n_members, uint64_t* set_cuts) {
    for (uint64_t k = 0; k <= n_members; ++k) set_cuts[k] = set_off[member_first[k] < n ? member_first[k] : n];
}
// k_kf_wrap_sizes and its scans
inline bool wrap_sizes(const uint64_t* z_off, uint64_t n_members, uint64_t* w_off, uint64_t* piece_first) {
    uint64_t o = 0, p = 0;
    bool ok = true;
    for (uint64_t m = 0; m < n_members; ++m) {
        w_off[m] = o;
        piece_first[m] = p;
        const uint64_t a = z_off[m], b = z_off[m + 1];
        if (b < a || b - a > kf::kMaxValue) ok = false;
        else if (b > a) {
            o += kf::wire_size(b - a, false);
            p += kf::pieces_of(b - a);
        }
    }
    w_off[n_members] = o;
    piece_first[n_members] = p;
    return ok;
}
// k_kf_wrap and k_kf_wrap_finish
inline void wrap(const uint8_t* z, const uint64_t* z_off, const uint64_t* piece_first, uint64_t n_members, const uint64_t* w_off, uint8_t* w, uint64_t w_cap,
                 uint32_t* piece_crc) {
    const uint64_t np = piece_first[n_members];
    std::vector<uint32_t> lds(kf::kLdsWords);
    if (np)
        run_wave([&] {
            kf::build_tables(lds.data());
            const kf::Lds s = kf::lds_of(lds.data());
            for (uint64_t g = 0; g < np; ++g) kf::wrap_piece(z, z_off, piece_first, n_members, g, w_off, w, w_cap, piece_crc, s);
        });
    for (uint64_t m = 0; m < n_members; ++m) kf::wrap_finish(z_off, piece_first, m, piece_crc, w_off, w, w_cap);
}

// fg_kafka_messageset_device: returns the total, or kBadArgs
inline uint64_t messageset(const uint8_t* bytes, uint64_t nbytes, const uint64_t* off, const uint8_t* skip, uint64_t n, uint8_t* set, uint64_t set_cap,
                           uint64_t* set_off) {
    if (!sizes(off, skip, n, nbytes, set_off)) return kBadArgs;
    if (set && set_off[n] <= set_cap && n) write(bytes, off, skip, n, set_off, set, set_cap);
    return set_off[n];
}
// fg_kafka_wrap_device
inline uint64_t wrap_members(const uint8_t* z, const uint64_t* z_off, uint64_t n_members, uint8_t* w, uint64_t w_cap, uint64_t* w_off) {
    std::vector<uint64_t> piece_first(n_members + 1u);
    if (!wrap_sizes(z_off, n_members, w_off, piece_first.data())) return kBadArgs;
    std::vector<uint32_t> piece_crc(piece_first[n_members] + 1u);
    if (w && w_off[n_members] <= w_cap) wrap(z, z_off, piece_first.data(), n_members, w_off, w, w_cap, piece_crc.data());
    return w_off[n_members];
}

}  // namespace fgk
