// frame_multi_host.cpp -- flowgger_amd/csrc/fg_frame_multi.hpp (the boundary logic of the segmented framer) compiled for the CPU
// (test infrastructure).  The framing scan itself is restated position by position (D = delimiter, E = the UTF-8 rule over the byte
// and its three predecessors, E(nbytes) = cut off by the end); the patches, the clamp and the finishing pass are the header's, run
// the two ways the kernels run them:
//   block == 0   one "lane" per segment index over the whole buffer (the classic form; new delimiters are counted per 16 KiB block)
//   block  > 0   every block of `block` bytes walks the boundaries that touch it and applies the bits that lie in it (the one-pass form)
// `reverse` visits the lanes in the opposite order: every bit has one owner, so the order must not matter.
#include <stdint.h>

#include <vector>

#include "fg_frame_multi.hpp"

namespace {

using namespace fg::fmulti;

struct Arrays {
    std::vector<uint8_t>& D;
    std::vector<uint8_t>& E;
    uint64_t lo, hi;  // positions this sink owns: [lo, hi)
    uint64_t* new_delims;
    bool mine(uint64_t x) const { return x >= lo && x < hi; }
    void set_delim(uint64_t x) const {
        if (!mine(x)) return;
        if (!D[x]) ++*new_delims;
        D[x] = 1;
    }
    void put_err(uint64_t x, bool v) const {
        if (mine(x)) E[x] = v ? 1 : 0;
    }
    void or_err(uint64_t x) const {
        if (mine(x)) E[x] = 1;
    }
};

}  // namespace

extern "C" {

// -> the slot count, or -(need) when cap is too small (nothing written then); c_out: the clamped starts (n_segs + 1)
long fgm_frame(const uint8_t* bytes, uint64_t nbytes, uint32_t delim, const uint64_t* seg_starts, const uint8_t* seg_final, uint64_t n_segs,
               uint64_t block, int reverse, uint64_t* offsets, uint8_t* kind, uint64_t cap, uint64_t* seg_first, uint64_t* seg_consumed,
               uint64_t* c_out, uint64_t* new_delims_out) {
    std::vector<uint64_t> c(n_segs + 1);
    uint64_t run = 0;
    for (uint64_t k = 0; k <= n_segs; ++k) c[k] = run = clamp_start(seg_starts[k], run, nbytes, k, n_segs);
    for (uint64_t k = 0; k <= n_segs; ++k) c_out[k] = c[k];
    auto byte = [&](uint64_t x) -> uint32_t { return bytes[x]; };
    // the scan, unpatched
    std::vector<uint8_t> D(nbytes + 1, 0), E(nbytes + 1, 0);
    for (uint64_t x = 0; x <= nbytes; ++x) {
        if (x < nbytes) D[x] = bytes[x] == delim;
        E[x] = fg::utf8::err_at_pos(bytes, nbytes, x);
    }
    uint64_t new_delims = 0;
    if (nbytes && n_segs >= 2) {
        if (block == 0) {
            for (uint64_t i = 1; i < n_segs; ++i) {
                const uint64_t k = reverse ? n_segs - i : i;
                uint64_t prev = 0, next = 0;
                const uint64_t p = boundary_at(c.data(), n_segs, nbytes, k, &prev, &next);
                if (p != kNoBoundary) patch_boundary(p, prev, next, nbytes, byte, Arrays{D, E, 0, nbytes + 1, &new_delims});
            }
        } else {
            const uint64_t nblk = nbytes / block + 1;
            for (uint64_t bi = 0; bi < nblk; ++bi) {
                const uint64_t base = (reverse ? nblk - 1 - bi : bi) * block;
                for (uint64_t k = block_first_index(c.data(), n_segs, base); k < n_segs && block_touched_by(c[k], base, block); ++k) {
                    uint64_t prev = 0, next = 0;
                    const uint64_t p = boundary_at(c.data(), n_segs, nbytes, k, &prev, &next);
                    if (p != kNoBoundary) patch_boundary(p, prev, next, nbytes, byte, Arrays{D, E, base, base + block, &new_delims});
                }
            }
        }
    }
    *new_delims_out = new_delims;
    // rank + emit
    uint64_t total = 0;
    for (uint64_t x = 0; x < nbytes; ++x) total += D[x];
    const uint64_t n = nbytes ? total + (bytes[nbytes - 1] != delim ? 1u : 0u) : 0;
    if (n > cap) return -(long)n;
    for (uint64_t i = 0; i < n; ++i) kind[i] = kSlotFrame;
    offsets[0] = 0;
    uint64_t rank = 0;
    for (uint64_t x = 0; x <= nbytes; ++x) {
        if (E[x] && rank < n) kind[rank] = kSlotBadUtf8;
        if (x < nbytes && D[x]) offsets[++rank] = x + 1;
    }
    if (n > total) offsets[n] = nbytes;
    // finish
    for (uint64_t k = 0; k < n_segs; ++k) {
        const SegResult r = finish_segment(c.data(), k, seg_final, offsets, n, delim, byte);
        seg_first[k] = r.first;
        seg_consumed[k] = r.consumed;
        if (r.carry < n) kind[r.carry] = kSlotCarry;
    }
    seg_first[n_segs] = n;
    return (long)n;
}

}  // extern "C"
