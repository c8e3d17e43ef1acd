// fg_frame_multi.hpp -- the boundary logic of the SEGMENTED framer (fg_frame_multi.hip): one buffer holds the chunks of K
// connections back to back, and every chunk is framed as a stream of its own.  HIP-free: the kernels instantiate it with sinks over
// their mask words, the CPU suite with a sink over plain arrays (tests/native/frame_multi_host.cpp).
//
// The framing scan (fg_frame.hip) computes, per byte position x of the buffer, a delimiter bit D(x) and a UTF-8 error bit E(x) --
// E from the byte and its three predecessors, E(nbytes) = "a sequence is cut off by the end".  A segment boundary at p (a segment
// starts at p, 0 < p < nbytes) changes three things:
//   (a) D(p - 1) is set: the tail of the segment before p ends there (nothing changes when that byte is a delimiter already);
//   (b) E(p), E(p + 1), E(p + 2) are recomputed with the bytes before p read as zero: a continuation byte that opens a segment is
//       stray, whatever the segment before ended with, and nothing is "missing" at p because somebody else's lead stands before it;
//   (c) E(p - 1) is set when the bytes before p end in an incomplete sequence (of THEIR segment): the verdict "cut off by the end"
//       lands in the tail's slot, because a position's slot is the number of delimiters strictly before it.
// Segments shorter than four bytes make these windows overlap.  Every error bit therefore has ONE owner, who computes its final value:
// position x belongs to the last boundary at or before it when x - boundary < 3, and then (c) of the NEXT boundary is folded into
// that value; otherwise nobody owns it and the next boundary may OR its (c) into the scan's own value.  Bits of one word are written by
// several owners, so a sink edits bits atomically.
#pragma once
#include <stdint.h>

#include "fg_utf8.hpp"

#if defined(__HIPCC__)
#define FG_FM_FN __host__ __device__ __forceinline__
#else
#define FG_FM_FN inline
#endif

namespace fg {
namespace fmulti {

constexpr uint8_t kSlotFrame = 0, kSlotBadUtf8 = 1, kSlotCarry = 2;  // FG_SLOT_* of include/fg_hip.h
constexpr uint64_t kNoBoundary = ~0ull;

// (fg_utf8.hpp's rule under the names it had while a copy lived here: test hosts written against them keep compiling)
FG_FM_FN bool utf8_err_at(uint32_t b, uint32_t p1, uint32_t p2, uint32_t p3) { return utf8::err_at(b, p1, p2, p3); }
FG_FM_FN bool utf8_cut_off(uint32_t p1, uint32_t p2, uint32_t p3) { return utf8::cut_off(p1, p2, p3); }

// seg_starts as the kernels use them: value k clamped into [value k - 1, nbytes], the first one 0 and the last one nbytes -- a list
// that does not tile the buffer frames SOMETHING, and nothing is read or written out of bounds for it.
FG_FM_FN uint64_t clamp_start(uint64_t raw, uint64_t running_max, uint64_t nbytes, uint64_t k, uint64_t n_segs) {
    if (k == 0) return 0;
    if (k >= n_segs) return nbytes;
    const uint64_t v = raw > running_max ? raw : running_max;
    return v < nbytes ? v : nbytes;
}

// first index in [lo, hi) with a[i] >= v (a non-decreasing)
FG_FM_FN uint64_t lower_bound_u64(const uint64_t* a, uint64_t lo, uint64_t hi, uint64_t v) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (a[mid] < v) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}
// first index in [lo, hi) with a[i] > v
FG_FM_FN uint64_t upper_bound_u64(const uint64_t* a, uint64_t lo, uint64_t hi, uint64_t v) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (a[mid] <= v) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// The clamped starts as the tile stages of the chained framers ask for them (fg_syslen_multi.hpp, fg_capnp_frame_multi.hpp: a stage
// works on tiles of kTileBytes and wants to know how far the frame that starts at a position may reach)
template <uint32_t kTileBytes>
struct Segs {
    static constexpr bool kSegmented = true;
    const uint64_t* c;  // n_segs + 1, non-decreasing, c[0] = 0, c[n_segs] = nbytes
    uint64_t n_segs;
    // the first index j with c[j] > p, n_segs when there is none: p < nbytes lies in segment j - 1, which ends at c[j]
    FG_FM_FN uint64_t behind(uint64_t p) const { return upper_bound_u64(c, 0, n_segs, p); }
    FG_FM_FN uint64_t limit(uint64_t p) const { return c[behind(p)]; }
    // ... for the positions of one tile: the boundaries inside it are c[j0 .. j1)
    struct Tile {
        const uint64_t* c;
        uint64_t j0, j1;
        FG_FM_FN uint64_t limit(uint64_t p) const { return c[j0 == j1 ? j0 : upper_bound_u64(c, j0, j1, p)]; }
    };
    FG_FM_FN Tile tile(uint64_t base) const {
        const uint64_t j0 = behind(base);
        return Tile{c, j0, upper_bound_u64(c, j0, n_segs, base + kTileBytes - 1u)};
    }
};

// The patches of the boundary at p (0 < p < nbytes).  prev: the nearest boundary before p (0 = none: the buffer's start); next: the
// nearest boundary behind p (kNoBoundary = none; the buffer's end is no boundary).  byte(x): the buffer's byte, asked for x < nbytes
// only.  sink: set_delim(x), put_err(x, v) (the bit's final value), or_err(x) -- x <= nbytes; a sink may ignore positions that are
// not its own (a block of the one-pass scan applies the bits that lie in it and leaves the rest to its neighbours).
template <class Byte, class Sink>
FG_FM_FN void patch_boundary(uint64_t p, uint64_t prev, uint64_t next, uint64_t nbytes, Byte&& byte, Sink&& sink) {
    sink.set_delim(p - 1u);                                                                   // (a)
    for (uint32_t d = 0; d < 3u; ++d) {                                                       // (b), with the next boundary's (c) folded in
        const uint64_t x = p + d;
        if (x > nbytes || x >= next) break;
        const uint32_t b = x < nbytes ? byte(x) : 0u;
        const uint32_t p1 = d >= 1u ? byte(x - 1u) : 0u, p2 = d >= 2u ? byte(x - 2u) : 0u;
        bool e = utf8::err_at(b, p1, p2, 0u);
        if (x + 1u == next) e |= utf8::cut_off(b, p1, p2);
        sink.put_err(x, e);
    }
    if (prev == 0 || p - prev >= 4u) {                                                        // (c), where p - 1 has no owner
        const uint32_t q1 = byte(p - 1u);
        const uint32_t q2 = p >= 2u && p - 2u >= prev ? byte(p - 2u) : 0u;
        const uint32_t q3 = p >= 3u && p - 3u >= prev ? byte(p - 3u) : 0u;
        if (utf8::cut_off(q1, q2, q3)) sink.or_err(p - 1u);
    }
}

// The boundary that the clamped seg_starts c[0 .. n_segs] put at index k (1 <= k < n_segs): c[k] when it lies inside the buffer and k
// is the first index with that value (empty segments repeat it), else kNoBoundary; *prev / *next as patch_boundary wants them.
FG_FM_FN uint64_t boundary_at(const uint64_t* c, uint64_t n_segs, uint64_t nbytes, uint64_t k, uint64_t* prev, uint64_t* next) {
    const uint64_t p = c[k];
    if (p == 0 || p >= nbytes || c[k - 1u] == p) return kNoBoundary;
    *prev = c[k - 1u];
    const uint64_t j = upper_bound_u64(c, k + 1u, n_segs + 1u, p);
    *next = j <= n_segs && c[j] < nbytes ? c[j] : kNoBoundary;
    return p;
}

// A block [base, base + block) of the one-pass scan applies the bits of the boundaries that TOUCH it -- one of p - 1 .. p + 2 lies in
// it: p in [base - 2, base + block] -- : the first index of c that can hold one, and whether the boundary value p still does (c is
// sorted, so the first one that does not ends the block's walk).
FG_FM_FN uint64_t block_first_index(const uint64_t* c, uint64_t n_segs, uint64_t base) {
    return lower_bound_u64(c, 1u, n_segs, base > 3u ? base - 2u : 1u);
}
FG_FM_FN bool block_touched_by(uint64_t p, uint64_t base, uint64_t block) { return p <= base + block; }

// What the finishing pass derives for segment k from the slot offsets[0 .. n_slots]: its first slot, whether its last slot is a CARRY
// (the unterminated tail of a segment that is not its connection's last), and the bytes its frames cover.
struct SegResult {
    uint64_t first;     // seg_first[k]
    uint64_t carry;     // the slot to mark FG_SLOT_CARRY, kNoBoundary = none
    uint64_t consumed;  // seg_consumed[k]
};
template <class Byte>
FG_FM_FN SegResult finish_segment(const uint64_t* c, uint64_t k, const uint8_t* seg_final, const uint64_t* offsets, uint64_t n_slots,
                                  uint32_t delim, Byte&& byte) {
    SegResult r;
    const uint64_t s = c[k], e = c[k + 1u];
    r.first = lower_bound_u64(offsets, 0, n_slots + 1u, s);  // (every segment start is a slot offset)
    r.carry = kNoBoundary;
    r.consumed = e - s;
    if (e > s && !(seg_final && seg_final[k]) && byte(e - 1u) != delim) {
        const uint64_t last = lower_bound_u64(offsets, r.first, n_slots + 1u, e) - 1u;  // the slot that ends at e
        if (last < n_slots) {  // (always, for offsets that belong to c; never read behind them for others)
            r.carry = last;
            r.consumed = offsets[last] - s;
        }
    }
    return r;
}

}  // namespace fmulti
}  // namespace fg
