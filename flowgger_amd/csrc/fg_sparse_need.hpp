// fg_sparse_need.hpp -- which 16-byte chunks of a group's window the SPARSE register window fetches (fg_pipeline.hpp,
// persistent_loop<..., SPARSE>; the RFC5424 kernel for short lines without structured data, fg_rfc5424.hip).
//
// The decoder of such a line looks at its header and at its last byte, never into the message.  The window keeps its shape -- NB
// coalesced buffer loads of 1 KiB, lines at their natural tile offsets -- and a lane whose chunk lies wholly inside a message is
// given an offset beyond the buffer descriptor's range (bit 31): it fetches nothing and gets zeros.  A chunk is NEEDED when it overlaps
//     [o0, min(o0 + H, o1))   the head of a line [o0, o1) of the group, or
//     [o1 - tail, o1)         the last bytes of one (the trims; tail = 4 under a framing that strips up to two terminator bytes).
// Lines are packed back to back, so the last bytes of line i lie in front of the head of line i + 1: lane i marks ONE run of chunks
// for both (need_head), and the lane of the group's last line a second one for its own end (need_tail).
// Pure arithmetic, no HIP dependency: tests/native/sparse_need_host.cpp checks it against a byte-by-byte model on the CPU.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define FG_NEED_HD __host__ __device__
#else
#define FG_NEED_HD
#endif

namespace fg {

// Head bytes of the sparse window.  HBM is fetched in 128-byte pieces whatever part of one is asked for (tools/probe/sparse_read.cpp,
// DESIGN.md 3.0), so of a 254-byte line H = 96 leaves 222 B to fetch, 112 leaves 238 and 128 nothing to skip; the bench corpus'
// header and the three bytes behind it that the cheap trim test reads end at byte 94 at the latest.
constexpr uint32_t kSparseHead = 96;
constexpr uint32_t kSparseTailPlain = 2, kSparseTailFramed = 4;
// below this average length a line's needed bytes touch every 128-byte piece the line does: nothing to skip
constexpr uint64_t kSparseFromLen = kSparseHead + kSparseTailPlain + 127u;

struct NeedRange {
    uint32_t c0, n;  // chunks [c0, c0 + n) of the tile; n == 0: none
};
// Everything below is in TILE bytes: tile byte 0 is the packed buffer's byte a0 (16-byte aligned, at or in front of the group's first
// line), a line [o0, o1) of the group is t0 = o0 - a0, len = o1 - o0.  Bytes in front of the tile do not count.
// the chunks that overlap tile bytes [b0, b1)
FG_NEED_HD inline NeedRange need_chunks(uint32_t b0, uint32_t b1) {
    if (b1 <= b0) return NeedRange{0u, 0u};
    const uint32_t c0 = b0 >> 4, c1 = (b1 - 1u) >> 4;
    return NeedRange{c0, c1 - c0 + 1u};
}
// a line of the group: its head and, unless it is the group's first line, the last bytes of the line in front of it -- at most
// (H + tail + 14) / 16 + 1 consecutive chunks
FG_NEED_HD inline NeedRange need_head(uint32_t t0, uint32_t len, uint32_t H, uint32_t tail, bool first) {
    const uint32_t b0 = first ? t0 : (t0 >= tail ? t0 - tail : 0u);
    return need_chunks(b0, t0 + (len > H ? H : len));
}
// the last bytes of the group's last line, which ends at tile byte t1
FG_NEED_HD inline NeedRange need_tail(uint32_t t1, uint32_t tail) { return need_chunks(t1 >= tail ? t1 - tail : 0u, t1); }

}  // namespace fg
