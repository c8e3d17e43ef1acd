// fg_utf8.hpp -- the framers' UTF-8 rule in its SCALAR form: well-formedness (Unicode 15 Table 3-7) judged AT one byte position
// from the byte and its three predecessors, so that no state is carried from position to position.  The dword-parallel form of the
// same rule is fuse::utf8_err_flags (fg_fuse.hpp); tests/test_utf8_rule_cpu.py ties the two together, bit for bit, and this one to
// Python's decoder.  What uses it: the octet-counted framers (fg_syslen.hpp, fg_syslen_multi.hpp), the UDP unpacker (fg_udp.hip), the
// boundary patches of the segmented framer (fg_frame_multi.hpp), the host hops of fg_host_pipeline.cpp and the CPU suite.
// No HIP, no wave primitives.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FG_U8H __host__ __device__ inline
#else
#define FG_U8H inline
#endif

namespace fg {
namespace utf8 {

// byte b, its predecessors p1 (nearest), p2, p3 (0 before the start of a payload): are the rules violated AT b?
FG_U8H bool err_at(uint32_t b, uint32_t p1, uint32_t p2, uint32_t p3) {
    const bool c1 = (p1 & 0xC0u) == 0x80u, c2 = (p2 & 0xC0u) == 0x80u;
    // a continuation byte is due here: after a lead, or as the 3rd / 4th byte of a sequence whose earlier bytes WERE continuations (a
    // sequence broken earlier was flagged there and expects nothing more -- so no expectation ever crosses an ASCII byte)
    const bool must = p1 >= 0xC0u || (p2 >= 0xE0u && c1) || (p3 >= 0xF0u && c2 && c1);
    bool err = ((b & 0xC0u) == 0x80u) != must;       // missing or stray continuation
    err |= b == 0xC0u || b == 0xC1u || b >= 0xF5u;   // bytes that never appear
    err |= p1 == 0xE0u && !(b & 0x20u);              // second-byte ranges: E0 A0..BF | ED 80..9F | F0 90..BF | F4 80..8F
    err |= p1 == 0xEDu && (b & 0x20u);
    err |= p1 == 0xF0u && !(b & 0x30u);
    err |= p1 == 0xF4u && (b & 0x30u);
    return err;
}
// ... for the position one past the end of a payload whose last bytes are p1, p2, p3: is a continuation still due?  (A sequence cut
// off by the end shows THERE, as the rule with b = 0.)
FG_U8H bool cut_off(uint32_t p1, uint32_t p2, uint32_t p3) { return err_at(0u, p1, p2, p3); }
// the rule at position i of the payload b[0 .. n), 0 <= i <= n: the bytes before the payload and the one behind it read as 0
FG_U8H bool err_at_pos(const uint8_t* b, uint64_t n, uint64_t i) {
    return err_at(i < n ? b[i] : 0u, i >= 1u ? b[i - 1u] : 0u, i >= 2u ? b[i - 2u] : 0u, i >= 3u ? b[i - 3u] : 0u);
}
// is the payload b[0 .. n) not valid UTF-8?  Positions 0 .. n INCLUSIVE: the last one holds "cut off by the end".
FG_U8H bool payload_bad(const uint8_t* b, uint64_t n) {
    for (uint64_t i = 0; i <= n; ++i)
        if (err_at_pos(b, n, i)) return true;
    return false;
}

}  // namespace utf8
}  // namespace fg
