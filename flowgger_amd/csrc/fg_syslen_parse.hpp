// fg_syslen_parse.hpp -- the length prefix of an octet-counted frame (read_msglen, src/flowgger/splitter/syslen_splitter.rs:17-25)
// and the sequential walk over a chunk: what the device framer (fg_syslen.hpp), the host hop of the host-buffer entry points
// (fg_host_pipeline.cpp) and the CPU suite share.  The position-based UTF-8 rule they judge payloads by is fg_utf8.hpp's: a sequence
// cut off by the end of a payload shows at the position behind it -- under this framing the next prefix's byte or the chunk's end --,
// so the callers ask for position `len` itself and flag the frame that ends there.  No HIP, no wave primitives.
#pragma once
#include <stdint.h>

#include "fg_utf8.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FG_SLH __host__ __device__ inline
#else
#define FG_SLH inline
#endif


namespace fg {
namespace syslen {

constexpr uint32_t kMaxPrefix = 24;  // FG_SYSLEN_MAX_PREFIX: bytes of "<len> " the device parser reads, the ' ' included
// fg_syslen_stop + "a well-formed prefix whose payload fits"
enum { ST_CLEAN = 0, ST_TAIL = 1, ST_BAD_LEN = 2, ST_LONG_PREFIX = 3, ST_VALID = 4 };
// the result words of a launch of the device framer (fg_syslen.hpp, fg_syslen_multi.hpp), as the host reads them back (fg_capi.cpp)
enum { H_DECLINE = 0, H_STOP = 1, H_NFRAMES = 2, H_CONSUMED = 3, H_TOTAL = 4, H_DONE = 5, H_WORDS = 16 };

struct Prefix {
    uint32_t st, plen;
    uint64_t len;
};
// read_msglen at position p of a chunk of nbytes: the bytes up to and including the first ' ', the text before it as
// usize::from_str (an optional '+', at least one digit, leading zeros, nothing else, the value fits 64 bits).  bound = the bytes
// looked at (kMaxPrefix on the device; the host hop passes ~0).
template <class Get>
FG_SLH Prefix parse_prefix(Get get, uint64_t p, uint64_t nbytes, uint64_t bound = kMaxPrefix) {
    Prefix r{ST_CLEAN, 0u, 0ull};
    if (p >= nbytes) return r;
    uint64_t v = 0;
    bool digits = false, ovf = false;
    for (uint64_t k = 0; k < bound; ++k) {
        if (p + k >= nbytes) { r.st = ST_TAIL; return r; }
        const uint32_t c = get(p + k);
        if (c == ' ') {
            r.plen = (uint32_t)k + 1u;
            r.len = v;
            if (!digits || ovf) r.st = ST_BAD_LEN;
            else r.st = v > nbytes - (p + k + 1u) ? ST_TAIL : ST_VALID;
            return r;
        }
        if (c == '+' && k == 0) continue;
        if (c < '0' || c > '9') { r.st = ST_BAD_LEN; return r; }
        const uint64_t d = c - '0';
        if (v > (~0ull - d) / 10ull) ovf = true;
        else v = v * 10ull + d;
        digits = true;
    }
    r.st = ST_LONG_PREFIX;
    return r;
}

// (the rule under the name it had while it lived here: test hosts written against that name keep compiling)
FG_SLH bool utf8_err_at(uint32_t b, uint32_t p1, uint32_t p2, uint32_t p3) { return utf8::err_at(b, p1, p2, p3); }

// The sequential walk (what the device logic must reproduce, and the host hop of the entry points that take host buffers): frames
// into `starts` / `plens` while they fit `cap`; returns the stop reason.  bound as parse_prefix.
template <class Push>
inline uint32_t host_walk(const uint8_t* bytes, uint64_t nbytes, uint64_t bound, uint64_t* consumed, Push push) {
    uint64_t pos = 0;
    auto get = [&](uint64_t p) { return (uint32_t)bytes[p]; };
    for (;;) {
        const Prefix pr = parse_prefix(get, pos, nbytes, bound);
        if (pr.st != ST_VALID) {
            *consumed = pos;
            return pr.st;
        }
        push(pos, pr.plen, pr.len);
        pos += pr.plen + pr.len;
    }
}

}  // namespace syslen
}  // namespace fg
