// fg_capnp_next.hpp -- where the Cap'n Proto message that starts at a word of a stream ends (capnp 0.14 serialize::read_message with
// default ReaderOptions, as CapnpSplitter::run calls it: src/flowgger/splitter/capnp_splitter.rs:24-46), and the sequential walk over
// a chunk: what the device framer (fg_capnp_frame.hpp), the host walk of the host-buffer entry points (fg_host_pipeline.cpp) and
// the CPU suite share.  No HIP, no wave primitives.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FG_CNH __host__ __device__ inline
#else
#define FG_CNH inline
#endif

namespace fg {
namespace capnpf {

constexpr uint64_t kMaxSegments = 512;    // "Too many segments" from this count on
constexpr uint64_t kMaxWords = 8ull << 20;  // "Message has N words, which is too large" beyond it
// fg_capnp_stop + "a whole message starts here"
enum { ST_CLEAN = 0, ST_TAIL = 1, ST_TOO_MANY_SEGMENTS = 2, ST_TOO_LARGE = 3, ST_VALID = 4 };
// the result words of a launch of the device framer (fg_capnp_frame.hpp, fg_capnp_frame_multi.hpp), as the host reads them back (fg_capi.cpp)
enum { H_DECLINE = 0, H_STOP = 1, H_NFRAMES = 2, H_CONSUMED = 3 /* a word index */, H_DONE = 4, H_NODES = 5, H_WORDS = 16 };

struct Next {
    uint32_t st;
    uint64_t words;  // ST_VALID: the words of the message, its segment table included
};
// The message at word w of a chunk of nbytes (a chunk starts at a message, so every start is a multiple of 8).  get32(p) = the
// little-endian u32 at byte p, p a multiple of 4 with p + 4 <= nbytes: nothing else is ever asked for.  At most 511 sizes are read.
template <class Get32>
FG_CNH Next next_at(Get32 get32, uint64_t w, uint64_t nbytes) {
    Next r{ST_CLEAN, 0ull};
    const uint64_t p = w * 8ull;
    if (p >= nbytes) return r;
    r.st = ST_TAIL;
    if (nbytes - p < 8ull) return r;
    const uint64_t segs = (uint64_t)get32(p) + 1ull;
    if (segs >= kMaxSegments) { r.st = ST_TOO_MANY_SEGMENTS; return r; }
    const uint64_t table = segs / 2ull + 1ull;  // words: roundup8(4 + 4 * segs) / 8
    if (nbytes - p < table * 8ull) return r;
    uint64_t words = 0;
    for (uint32_t k = 0; k < (uint32_t)segs; ++k) words += get32(p + 4ull + 4ull * k);
    if (words > kMaxWords) { r.st = ST_TOO_LARGE; return r; }
    if (nbytes - p < (table + words) * 8ull) return r;
    r.st = ST_VALID;
    r.words = table + words;
    return r;
}

// The sequential walk (what the device logic must reproduce): push(byte offset) for every whole message; returns the stop reason,
// *consumed = the position of the table at which the walk stopped.
template <class Push>
inline uint32_t host_walk(const uint8_t* bytes, uint64_t nbytes, uint64_t* consumed, Push push) {
    auto get32 = [&](uint64_t p) { uint32_t v; memcpy(&v, bytes + p, 4); return v; };
    uint64_t w = 0;
    for (;;) {
        const Next nx = next_at(get32, w, nbytes);
        if (nx.st != ST_VALID) {
            *consumed = w * 8ull;
            return nx.st;
        }
        push(w * 8ull);
        w += nx.words;
    }
}

}  // namespace capnpf
}  // namespace fg
