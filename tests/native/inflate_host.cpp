// inflate_host.cpp -- the UDP input's inflate core (flowgger_amd/csrc/fg_inflate.hpp) on the CPU, one datagram per call, in the
// order the kernels of fg_udp.hip run it: count, write into a slot of exactly the counted size, UTF-8 (test infrastructure).
#include <vector>

#include "fg_inflate.hpp"
#include "fg_utf8.hpp"

using namespace fg::inflate;

extern "C" uint32_t fgi_tab_bytes_per_lane() { return kTabBytesPerLane; }
extern "C" uint32_t fgi_classify(const uint8_t* p, uint64_t len) { return classify(p, len); }

// out: at least max(max_inflated + 1, len) bytes.  Returns the final fg_udp_status; *size = the bytes of the datagram's slot (0 for a datagram
// the count pass drops), *drop = whether it is decoded.
extern "C" uint32_t fgi_unpack(const uint8_t* p, uint64_t len, uint32_t max_inflated, uint8_t* out, uint32_t* size, uint8_t* drop) {
    uint16_t h[kHalfWords];
    uint8_t b[kLenBytes];
    const Tabs t{h, b, 1u};
    uint32_t st = count_datagram(p, len, max_inflated, t, size);
    if (st == UDP_RAW)
        for (uint32_t k = 0; k < *size; ++k) out[k] = p[k];
    st = write_datagram(p, len, st, *size, t, out);
    *drop = st > UDP_GZIP;
    if (*drop) return st;
    if (fg::utf8::payload_bad(out, *size)) {
        *drop = 1;
        return UDP_BAD_UTF8;
    }
    return st;
}

// a batch, datagram by datagram: out_offsets[n + 1] / packed bytes / drop / status, as fg_udp_unpack_device leaves them
extern "C" uint64_t fgi_unpack_batch(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint32_t max_inflated, uint8_t* out, uint64_t out_cap,
                                     uint64_t* out_offsets, uint8_t* drop, uint8_t* status) {
    uint64_t room = max_inflated;  // (a bare record is not inflated: it takes what it is long)
    for (uint64_t i = 0; i < n; ++i) room = offsets[i + 1] - offsets[i] > room ? offsets[i + 1] - offsets[i] : room;
    std::vector<uint8_t> tmp(room + 16u);
    uint64_t o = 0;
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t size = 0;
        status[i] = (uint8_t)fgi_unpack(bytes + offsets[i], offsets[i + 1] - offsets[i], max_inflated, tmp.data(), &size, &drop[i]);
        out_offsets[i] = o;
        if (o + size <= out_cap)
            for (uint32_t k = 0; k < size; ++k) out[o + k] = tmp[k];
        o += size;
    }
    out_offsets[n] = o;
    return o;
}
