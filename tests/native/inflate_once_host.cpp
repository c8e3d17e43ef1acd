// inflate_once_host.cpp -- the one-walk form of the UDP input's inflate core (flowgger_amd/csrc/fg_inflate.hpp: stage_datagram) on the
// CPU, in the order the kernels of fg_udp.hip run it: every datagram staged in one walk, the sizes scanned, the spilled rows written
// into their slots by write_datagram, the others copied from their stage or from the datagram, UTF-8 (test infrastructure).
// Every stage is an allocation of exactly its capacity, so that a byte past one is a sanitizer's to report.
#include <cstring>
#include <vector>

#include "fg_inflate.hpp"
#include "fg_utf8.hpp"

using namespace fg::inflate;

extern "C" uint32_t fgo_stage_capacity(const uint8_t* p, uint64_t len, uint32_t max_inflated) { return stage_capacity(p, len, max_inflated); }

// w: the stage capacity of every datagram, or null for the policy's.  out null: nothing is packed (the sizing call of a test; the
// device entry has none).  Returns the packed bytes; *n_spilled = the datagrams whose bytes did not fit their stage.
extern "C" uint64_t fgo_unpack_batch(const uint8_t* bytes, const uint64_t* offsets, uint64_t n, uint32_t max_inflated, const uint32_t* w, uint8_t* out,
                                     uint64_t out_cap, uint64_t* out_offsets, uint8_t* drop, uint8_t* status, uint64_t* n_spilled) {
    uint16_t h[kHalfWords];
    uint8_t b[kLenBytes];
    const Tabs t{h, b, 1u};
    std::vector<std::vector<uint8_t>> stage(n);
    std::vector<uint32_t> size(n);
    std::vector<uint8_t> spilled(n);
    uint64_t o = 0;
    *n_spilled = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* p = bytes + offsets[i];
        const uint64_t len = offsets[i + 1] - offsets[i];
        const uint32_t cap = classify(p, len) == UDP_RAW ? 0u : w ? w[i] : stage_capacity(p, len, max_inflated);
        stage[i].resize(cap);
        uint32_t sp = 0;
        status[i] = (uint8_t)stage_datagram(p, len, max_inflated, cap, t, stage[i].data(), &size[i], &sp);
        drop[i] = status[i] > UDP_GZIP;
        spilled[i] = (uint8_t)sp;
        *n_spilled += sp;
        if (!sp && status[i] != UDP_RAW && size[i] > cap) return ~0ull;  // (a staged row lies in its stage)
        out_offsets[i] = o;
        o += size[i];
    }
    out_offsets[n] = o;
    if (!out || o > out_cap) return o;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* p = bytes + offsets[i];
        uint8_t* slot = out + out_offsets[i];
        if (spilled[i]) {
            const uint32_t st = write_datagram(p, offsets[i + 1] - offsets[i], status[i], size[i], t, slot);
            if (st != status[i]) {
                status[i] = (uint8_t)st;
                drop[i] = 1;
            }
        } else if (size[i]) {
            std::memcpy(slot, status[i] == UDP_RAW ? p : stage[i].data(), size[i]);
        }
        if (!drop[i] && fg::utf8::payload_bad(slot, size[i])) {
            status[i] = (uint8_t)UDP_BAD_UTF8;
            drop[i] = 1;
        }
    }
    return o;
}
