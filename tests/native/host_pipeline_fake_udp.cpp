// host_pipeline_fake_udp.cpp -- the fake launchers of host_pipeline_fake.cpp plus the UDP unpacker's one-walk launchers, which that file
// leaves undefined (they are weak references): host loops over flowgger_amd/csrc/fg_inflate.hpp with the contract of the kernels of
// fg_udp.hip, each counted, so that a test sees how often the walk ran.  A look at the packed buffer's capacity lets a test size a
// batch one byte beyond it.  Test infrastructure.
#include "host_pipeline_fake.cpp"

#include "../../flowgger_amd/csrc/fg_inflate.hpp"
#include "../../flowgger_amd/csrc/fg_utf8.hpp"

namespace {
unsigned long long g_udp_stage = 0, g_udp_respill = 0, g_udp_pack = 0;
}
extern "C" void fgf_udp_launches(unsigned long long out[3], int reset) {
    out[0] = g_udp_stage;
    out[1] = g_udp_respill;
    out[2] = g_udp_pack;
    if (reset) g_udp_stage = g_udp_respill = g_udp_pack = 0;
}
extern "C" unsigned long long fgf_packed_cap(const fg_ctx* ctx) { return ctx->d_sl_packed_cap; }

extern "C" uint64_t fg_udp_stage_bytes(uint64_t nbytes, uint64_t n) {
    return (uint64_t)fg::inflate::kStageK * nbytes + n * (uint64_t)(fg::inflate::kStageC + 32u) + 16u;
}
extern "C" int fg_launch_udp_stage(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint32_t max_inflated, uint32_t* d_stage_sizes,
                                   uint64_t* d_stage_sums, uint64_t* d_stage_off, uint8_t* d_stage, uint64_t stage_cap, uint32_t* d_sizes,
                                   uint64_t* d_block_sums, uint64_t* d_out_offsets, uint8_t* d_status, uint8_t* d_drop, uint8_t* d_spilled,
                                   uint32_t* d_n_spilled, hipStream_t s) {
    namespace inf = fg::inflate;
    FAKE_LAUNCH(s);
    ++g_udp_stage;
    uint16_t h[inf::kHalfWords];
    uint8_t b[inf::kLenBytes];
    const inf::Tabs t{h, b, 1u};
    uint64_t at = 0, o = 0;
    *d_n_spilled = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* p = d_bytes + d_offsets[i];
        const uint64_t len = d_offsets[i + 1] - d_offsets[i];
        const uint32_t w = inf::stage_capacity(p, len, max_inflated), slot = (w + 15u) & ~15u;
        if (at + slot > stage_cap) return -9;  // (the bound the host sized the stages by does not hold)
        d_stage_sizes[i] = slot;
        d_stage_off[i] = at;
        uint32_t sp = 0;
        d_status[i] = (uint8_t)inf::stage_datagram(p, len, max_inflated, w, t, d_stage + at, &d_sizes[i], &sp);
        d_drop[i] = d_status[i] > inf::UDP_GZIP;
        d_spilled[i] = (uint8_t)sp;
        *d_n_spilled += sp;
        d_out_offsets[i] = o;
        o += d_sizes[i];
        at += slot;
        if (i % 64 == 0) d_block_sums[i / 64] = d_stage_sums[i / 64] = 0;
        d_block_sums[i / 64] += d_sizes[i];
        d_stage_sums[i / 64] += slot;
    }
    d_stage_off[n] = at;
    d_out_offsets[n] = o;
    return 0;
}
extern "C" int fg_launch_udp_write_spilled(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_out_offsets, uint8_t* d_out,
                                           uint64_t out_cap, uint8_t* d_status, uint8_t* d_drop, const uint8_t* d_spilled, hipStream_t s) {
    namespace inf = fg::inflate;
    FAKE_LAUNCH(s);
    ++g_udp_respill;
    uint16_t h[inf::kHalfWords];
    uint8_t b[inf::kLenBytes];
    const inf::Tabs t{h, b, 1u};
    for (uint64_t i = 0; i < n; ++i) {
        if (!d_spilled[i]) continue;
        if (d_out_offsets[i + 1] > out_cap) return -9;
        const uint32_t st = inf::write_datagram(d_bytes + d_offsets[i], d_offsets[i + 1] - d_offsets[i], d_status[i],
                                                (uint32_t)(d_out_offsets[i + 1] - d_out_offsets[i]), t, d_out + d_out_offsets[i]);
        if (st != d_status[i]) {
            d_status[i] = (uint8_t)st;
            d_drop[i] = 1;
        }
    }
    return 0;
}
extern "C" int fg_launch_udp_pack(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_out_offsets, uint8_t* d_out,
                                  uint64_t out_cap, uint8_t* d_status, uint8_t* d_drop, const uint8_t* d_stage, const uint64_t* d_stage_off, uint64_t,
                                  const uint8_t* d_spilled, hipStream_t s) {
    namespace inf = fg::inflate;
    FAKE_LAUNCH(s);
    ++g_udp_pack;
    if (d_out_offsets[n] > out_cap) return -9;
    for (uint64_t i = 0; i < n; ++i) {
        uint8_t* slot = d_out + d_out_offsets[i];
        const uint64_t size = d_out_offsets[i + 1] - d_out_offsets[i];
        if (!d_spilled[i] && size) memcpy(slot, d_status[i] == inf::UDP_RAW ? d_bytes + d_offsets[i] : d_stage + d_stage_off[i], size);
        if (!d_drop[i] && fg::utf8::payload_bad(slot, (uint32_t)size)) {
            d_status[i] = (uint8_t)inf::UDP_BAD_UTF8;
            d_drop[i] = 1;
        }
    }
    return 0;
}
