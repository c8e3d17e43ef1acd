// host_pipeline_fake_kafka.cpp -- the fake launchers of host_pipeline_fake_deflate.cpp plus those of the Kafka message sets, which that
// file leaves undefined (they are weak references): host loops over flowgger_amd/csrc/fg_kafka.hpp on the wave emulation
// (kafka_driver.hpp) with the contract of the kernels of fg_kafka.hip, each counted.  Test infrastructure.
#include "host_pipeline_fake_deflate.cpp"

#include "kafka_driver.hpp"

namespace {
unsigned long long g_kf[5] = {0, 0, 0, 0, 0};  // sizes, write, cuts, wrap_sizes, wrap
}
extern "C" void fgf_kafka_launches(unsigned long long out[5], int reset) {
    for (int k = 0; k < 5; ++k) {
        out[k] = g_kf[k];
        if (reset) g_kf[k] = 0;
    }
}
extern "C" int fgf_ctx_wire(const fg_ctx* ctx) { return ctx->wire; }

extern "C" uint32_t fg_kafka_message_overhead(void) { return fg::kafka::kOverhead; }
extern "C" uint64_t fg_kafka_bound(uint64_t nbytes, uint64_t n, uint64_t n_members) { return fg::kafka::bound(nbytes, n, n_members); }
extern "C" int fg_launch_kafka_sizes(const uint64_t* d_off, const uint8_t* d_skip, uint64_t n, uint64_t nbytes, uint32_t* d_sizes, uint64_t*,
                                     uint64_t* d_set_offsets, uint32_t* d_err, hipStream_t s) {
    FAKE_LAUNCH(s);
    ++g_kf[0];
    *d_err = fgk::sizes(d_off, d_skip, n, nbytes, d_set_offsets) ? 0u : 1u;
    for (uint64_t i = 0; i < n; ++i) d_sizes[i] = (uint32_t)(d_set_offsets[i + 1] - d_set_offsets[i]);
    return 0;
}
extern "C" int fg_launch_kafka_write(const uint8_t* d_bytes, const uint64_t* d_off, const uint8_t* d_skip, uint64_t n, const uint64_t* d_set_offsets,
                                     uint8_t* d_set, uint64_t set_cap, int, hipStream_t s) {
    FAKE_LAUNCH(s);
    ++g_kf[1];
    if (d_set_offsets[n] > set_cap) return -9;  // (the buffer does not hold the set)
    fgk::write(d_bytes, d_off, d_skip, n, d_set_offsets, d_set, set_cap);
    return 0;
}
extern "C" int fg_launch_kafka_cuts(const uint64_t* d_set_offsets, const uint64_t* d_member_first, uint64_t n, uint64_t n_members, uint64_t* d_set_cuts,
                                    hipStream_t s) {
    FAKE_LAUNCH(s);
    ++g_kf[2];
    fgk::cuts(d_set_offsets, d_member_first, n, n_members, d_set_cuts);
    return 0;
}
extern "C" int fg_launch_kafka_wrap_sizes(const uint64_t* d_z_offsets, uint64_t n_members, uint32_t* d_wsize, uint32_t* d_npiece, uint64_t*,
                                          uint64_t* d_w_offsets, uint64_t* d_piece_first, uint32_t* d_err, hipStream_t s) {
    FAKE_LAUNCH(s);
    ++g_kf[3];
    *d_err = fgk::wrap_sizes(d_z_offsets, n_members, d_w_offsets, d_piece_first) ? 0u : 1u;
    for (uint64_t m = 0; m < n_members; ++m) {
        d_wsize[m] = (uint32_t)(d_w_offsets[m + 1] - d_w_offsets[m]);
        d_npiece[m] = (uint32_t)(d_piece_first[m + 1] - d_piece_first[m]);
    }
    return 0;
}
extern "C" int fg_launch_kafka_wrap(const uint8_t* d_z, const uint64_t* d_z_offsets, const uint64_t* d_piece_first, uint64_t n_members, uint64_t n_pieces,
                                    const uint64_t* d_w_offsets, uint8_t* d_w, uint64_t w_cap, uint32_t* d_piece_crc, int, hipStream_t s) {
    FAKE_LAUNCH(s);
    ++g_kf[4];
    if (n_pieces != d_piece_first[n_members] || d_w_offsets[n_members] > w_cap) return -9;
    fgk::wrap(d_z, d_z_offsets, d_piece_first, n_members, d_w_offsets, d_w, w_cap, d_piece_crc);
    return 0;
}
