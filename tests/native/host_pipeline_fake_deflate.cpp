// host_pipeline_fake_deflate.cpp -- the fake launchers of host_pipeline_fake_udp.cpp plus the output compressor's, which those files leave
// undefined (they are weak references): host loops over flowgger_amd/csrc/fg_deflate.hpp on the wave emulation (deflate_driver.hpp) with
// the contract of the kernels of fg_deflate.hip, each counted.  A look at the capacities the compress stage grows lets a test watch
// them grow and be reused.  Test infrastructure.
#include "host_pipeline_fake_udp.cpp"

#include "deflate_driver.hpp"

namespace {
unsigned long long g_df[5] = {0, 0, 0, 0, 0};  // cuts, count, blocks, sizes, pack
}
extern "C" void fgf_deflate_launches(unsigned long long out[5], int reset) {
    for (int k = 0; k < 5; ++k) {
        out[k] = g_df[k];
        if (reset) g_df[k] = 0;
    }
}
extern "C" void fgf_deflate_caps(const fg_ctx* ctx, unsigned long long out[4]) {
    out[0] = ctx->d_df_slots_cap;
    out[1] = ctx->d_zout_cap;
    out[2] = ctx->h_zout_cap;
    out[3] = ctx->d_df_cut_cap;
}

extern "C" uint32_t fg_deflate_block_bytes(void) { return fg::deflate::kBlock; }
extern "C" uint64_t fg_deflate_bound(uint64_t nbytes, uint64_t n_members) { return fg::deflate::bound(nbytes, n_members); }
extern "C" uint64_t fg_deflate_slot_bytes(uint64_t nbytes, uint64_t n_blocks) { return fg::deflate::slot_bytes(nbytes, n_blocks); }
extern "C" int fg_launch_deflate_cuts(const uint64_t* d_off, uint64_t n, uint64_t coalesce, uint64_t member_bytes, uint32_t*, uint64_t*, uint64_t*,
                                      uint64_t* d_member_first, uint64_t* d_cuts, uint64_t* d_n_members, hipStream_t s) {
    FAKE_LAUNCH(s);
    ++g_df[0];
    *d_n_members = fgd::members(d_off, n, coalesce, member_bytes, d_member_first, d_cuts);
    return 0;
}
extern "C" int fg_launch_deflate_count(const uint64_t* d_cuts, uint64_t n_members, uint64_t nbytes, uint32_t* d_nblk, uint64_t*, uint64_t* d_blk_first,
                                       uint32_t* d_err, hipStream_t s) {
    FAKE_LAUNCH(s);
    ++g_df[1];
    *d_err = fgd::count(d_cuts, n_members, nbytes, d_blk_first) ? 0u : 1u;
    for (uint64_t m = 0; m < n_members; ++m) d_nblk[m] = (uint32_t)(d_blk_first[m + 1] - d_blk_first[m]);
    return 0;
}
extern "C" int fg_launch_deflate_blocks(const uint8_t* d_bytes, const uint64_t* d_cuts, const uint64_t* d_blk_first, uint64_t n_members, uint64_t n_blocks,
                                        uint8_t* d_slots, uint64_t slots_cap, uint32_t* d_blk_size, uint32_t* d_blk_crc, uint32_t* d_ticket, int,
                                        hipStream_t s) {
    FAKE_LAUNCH(s);
    ++g_df[2];
    if (n_blocks != d_blk_first[n_members] || slots_cap < fg::deflate::slot_bytes(d_cuts[n_members], n_blocks)) return -9;  // (the slots do not hold the batch)
    *d_ticket = (uint32_t)n_blocks;
    fgd::blocks(d_bytes, d_cuts, d_blk_first, n_members, d_slots, d_blk_size, d_blk_crc);
    return 0;
}
extern "C" int fg_launch_deflate_sizes(const uint64_t* d_cuts, const uint64_t* d_blk_first, uint64_t n_members, const uint32_t* d_blk_size,
                                       const uint32_t* d_blk_crc, uint32_t* d_blk_rel, uint32_t* d_member_crc, uint32_t* d_msize, uint64_t*,
                                       uint64_t* d_z_offsets, hipStream_t s) {
    FAKE_LAUNCH(s);
    ++g_df[3];
    fgd::sizes(d_cuts, d_blk_first, n_members, d_blk_size, d_blk_crc, d_blk_rel, d_member_crc, d_z_offsets);
    for (uint64_t m = 0; m < n_members; ++m) d_msize[m] = (uint32_t)(d_z_offsets[m + 1] - d_z_offsets[m]);
    return 0;
}
extern "C" int fg_launch_deflate_pack(const uint8_t* d_bytes, const uint64_t* d_cuts, const uint64_t* d_blk_first, uint64_t n_members, uint64_t n_blocks,
                                      const uint8_t* d_slots, const uint32_t* d_blk_size, const uint32_t* d_blk_rel, const uint32_t* d_member_crc,
                                      const uint64_t* d_z_offsets, uint8_t* d_z, uint64_t z_cap, hipStream_t s) {
    FAKE_LAUNCH(s);
    ++g_df[4];
    if (n_blocks != d_blk_first[n_members] || d_z_offsets[n_members] > z_cap) return -9;
    fgd::pack(d_bytes, d_cuts, d_blk_first, n_members, d_slots, d_blk_size, d_blk_rel, d_member_crc, d_z_offsets, d_z, z_cap);
    return 0;
}
