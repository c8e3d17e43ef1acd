// host_pipeline_fake_deflate_dyn.cpp -- the fake launchers of host_pipeline_fake_deflate.cpp plus the one it leaves undefined, the block
// launcher of FG_DEFLATE_DYNAMIC: a host loop over fg::deflate::compress_block_dyn (deflate_dyn_driver.hpp) with the contract of
// fg_launch_deflate_blocks_dyn, counted apart from the fixed mode's.  Test infrastructure.
#include "host_pipeline_fake_deflate.cpp"

#include "deflate_dyn_driver.hpp"

namespace {
unsigned long long g_df_dyn = 0;
}
extern "C" unsigned long long fgf_deflate_dyn_launches(int reset) {
    const unsigned long long v = g_df_dyn;
    if (reset) g_df_dyn = 0;
    return v;
}
extern "C" int fgf_deflate_mode(const fg_ctx* ctx) { return ctx->deflate_mode; }
extern "C" int fg_launch_deflate_blocks_dyn(const uint8_t* d_bytes, const uint64_t* d_cuts, const uint64_t* d_blk_first, uint64_t n_members,
                                            uint64_t n_blocks, uint8_t* d_slots, uint64_t slots_cap, uint32_t* d_blk_size, uint32_t* d_blk_crc,
                                            uint32_t* d_ticket, int, hipStream_t s) {
    FAKE_LAUNCH(s);
    ++g_df_dyn;
    if (n_blocks != d_blk_first[n_members] || slots_cap < fg::deflate::slot_bytes(d_cuts[n_members], n_blocks)) return -9;  // (the slots do not hold the batch)
    *d_ticket = (uint32_t)n_blocks;
    fgd::blocks_dyn(d_bytes, d_cuts, d_blk_first, n_members, d_slots, d_blk_size, d_blk_crc, nullptr);
    return 0;
}
