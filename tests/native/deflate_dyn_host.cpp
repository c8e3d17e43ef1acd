// deflate_dyn_host.cpp -- the output compressor's core in both modes on the CPU (deflate_host.cpp with the mode, the per-block report of
// compress_block_dyn and the code builder alone); test infrastructure.
#include "deflate_dyn_driver.hpp"

extern "C" uint32_t fgd_block_bytes() { return fg::deflate::kBlock; }
extern "C" uint64_t fgd_bound(uint64_t nbytes, uint64_t n_members) { return fg::deflate::bound(nbytes, n_members); }
extern "C" uint64_t fgd_deflate_mode(const uint8_t* bytes, uint64_t nbytes, const uint64_t* cuts, uint64_t n_members, int mode, uint8_t* z, uint64_t z_cap,
                                     uint64_t* z_offsets, uint32_t* blk_info) {
    return fgd::deflate_mode(bytes, nbytes, cuts, n_members, mode, z, z_cap, z_offsets, blk_info);
}
extern "C" uint32_t fgd_build_lengths(const uint32_t* freq, uint32_t n, uint32_t limit, uint32_t* lengths, uint32_t* limited) {
    return fgd::build(freq, n, limit, lengths, limited);
}
