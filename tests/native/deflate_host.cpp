// deflate_host.cpp -- the output compressor's core (flowgger_amd/csrc/fg_deflate.hpp) on the CPU, a wave being 64 fibers, in the order the
// kernels of fg_deflate.hip run it (test infrastructure).
#include "deflate_driver.hpp"

extern "C" uint32_t fgd_block_bytes() { return fg::deflate::kBlock; }
extern "C" uint64_t fgd_bound(uint64_t nbytes, uint64_t n_members) { return fg::deflate::bound(nbytes, n_members); }
extern "C" uint64_t fgd_deflate(const uint8_t* bytes, uint64_t nbytes, const uint64_t* cuts, uint64_t n_members, uint8_t* z, uint64_t z_cap,
                                uint64_t* z_offsets) {
    return fgd::deflate(bytes, nbytes, cuts, n_members, z, z_cap, z_offsets);
}
extern "C" uint64_t fgd_members(const uint64_t* off, uint64_t n, uint64_t coalesce, uint64_t member_bytes, uint64_t* member_first, uint64_t* cuts) {
    return fgd::members(off, n, coalesce, member_bytes, member_first, cuts);
}
