// fg_syslen.hip -- launch code of the octet-counted ("syslen") framer.  The parsing and the per-tile logic are in fg_syslen.hpp (which
// the CPU suite runs over the wave emulation); nothing here decides anything about the stream.
//
// Reference: SyslenSplitter::run / read_msglen   src/flowgger/splitter/syslen_splitter.rs:17-57
//
// Four kernels, all one wave per workgroup (tools/kres.py, gfx950: 8 waves per SIMD each):
//   k_syslen_resolve  one wave per 4 KiB tile, 5200 B of LDS (the tile, its look-ahead, the exit list)
//   k_syslen_walk     one lane per inbox entry (16 per tile), four tiles per wave, no LDS
//   k_syslen_jump     one thread per node, launched ceil(log2(tiles)) times
//   k_syslen_emit     one wave per tile, 2064 B of LDS (a strip of 64 frames)
#include <hip/hip_runtime.h>

#include "fg_syslen.hpp"

namespace fg {
namespace syslen {

__global__ __launch_bounds__(64) void k_syslen_resolve(const uint8_t* __restrict__ bytes, uint64_t nbytes, Scratch sc) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kLdsWords];
    resolve_route(bytes, nbytes, blockIdx.x, sc, lds);
}
__global__ __launch_bounds__(64) void k_syslen_walk(const uint8_t* __restrict__ bytes, uint64_t nbytes, Scratch sc) {
    const uint32_t tile = blockIdx.x * (64u / kInbox) + threadIdx.x / kInbox;
    if (tile < sc.tiles) walk_node(bytes, nbytes, tile, threadIdx.x % kInbox, sc);
}
__global__ __launch_bounds__(64) void k_syslen_jump(Scratch sc, uint32_t r) {
    const uint32_t tile = blockIdx.x * (64u / kInbox) + threadIdx.x / kInbox;
    if (tile < sc.tiles) jump_round(tile, threadIdx.x % kInbox, r, sc);
}
__global__ __launch_bounds__(64) void k_syslen_emit(const uint8_t* __restrict__ bytes, uint64_t nbytes, Scratch sc, uint8_t* __restrict__ packed,
                                                    uint64_t* __restrict__ offsets, uint64_t* __restrict__ starts, uint8_t* __restrict__ bad,
                                                    uint64_t cap) {
    __shared__ uint32_t lds[kEmitLdsWords];
    emit_tile(bytes, nbytes, blockIdx.x, sc, packed, offsets, starts, bad, cap, lds);
}

}  // namespace syslen
}  // namespace fg

extern "C" uint64_t fg_syslen_scratch_bytes(uint64_t nbytes) { return fg::syslen::scratch_words(nbytes) * 4u + 256u; }
extern "C" uint64_t fg_syslen_max_bytes(void) { return fg::syslen::kMaxBytes; }
// Queues the whole framer on `stream`; *d_hdr_out = the device words (H_*: decline, stop reason, frames, consumed, payload bytes, done)
// the caller reads once the stream has run.  d_bad is cleared for `cap` frames.
extern "C" int fg_launch_syslen(const uint8_t* d_bytes, uint64_t nbytes, uint8_t* scratch, uint8_t* d_packed, uint64_t* d_offsets,
                                uint64_t* d_starts, uint8_t* d_bad, uint64_t cap, uint32_t** d_hdr_out, hipStream_t stream) {
    using namespace fg::syslen;
    if (nbytes > kMaxBytes) return -1;
    const Scratch sc = carve(reinterpret_cast<uint32_t*>(scratch), nbytes);
    (void)hipMemsetAsync(scratch, 0, scratch_zero_words(nbytes) * 4u, stream);
    if (cap) (void)hipMemsetAsync(d_bad, 0, cap, stream);
    const uint32_t per = 64u / kInbox, groups = (sc.tiles + per - 1u) / per;
    hipLaunchKernelGGL(k_syslen_resolve, dim3(sc.tiles), dim3(64), 0, stream, d_bytes, nbytes, sc);
    hipLaunchKernelGGL(k_syslen_walk, dim3(groups), dim3(64), 0, stream, d_bytes, nbytes, sc);
    for (uint32_t r = 1; r <= sc.rounds; ++r) hipLaunchKernelGGL(k_syslen_jump, dim3(groups), dim3(64), 0, stream, sc, r);
    hipLaunchKernelGGL(k_syslen_emit, dim3(sc.tiles), dim3(64), 0, stream, d_bytes, nbytes, sc, d_packed, d_offsets, d_starts, d_bad, cap);
    *d_hdr_out = sc.hdr;
    return (int)hipGetLastError();
}
