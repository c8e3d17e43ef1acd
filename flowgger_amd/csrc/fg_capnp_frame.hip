// fg_capnp_frame.hip -- launch code of the Cap'n Proto stream framer.  The rule and the per-tile logic are in fg_capnp_next.hpp and
// fg_capnp_frame.hpp (which the CPU suite runs over the wave emulation); nothing here decides anything about the stream.
//
// Reference: CapnpSplitter::run / capnp::serialize::read_message   src/flowgger/splitter/capnp_splitter.rs:24-46
//
// Five kernels, all one wave per workgroup:
//   k_capnpf_mark    one wave per tile of 512 words (4 KiB), 10 384 B of LDS (the tile and three words per word of it)
//   k_capnpf_nodes   the same, for the tiles with marked words
//   k_capnpf_link    one thread per node slot
//   k_capnpf_jump    one thread per node slot, launched ceil(log2(tiles)) times
//   k_capnpf_emit    one wave per tile; the tiles the chain does not enter return at once
#include <hip/hip_runtime.h>

#include "fg_capnp_frame.hpp"

namespace fg {
namespace capnpf {

__global__ __launch_bounds__(64) void k_capnpf_mark(const uint8_t* __restrict__ bytes, uint64_t nbytes, Scratch sc) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kLdsWords];
    mark_tile(bytes, nbytes, blockIdx.x, sc, lds);
}
__global__ __launch_bounds__(64) void k_capnpf_nodes(const uint8_t* __restrict__ bytes, uint64_t nbytes, Scratch sc) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kLdsWords];
    nodes_tile(bytes, nbytes, blockIdx.x, sc, lds);
}
__global__ __launch_bounds__(64) void k_capnpf_link(Scratch sc) {
    const uint32_t u = blockIdx.x * 64u + threadIdx.x;
    if (u < sc.node_cap) link_node(u, sc);
}
__global__ __launch_bounds__(64) void k_capnpf_jump(Scratch sc, uint32_t r) {
    const uint32_t u = blockIdx.x * 64u + threadIdx.x;
    if (u < sc.node_cap) jump_round(u, r, sc);
}
__global__ __launch_bounds__(64) void k_capnpf_emit(const uint8_t* __restrict__ bytes, uint64_t nbytes, Scratch sc, uint64_t* __restrict__ offsets,
                                                    uint64_t cap) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kLdsWords];
    emit_tile(bytes, nbytes, blockIdx.x, sc, offsets, cap, lds);
}

}  // namespace capnpf
}  // namespace fg

extern "C" uint64_t fg_capnp_frame_scratch_bytes(uint64_t nbytes) { return fg::capnpf::scratch_words(nbytes) * 4u + 256u; }
extern "C" uint64_t fg_capnp_frame_max_bytes(void) { return fg::capnpf::kMaxBytes; }
// Queues the whole framer on `stream`; *d_hdr_out = the device words (H_*: decline, stop reason, messages, consumed as a word index,
// done, nodes) the caller reads once the stream has run.
extern "C" int fg_launch_capnp_frame(const uint8_t* d_bytes, uint64_t nbytes, uint8_t* scratch, uint64_t* d_offsets, uint64_t cap,
                                     uint32_t** d_hdr_out, hipStream_t stream) {
    using namespace fg::capnpf;
    if (nbytes > kMaxBytes) return -1;
    const Scratch sc = carve(reinterpret_cast<uint32_t*>(scratch), nbytes);
    (void)hipMemsetAsync(scratch, 0, scratch_zero_words(nbytes) * 4u, stream);
    (void)hipMemsetAsync(sc.bitmap, 1, 1, stream);  // word 0: the stream's own start
    const uint32_t groups = (sc.node_cap + 63u) / 64u;
    hipLaunchKernelGGL(k_capnpf_mark, dim3(sc.tiles), dim3(64), 0, stream, d_bytes, nbytes, sc);
    hipLaunchKernelGGL(k_capnpf_nodes, dim3(sc.tiles), dim3(64), 0, stream, d_bytes, nbytes, sc);
    hipLaunchKernelGGL(k_capnpf_link, dim3(groups), dim3(64), 0, stream, sc);
    for (uint32_t r = 1; r <= sc.rounds; ++r) hipLaunchKernelGGL(k_capnpf_jump, dim3(groups), dim3(64), 0, stream, sc, r);
    hipLaunchKernelGGL(k_capnpf_emit, dim3(sc.tiles), dim3(64), 0, stream, d_bytes, nbytes, sc, d_offsets, cap);
    *d_hdr_out = sc.hdr;
    return (int)hipGetLastError();
}
