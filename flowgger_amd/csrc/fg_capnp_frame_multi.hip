// fg_capnp_frame_multi.hip -- launch code of the SEGMENTED Cap'n Proto stream framer: the chunks of many connections, one launch.  The
// per-tile logic is in fg_capnp_frame_multi.hpp and fg_capnp_frame.hpp (which the CPU suite runs over the wave emulation); nothing here
// decides anything about the streams.
//
// Reference: a CapnpSplitter per connection   src/flowgger/input/tcp/tcp_input.rs:39-47, splitter/capnp_splitter.rs:24-46
//
// One wave per workgroup everywhere:
//   k_seg_clamp (fg_frame_multi.hip)   the segment starts, non-decreasing and inside the buffer
//   k_cpm_roots     one lane per segment: the starts rounded down to a word, the bitmap bit of every non-empty segment's first word
//   k_cpm_mark      one wave per tile of 512 words (4 KiB), 10 384 B of LDS
//   k_cpm_nodes     the same, for the tiles with marked words
//   k_cpm_link      one lane per node slot
//   k_cpm_jump      one lane per node slot, launched ceil(log2(tiles)) times
//   k_cpm_collect   one lane per node slot
//   k_cpm_scan      one wave over the segments
//   k_cpm_emit      one wave per tile; the tiles without a true chain return at once
#include <hip/hip_runtime.h>

#include "fg_capnp_frame_multi.hpp"

namespace fg {
namespace capnpf {

__global__ __launch_bounds__(64) void k_cpm_roots(MScratch sc) {
    const uint64_t k = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (k <= sc.n_segs) seg_root(k, sc);
}
__global__ __launch_bounds__(64) void k_cpm_mark(const uint8_t* __restrict__ bytes, uint64_t nbytes, MScratch sc) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kLdsWords];
    mark_tile(bytes, nbytes, blockIdx.x, sc, lds, sc.segs());
}
__global__ __launch_bounds__(64) void k_cpm_nodes(const uint8_t* __restrict__ bytes, uint64_t nbytes, MScratch sc) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kLdsWords];
    nodes_tile(bytes, nbytes, blockIdx.x, sc, lds, sc.segs());
}
__global__ __launch_bounds__(64) void k_cpm_link(MScratch sc) {
    const uint32_t u = blockIdx.x * 64u + threadIdx.x;
    if (u < sc.node_cap) link_node(u, sc, sc.segs());
}
__global__ __launch_bounds__(64) void k_cpm_jump(MScratch sc, uint32_t r) {
    const uint32_t u = blockIdx.x * 64u + threadIdx.x;
    if (u < sc.node_cap) jump_round(u, r, sc);
}
__global__ __launch_bounds__(64) void k_cpm_collect(MScratch sc) {
    const uint32_t u = blockIdx.x * 64u + threadIdx.x;
    if (u < sc.node_cap) m_collect(u, sc);
}
__global__ __launch_bounds__(64) void k_cpm_scan(MScratch sc, uint64_t cap, uint64_t* __restrict__ offsets, uint8_t* __restrict__ kind,
                                                 uint64_t* __restrict__ seg_first, uint64_t* __restrict__ seg_consumed, uint8_t* __restrict__ seg_stop) {
    m_scan(sc, cap, offsets, kind, seg_first, seg_consumed, seg_stop);
}
__global__ __launch_bounds__(64) void k_cpm_emit(const uint8_t* __restrict__ bytes, uint64_t nbytes, MScratch sc, uint64_t* __restrict__ offsets,
                                                 uint8_t* __restrict__ kind, uint64_t cap) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kLdsWords];
    m_emit_tile(bytes, nbytes, blockIdx.x, sc, offsets, kind, cap, lds);
}

}  // namespace capnpf
}  // namespace fg

extern "C" int fg_launch_seg_clamp(const uint64_t* d_seg_starts, uint64_t n_segs, uint64_t nbytes, uint64_t* d_c, hipStream_t stream);

extern "C" uint64_t fg_capnp_frame_multi_scratch_bytes(uint64_t nbytes, uint64_t n_segs) {
    return fg::capnpf::m_scratch_words(nbytes, n_segs) * 4u + 256u;
}
// Queues the whole framer on `stream` (n_segs > 0); *d_hdr_out = the device words (H_DECLINE, H_NFRAMES = the slots, H_DONE) the caller
// reads once the stream has run.  d_offsets has cap + 1 entries, d_kind cap, d_seg_first n_segs + 1, d_seg_consumed and d_seg_stop
// n_segs; none of them is touched unless the slots fit.  d_bytes is readable up to nbytes rounded up to 16.  -1: sizes the scratch
// words cannot hold.
extern "C" int fg_launch_capnp_frame_multi(const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_seg_starts, uint64_t n_segs, uint8_t* scratch,
                                           uint64_t* d_offsets, uint8_t* d_kind, uint64_t cap, uint64_t* d_seg_first, uint64_t* d_seg_consumed,
                                           uint8_t* d_seg_stop, uint32_t** d_hdr_out, hipStream_t stream) {
    using namespace fg::capnpf;
    if (nbytes > kMaxBytes || n_segs == 0 || n_segs > kMaxSegs) return -1;
    const MScratch sc = m_carve(reinterpret_cast<uint32_t*>(scratch), nbytes, n_segs);
    (void)hipMemsetAsync(scratch, 0, m_zero_words(nbytes, n_segs) * 4u, stream);
    (void)hipMemsetAsync(sc.sg_stop, 0xFF, n_segs * 4u, stream);
    int rc = fg_launch_seg_clamp(d_seg_starts, n_segs, nbytes, sc.raw, stream);
    if (rc != 0) return rc;
    const uint32_t groups = (sc.node_cap + 63u) / 64u;
    hipLaunchKernelGGL(k_cpm_roots, dim3((uint32_t)((n_segs + 1u + 63u) / 64u)), dim3(64), 0, stream, sc);
    hipLaunchKernelGGL(k_cpm_mark, dim3(sc.tiles), dim3(64), 0, stream, d_bytes, nbytes, sc);
    hipLaunchKernelGGL(k_cpm_nodes, dim3(sc.tiles), dim3(64), 0, stream, d_bytes, nbytes, sc);
    hipLaunchKernelGGL(k_cpm_link, dim3(groups), dim3(64), 0, stream, sc);
    for (uint32_t r = 1; r <= sc.rounds; ++r) hipLaunchKernelGGL(k_cpm_jump, dim3(groups), dim3(64), 0, stream, sc, r);
    hipLaunchKernelGGL(k_cpm_collect, dim3(groups), dim3(64), 0, stream, sc);
    hipLaunchKernelGGL(k_cpm_scan, dim3(1), dim3(64), 0, stream, sc, cap, d_offsets, d_kind, d_seg_first, d_seg_consumed, d_seg_stop);
    hipLaunchKernelGGL(k_cpm_emit, dim3(sc.tiles), dim3(64), 0, stream, d_bytes, nbytes, sc, d_offsets, d_kind, cap);
    *d_hdr_out = sc.hdr;
    return (int)hipGetLastError();
}
