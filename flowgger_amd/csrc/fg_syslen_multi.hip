// fg_syslen_multi.hip -- launch code of the SEGMENTED octet-counted framer: the chunks of many connections, one launch.  The per-tile
// logic is in fg_syslen_multi.hpp and fg_syslen.hpp (which the CPU suite runs over the wave emulation); nothing here decides anything
// about the streams.
//
// Reference: a SyslenSplitter per connection   src/flowgger/input/tcp/tcp_input.rs:39-47, splitter/syslen_splitter.rs:10-57
//
// One wave per workgroup everywhere (tools/kres.py, gfx950: 8 waves per SIMD each):
//   k_seg_clamp (fg_frame_multi.hip)   the segment starts as the kernels use them
//   k_slm_resolve   one wave per 4 KiB tile, 5200 B of LDS
//   k_slm_walk      one lane per node (tiles x 16 inbox entries, then one root per segment), no LDS
//   k_slm_jump      one lane per node, launched ceil(log2(tiles)) times
//   k_slm_collect   one lane per node
//   k_slm_scan      one wave over the segments
//   k_slm_emit      one wave per tile, 3088 B of LDS (a strip of 64 frames)
// and, for fg_transcode_multi_batch, the per-segment cut behind the first payload that is not UTF-8:
//   k_slm_cut_find  one lane per frame, no LDS
//   k_slm_cut_mark  one lane per frame, no LDS
#include <hip/hip_runtime.h>

#include "../../include/fg_hip.h"
#include "fg_syslen_multi.hpp"

static_assert(fg::syslen::kCutMark == FG_SLOT_UNREACHED, "the cut writes fg_slot_kind values");

namespace fg {
namespace syslen {

__global__ __launch_bounds__(64) void k_slm_resolve(const uint8_t* __restrict__ bytes, uint64_t nbytes, MScratch sc) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kLdsWords];
    resolve_route(bytes, nbytes, blockIdx.x, sc, lds, sc.segs());
}
__global__ __launch_bounds__(64) void k_slm_walk(const uint8_t* __restrict__ bytes, MScratch sc) {
    const uint32_t u = blockIdx.x * 64u + threadIdx.x;
    if (u < sc.nodes) m_walk(bytes, u, sc);
}
__global__ __launch_bounds__(64) void k_slm_jump(MScratch sc, uint32_t r) {
    const uint32_t u = blockIdx.x * 64u + threadIdx.x;
    if (u < sc.nodes) m_jump(u, r, sc);
}
__global__ __launch_bounds__(64) void k_slm_collect(MScratch sc) {
    const uint32_t u = blockIdx.x * 64u + threadIdx.x;
    if (u < sc.nodes) m_collect(u, sc);
}
__global__ __launch_bounds__(64) void k_slm_scan(MScratch sc, uint64_t cap, uint64_t* __restrict__ offsets, uint64_t* __restrict__ seg_first,
                                                 uint64_t* __restrict__ seg_consumed, uint8_t* __restrict__ seg_stop) {
    m_scan(sc, cap, offsets, seg_first, seg_consumed, seg_stop);
}
__global__ __launch_bounds__(64) void k_slm_emit(const uint8_t* __restrict__ bytes, MScratch sc, uint8_t* __restrict__ packed,
                                                 uint64_t* __restrict__ offsets, uint64_t* __restrict__ starts, uint8_t* __restrict__ bad, uint64_t cap) {
    __shared__ uint32_t lds[kEmitLdsWords];
    m_emit(bytes, blockIdx.x, sc, packed, offsets, starts, bad, cap, lds);
}
__global__ __launch_bounds__(64) void k_slm_cut_find(const uint8_t* __restrict__ bad, uint64_t n, const uint64_t* __restrict__ seg_first,
                                                     uint64_t n_segs, uint32_t* __restrict__ cut) {
    const uint64_t i = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (i < n) cut_find(bad, i, seg_first, n_segs, cut);
}
__global__ __launch_bounds__(64) void k_slm_cut_mark(uint8_t* __restrict__ bad, uint64_t n, const uint64_t* __restrict__ seg_first, uint64_t n_segs,
                                                     const uint32_t* __restrict__ cut) {
    const uint64_t i = (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (i < n) cut_mark(bad, i, seg_first, n_segs, cut);
}

}  // namespace syslen
}  // namespace fg

extern "C" int fg_launch_seg_clamp(const uint64_t* d_seg_starts, uint64_t n_segs, uint64_t nbytes, uint64_t* d_c, hipStream_t stream);

extern "C" uint64_t fg_syslen_multi_scratch_bytes(uint64_t nbytes, uint64_t n_segs) {
    return fg::syslen::m_scratch_words(nbytes, n_segs) * 4u + 256u;
}
// Queues the whole framer on `stream` (nbytes > 0, n_segs > 0); *d_hdr_out = the device words (H_DECLINE, H_NFRAMES, H_TOTAL, H_DONE) the
// caller reads once the stream has run.  d_bad is cleared for `cap` frames; d_offsets has cap + 1 entries, d_starts cap, d_seg_first
// n_segs + 1, d_seg_consumed and d_seg_stop n_segs.  -1: sizes the scratch words cannot hold.
extern "C" int fg_launch_syslen_multi(const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_seg_starts, uint64_t n_segs, uint8_t* scratch,
                                      uint8_t* d_packed, uint64_t* d_offsets, uint64_t* d_starts, uint8_t* d_bad, uint64_t cap,
                                      uint64_t* d_seg_first, uint64_t* d_seg_consumed, uint8_t* d_seg_stop, uint32_t** d_hdr_out,
                                      hipStream_t stream) {
    using namespace fg::syslen;
    if (nbytes == 0 || nbytes > kMaxBytes || n_segs == 0 || n_segs > kMaxSegs) return -1;
    const MScratch sc = m_carve(reinterpret_cast<uint32_t*>(scratch), nbytes, n_segs);
    (void)hipMemsetAsync(scratch, 0, m_zero_words(nbytes, n_segs) * 4u, stream);
    (void)hipMemsetAsync(sc.sg_stop, 0xFF, n_segs * 4u, stream);
    if (cap) (void)hipMemsetAsync(d_bad, 0, cap, stream);
    int rc = fg_launch_seg_clamp(d_seg_starts, n_segs, nbytes, sc.c, stream);
    if (rc != 0) return rc;
    const uint32_t groups = (sc.nodes + 63u) / 64u;
    hipLaunchKernelGGL(k_slm_resolve, dim3(sc.tiles), dim3(64), 0, stream, d_bytes, nbytes, sc);
    hipLaunchKernelGGL(k_slm_walk, dim3(groups), dim3(64), 0, stream, d_bytes, sc);
    for (uint32_t r = 1; r <= sc.rounds; ++r) hipLaunchKernelGGL(k_slm_jump, dim3(groups), dim3(64), 0, stream, sc, r);
    hipLaunchKernelGGL(k_slm_collect, dim3(groups), dim3(64), 0, stream, sc);
    hipLaunchKernelGGL(k_slm_scan, dim3(1), dim3(64), 0, stream, sc, cap, d_offsets, d_seg_first, d_seg_consumed, d_seg_stop);
    hipLaunchKernelGGL(k_slm_emit, dim3(sc.tiles), dim3(64), 0, stream, d_bytes, sc, d_packed, d_offsets, d_starts, d_bad, cap);
    *d_hdr_out = sc.hdr;
    return (int)hipGetLastError();
}

extern "C" uint64_t fg_syslen_cut_scratch_bytes(uint64_t n_segs) { return fg::syslen::cut_words(n_segs) * 4u; }
// Queues the cut on `stream`: d_bad[n] (0 / 1) and d_seg_first[n_segs + 1] as the framer above left them, d_cut =
// fg_syslen_cut_scratch_bytes(n_segs) bytes.  Nothing to do without frames or segments.  -1: more frames than a 32-bit word numbers.
extern "C" int fg_launch_syslen_cut(uint8_t* d_bad, uint64_t n, const uint64_t* d_seg_first, uint64_t n_segs, uint32_t* d_cut, hipStream_t stream) {
    using namespace fg::syslen;
    if (n == 0 || n_segs == 0) return 0;
    if (n >= kCutNone || n_segs > kMaxSegs) return -1;
    (void)hipMemsetAsync(d_cut, 0xFF, cut_words(n_segs) * 4u, stream);
    const uint32_t groups = (uint32_t)((n + 63u) / 64u);
    hipLaunchKernelGGL(k_slm_cut_find, dim3(groups), dim3(64), 0, stream, d_bad, n, d_seg_first, n_segs, d_cut);
    hipLaunchKernelGGL(k_slm_cut_mark, dim3(groups), dim3(64), 0, stream, d_bad, n, d_seg_first, n_segs, d_cut);
    return (int)hipGetLastError();
}
