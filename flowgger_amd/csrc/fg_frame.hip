// fg_frame.hip -- gfx950 kernels for the step BEFORE Decoder::decode: framing a raw byte stream
// into lines and rejecting lines that are not valid UTF-8.
//
// Reference semantics:
//   LineSplitter  `for line in buf_reader.lines()`   src/flowgger/splitter/line_splitter.rs:17-25
//       BufRead::lines(): split on '\n'; the '\n' and ONE preceding '\r' are not part of the line;
//       a final unterminated piece is a line if it is non-empty; invalid UTF-8 -> InvalidData ->
//       stderr "Invalid UTF-8 input", the line is dropped.
//   NulSplitter   `for line in buf_reader.split(0)` + str::from_utf8   nul_splitter.rs:18-40
//   (SyslenSplitter's "<len> " prefix chain has its own kernels: fg_syslen.hip.)
//
// Output: frame i = bytes[offsets[i] .. offsets[i+1]) INCLUDING its terminator (the decode
// kernels strip "\n" / "\r\n" / "\0" themselves, fg_decode_frames_device), bad_utf8[i] = 1 when
// the frame is not valid UTF-8.
//
// ONE streaming pass (k_frame_onepass, round 4): a wave takes a 16 KiB tile -- 16 B per lane and row, per 16-byte chunk a delimiter
// mask and a UTF-8 error mask -- counts its delimiters, learns how many lie before its tile from the tiles before it (a chained
// scan with decoupled look-back over one 8-byte descriptor per tile: flag | count), and writes the offsets of ITS delimiters and the
// bad-UTF-8 flags of ITS error positions from the masks it still holds (transposed through 4 KiB of LDS so that a lane owns 256
// consecutive bytes).  The stream is read once; nothing but the descriptors is written besides the output.
// The classic form (k_frame_scan -> k_frame_prefix -> k_frame_emit: masks to HBM, a one-workgroup scan of the tile counts, a second
// pass over the masks; 39 GB of traffic for a 25.5 GB stream) is kept as the fall-back: a wave that waits on a predecessor's
// descriptor longer than kSpinLimit polls raises an abort word and leaves the sentinel as the range's total, the launcher's caller
// sees it and runs the classic kernels (forward progress of the chain rests on workgroups being dispatched in index order; the bound makes a
// platform where that ever fails slow, not hung).
// UTF-8 validity is judged per byte position from the byte and its three predecessors (the
// table-free form of the well-formedness rules, Unicode 15 Table 3-7), so blocks, waves and
// lanes need no carried state; an error is always flagged inside the frame it belongs to
// because the terminators are ASCII.  The rule and the 16-byte chunk classifier are the fused decoders' (fg_fuse.hpp
// fuse::chunk_masks); the scan of a block and the emit of a lane's masks are written once, in fg_frame_kernels.hpp, for both forms
// and for the segmented framer (fg_frame_multi.hip).
#include "fg_pipeline.hpp"
#include "fg_frame_kernels.hpp"

namespace fg {

// pass 1.  masks[chunk] = delimiter mask | error mask << 16 (chunk = 16 bytes); counts[block].
// (blk0: first block of the range this launch covers -- a SLICE of the stream whose bytes have arrived; the pipelined host path frames
//  slice by slice while the next one is still on the link)
// COPY (frame_scan_block): the upload of the raw-stream host path without the copy engine (fg_host_pipeline.cpp).
template <bool COPY>
__global__ __launch_bounds__(kWave) void k_frame_scan(const uint8_t* __restrict__ bytes, uint64_t nbytes, uint32_t delim_pat,
                                                     uint32_t* __restrict__ masks, uint32_t* __restrict__ counts, uint64_t blk0,
                                                     uint8_t* __restrict__ copy_to) {
    const uint32_t lane = threadIdx.x;
    const uint64_t blk = blk0 + blockIdx.x;
    uint32_t total = frame_scan_block<COPY>(bytes, nbytes, delim_pat, blk * kFrameBlock, lane, copy_to,
                                            [&](int k, uint32_t m) { masks[blk * (kFrameBlock / 16u) + k * kWave + lane] = m; });
    // wave sum -> counts[blk]
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) total += __shfl_xor(total, d, kWave);
    if (lane == 0) counts[blk] = total;
}

// exclusive scan of counts[0..nblk) -> pref[0..nblk], pref[nblk] = total; one workgroup.  carry_in: the scan continues the one
// of the blocks before (pref[0] already holds their total: the previous slice's pref[nblk]).
__global__ __launch_bounds__(1024) void k_frame_prefix(const uint32_t* __restrict__ counts, uint64_t nblk, uint64_t* __restrict__ pref,
                                                       uint32_t carry_in) {
    __shared__ uint64_t wave_tot[16];
    __shared__ uint64_t carry_s;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    if (tid == 0) carry_s = carry_in ? pref[0] : 0;
    __syncthreads();
    for (uint64_t b0 = 0; b0 < nblk; b0 += 1024) {
        const uint64_t i = b0 + tid;
        uint64_t x = i < nblk ? counts[i] : 0;
        uint64_t inc = x;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            uint64_t y = __shfl_up(inc, d, 64);
            if (lane >= (uint32_t)d) inc += y;
        }
        if (lane == 63) wave_tot[wv] = inc;
        __syncthreads();
        uint64_t off = carry_s;
        for (uint32_t w = 0; w < wv; ++w) off += wave_tot[w];
        if (i < nblk) pref[i] = off + inc - x;
        __syncthreads();
        if (tid == 1023) carry_s = off + inc;
        __syncthreads();
    }
    if (tid == 0) pref[nblk] = carry_s;
}

// pass 2.  A lane owns 16 consecutive chunks (256 bytes) of its block.
// (blk0 / whole: see k_frame_scan; a slice launch leaves the end of a final unterminated frame to the host, which knows the total
//  only after the last slice)
__global__ __launch_bounds__(kWave) void k_frame_emit(const uint32_t* __restrict__ masks, const uint64_t* __restrict__ pref,
                                                     uint64_t nbytes, uint64_t nblk, uint64_t* __restrict__ offsets,
                                                     uint8_t* __restrict__ bad, uint64_t cap, uint64_t blk0, uint32_t whole) {
    const uint32_t lane = threadIdx.x;
    const uint64_t blk = blk0 + blockIdx.x;
    uint32_t w[16], any_err;
    const uint32_t mine = frame_lane_words(masks + blk * (kFrameBlock / 16u) + lane * 16u, w, &any_err);
    uint32_t total;
    const uint32_t ex = wave_exclusive_sum(mine, &total);
    uint64_t rank = pref[blk] + ex;  // delimiters before this lane's first byte
    if (blk == 0 && lane == 0) {
        offsets[0] = 0;
        if (whole) {
            const uint64_t total_delims = pref[nblk];
            if (total_delims + 1 <= cap) offsets[total_delims + 1] = nbytes;  // end of a final unterminated frame
        }
    }
    if (mine == 0 && any_err == 0) return;
    frame_emit_lane(w, rank, blk * (uint64_t)kFrameBlock + (uint64_t)lane * 256u, offsets, bad, cap);
}

// the one-pass form (fg_frame_kernels.hpp frame_onepass: the segmented framer of fg_frame_multi.hip instantiates the same body)
template <bool COPY>
__global__ __launch_bounds__(kWave* kTileWaves) void k_frame_onepass(const uint8_t* __restrict__ bytes, uint64_t nbytes, uint32_t delim_pat,
                                                                    uint64_t* __restrict__ desc, uint64_t* __restrict__ pref,
                                                                    uint32_t* __restrict__ abort_w, uint64_t* __restrict__ offsets,
                                                                    uint8_t* __restrict__ bad, uint64_t cap, uint64_t tile0, uint64_t blk1,
                                                                    uint64_t nblk, uint32_t whole, uint8_t* __restrict__ copy_to) {
    frame_onepass<COPY>(bytes, nbytes, delim_pat, desc, pref, abort_w, offsets, bad, cap, tile0, blk1, nblk, whole, copy_to, NoSegments{});
}

}  // namespace fg

extern "C" uint64_t fg_frame_scratch_bytes(uint64_t nbytes) { return FrameScratch::bytes(frame_blocks(nbytes)); }
extern "C" uint64_t fg_frame_block_bytes(void) { return fg::kFrameBlock; }
extern "C" uint64_t fg_frame_slice_align(void) { return (uint64_t)fg::kFrameBlock * fg::kTileWaves; }  // slice boundaries: whole tiles

// A kernel with a COPY twin (same parameters: the bytes first, copy_to last).  src != null: the bytes are read from `src` (the device
// view of the caller's pinned buffer, same offsets) and stored to d_bytes by the kernel itself -- no upload has to have happened.
template <class K, class... Mid>
static void launch_copy_twin(K plain, K copy, uint32_t grid, uint32_t block, hipStream_t stream, const uint8_t* d_bytes, const uint8_t* src, Mid... mid) {
    if (src) hipLaunchKernelGGL(copy, dim3(grid), dim3(block), 0, stream, src, mid..., const_cast<uint8_t*>(d_bytes));
    else hipLaunchKernelGGL(plain, dim3(grid), dim3(block), 0, stream, d_bytes, mid..., (uint8_t*)nullptr);
}
// The blocks [blk0, blk1) of a stream of nblk, in either form; the launchers below say what they promise.  whole: the range is the
// stream (the kernels then write the end of a final unterminated frame themselves).
static void classic_scan(const FrameScratch& sc, const uint8_t* d_bytes, uint64_t nbytes, uint32_t delim, uint64_t blk0, uint64_t blk1, hipStream_t stream,
                         const uint8_t* src) {
    launch_copy_twin(fg::k_frame_scan<false>, fg::k_frame_scan<true>, (uint32_t)(blk1 - blk0), fg::kWave, stream, d_bytes, src, nbytes, delim * 0x01010101u,
                     sc.masks, sc.counts, blk0);
}
static void classic_emit(const FrameScratch& sc, uint64_t nbytes, uint64_t nblk, uint64_t* d_offsets, uint8_t* d_bad, uint64_t cap, uint64_t blk0,
                         uint64_t blk1, hipStream_t stream, bool whole) {
    hipLaunchKernelGGL(fg::k_frame_prefix, dim3(1), dim3(1024), 0, stream, sc.counts + blk0, blk1 - blk0, sc.pref + blk0, blk0 ? 1u : 0u);
    hipLaunchKernelGGL(fg::k_frame_emit, dim3((uint32_t)(blk1 - blk0)), dim3(fg::kWave), 0, stream, sc.masks, sc.pref, nbytes, nblk, d_offsets, d_bad, cap, blk0,
                       whole ? 1u : 0u);
}
// classic: 0 the one-pass form, 1 the three-kernel form, 2 the one-pass form with its self-test stall (the second tile of the STREAM's
// first launch publishes nothing: a stream of three tiles or more WILL report FG_FRAME_ABORTED)
static int frame_range(const uint8_t* d_bytes, uint64_t nbytes, uint32_t delim, uint8_t* scratch, uint64_t* d_offsets, uint8_t* d_bad, uint64_t cap,
                       uint64_t blk0, uint64_t blk1, uint64_t** d_total_out, hipStream_t stream, const uint8_t* src, int classic, bool whole) {
    const uint64_t nblk = frame_blocks(nbytes);
    if (nblk > 0x7FFFFFFFull || blk1 > nblk || blk0 >= blk1) return -1;
    const FrameScratch sc(scratch, nblk);
    *d_total_out = sc.pref + blk1;
    if (classic == 1) {
        classic_scan(sc, d_bytes, nbytes, delim, blk0, blk1, stream, src);
        classic_emit(sc, nbytes, nblk, d_offsets, d_bad, cap, blk0, blk1, stream, whole);
        return (int)hipGetLastError();
    }
    // (tiles of kTileWaves blocks: a slice that is not the stream's first starts at a multiple of fg_frame_slice_align())
    if (blk0 % fg::kTileWaves) return -1;
    frame_onepass_reset(sc, nblk, blk1, blk0 == 0, stream);
    const uint64_t tile0 = blk0 / fg::kTileWaves;
    const uint32_t flags = (whole ? fg::kWholeStream : 0u) | (classic == 2 && blk0 == 0 ? fg::kSelfTestStall : 0u);
    launch_copy_twin(fg::k_frame_onepass<false>, fg::k_frame_onepass<true>, (uint32_t)((blk1 + fg::kTileWaves - 1) / fg::kTileWaves - tile0),
                     fg::kWave * fg::kTileWaves, stream, d_bytes, src, nbytes, delim * 0x01010101u, sc.desc, sc.pref, sc.abort_w, d_offsets, d_bad, cap, tile0,
                     blk1, nblk, flags);
    return (int)hipGetLastError();
}

// The whole stream.  *d_total_out: the device word that will hold the delimiter count -- or FG_FRAME_ABORTED (~0), after which the
// caller launches again with classic = 1 (same arguments; everything is rewritten).
extern "C" int fg_launch_frame(const uint8_t* d_bytes, uint64_t nbytes, uint32_t delim, uint8_t* scratch, uint64_t* d_offsets,
                               uint8_t* d_bad, uint64_t cap, uint64_t** d_total_out, hipStream_t stream, int classic) {
    const uint64_t nblk = frame_blocks(nbytes);
    if (nblk > 0x7FFFFFFFull) return -1;
    (void)hipMemsetAsync(d_bad, 0, cap, stream);
    return frame_range(d_bytes, nbytes, delim, scratch, d_offsets, d_bad, cap, 0, nblk, d_total_out, stream, nullptr, classic, true);
}

// The classic form in two halves, for a caller that edits the masks and the block counts between them (fg_frame_multi.hip: segment
// boundaries): the scan, then prefix + emit.  Same scratch, same results as fg_launch_frame(classic = 1); d_bad is the caller's to clear.
extern "C" int fg_launch_frame_classic_scan(const uint8_t* d_bytes, uint64_t nbytes, uint32_t delim, uint8_t* scratch, uint32_t** d_masks,
                                            uint32_t** d_counts, hipStream_t stream) {
    const uint64_t nblk = frame_blocks(nbytes);
    if (nblk > 0x7FFFFFFFull) return -1;
    const FrameScratch sc(scratch, nblk);
    *d_masks = sc.masks;
    *d_counts = sc.counts;
    classic_scan(sc, d_bytes, nbytes, delim, 0, nblk, stream, nullptr);
    return (int)hipGetLastError();
}
extern "C" int fg_launch_frame_classic_emit(uint64_t nbytes, uint8_t* scratch, uint64_t* d_offsets, uint8_t* d_bad, uint64_t cap,
                                            uint64_t** d_total_out, hipStream_t stream) {
    const uint64_t nblk = frame_blocks(nbytes);
    if (nblk > 0x7FFFFFFFull) return -1;
    const FrameScratch sc(scratch, nblk);
    *d_total_out = sc.pref + nblk;
    classic_emit(sc, nbytes, nblk, d_offsets, d_bad, cap, 0, nblk, stream, true);
    return (int)hipGetLastError();
}

// One SLICE of the stream: the blocks [blk0, blk1) (slice boundaries are multiples of the 16 KiB block; the last slice ends at
// frame_blocks(nbytes)), whose bytes -- and everything before them -- are in d_bytes (or, src != null, arrive there through the scan:
// launch_copy_twin).  Continues the delimiter ranks where the slice before stopped; *d_total_out = the device word that holds the
// delimiters up to the end of this slice.  d_bad must have been cleared for the whole batch beforehand; offsets[total + 1] of a final
// unterminated frame is the caller's business.  Slices of one stream are launched in order, all classic or all one-pass (the first
// slice clears the descriptors of the whole stream).
extern "C" int fg_launch_frame_slice(const uint8_t* d_bytes, uint64_t nbytes, uint32_t delim, uint8_t* scratch, uint64_t* d_offsets,
                                     uint8_t* d_bad, uint64_t cap, uint64_t blk0, uint64_t blk1, uint64_t** d_total_out,
                                     hipStream_t stream, const uint8_t* src, int classic) {
    return frame_range(d_bytes, nbytes, delim, scratch, d_offsets, d_bad, cap, blk0, blk1, d_total_out, stream, src, classic, false);
}

// One 8-byte word from device memory into ANY device-addressable memory (a pinned host word included) by a kernel: the sliced host
// paths bring their per-slice counters back this way, because a hipMemcpy of 8 bytes queues on the same copy engine as the 32 MiB
// uploads that were issued ahead of it and would wait for all of them (profiles/r04a_timeline_*).
namespace fg {
__global__ void k_poke64(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst) {
    if (threadIdx.x == 0) {
        const uint64_t v = *src;
        __atomic_store_n(dst, v, __ATOMIC_RELAXED);
        __threadfence_system();
    }
}
}  // namespace fg
extern "C" int fg_launch_poke64(const uint64_t* d_src, uint64_t* dst_devview, hipStream_t stream) {
    hipLaunchKernelGGL(fg::k_poke64, dim3(1), dim3(64), 0, stream, d_src, dst_devview);
    return (int)hipGetLastError();
}

