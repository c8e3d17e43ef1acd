// fg_frame_multi.hip -- gfx950 kernels that frame the chunks of MANY connections in one launch: the buffer holds K segments back to
// back (seg_starts), each is framed as a stream of its own (`BufRead::lines()` / `split(0)` per connection: input/tcp/tcp_input.rs:39-47
// gives every connection its own splitter, splitter/line_splitter.rs:17-54), and the slots that come out -- bytes + n + 1 offsets + a
// per-slot kind -- are what the decode kernels take already.
//
// The framing itself is fg_frame.hip's, in both its forms; a segment boundary is three patches to the mask words that scan computes
// (fg_frame_multi.hpp has the logic and says why every bit has one owner):
//   classic   k_frame_scan -> k_seg_patch (one lane per boundary: masks in HBM, block counts adjusted) -> k_frame_prefix -> k_frame_emit
//   one-pass  k_frame_onepass_seg: fg_frame_kernels.hpp's body (frame_onepass) with a hook between "masks in LDS" and "count": a wave finds the boundaries
//             that touch its 16 KiB block by a binary search over the segment starts (none is the common case and costs that search),
//             patches its masks where they lie and counts again.  Look-back, spin bound and abort word are the body's own.
// Around them: k_seg_clamp (the segment starts as the kernels use them: non-decreasing, inside the buffer -- memory safety does not
// depend on the caller's list) and k_seg_finish (one lane per segment: its first slot, FG_SLOT_CARRY on the unterminated tail of a
// segment that is not final, the bytes its frames cover; one lane the slot count).
#include "fg_pipeline.hpp"
#include "fg_frame_kernels.hpp"
#include "fg_frame_multi.hpp"

namespace fg {

// c[k] = seg_starts[k] clamped into [c[k - 1], nbytes], c[0] = 0, c[n_segs] = nbytes: a running maximum; one workgroup.
__global__ __launch_bounds__(1024) void k_seg_clamp(const uint64_t* __restrict__ raw, uint64_t n_segs, uint64_t nbytes, uint64_t* __restrict__ c) {
    __shared__ uint64_t wave_max[16];
    __shared__ uint64_t carry_s;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (uint64_t k0 = 0; k0 <= n_segs; k0 += 1024) {
        const uint64_t k = k0 + tid;
        uint64_t v = 0;
        if (k != 0 && k <= n_segs) {
            v = raw[k];
            if (v > nbytes) v = nbytes;
        }
        uint64_t inc = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t y = __shfl_up(inc, d, 64);
            if (lane >= (uint32_t)d && y > inc) inc = y;
        }
        if (lane == 63) wave_max[wv] = inc;
        __syncthreads();
        uint64_t m = carry_s;
        for (uint32_t w = 0; w < wv; ++w) m = wave_max[w] > m ? wave_max[w] : m;
        if (inc > m) m = inc;
        if (k <= n_segs) c[k] = k == n_segs ? nbytes : m;
        __syncthreads();
        if (tid == 1023) carry_s = m;
        __syncthreads();
    }
}

// mask words of the classic form (HBM): word x / 16, delimiter bit x % 16, error bit 16 + x % 16; a delimiter that is new is counted
struct GlobalMaskSink {
    uint32_t* masks;
    uint32_t* counts;
    __device__ void set_delim(uint64_t x) const {
        const uint32_t bit = 1u << (uint32_t)(x & 15u);
        if (!(atomicOr(masks + (x >> 4), bit) & bit)) atomicAdd(counts + x / kFrameBlock, 1u);
    }
    __device__ void put_err(uint64_t x, bool v) const {
        const uint32_t bit = 0x10000u << (uint32_t)(x & 15u);
        if (v) atomicOr(masks + (x >> 4), bit);
        else atomicAnd(masks + (x >> 4), ~bit);
    }
    __device__ void or_err(uint64_t x) const { atomicOr(masks + (x >> 4), 0x10000u << (uint32_t)(x & 15u)); }
};

// classic form: one lane per segment index; the lane of a boundary's first index applies its patches
__global__ __launch_bounds__(256) void k_seg_patch(const uint8_t* __restrict__ bytes, uint64_t nbytes, const uint64_t* __restrict__ c, uint64_t n_segs,
                                                   uint32_t* __restrict__ masks, uint32_t* __restrict__ counts) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x + 1u;
    if (k >= n_segs) return;
    uint64_t prev = 0, next = 0;
    const uint64_t p = fmulti::boundary_at(c, n_segs, nbytes, k, &prev, &next);
    if (p == fmulti::kNoBoundary) return;
    fmulti::patch_boundary(p, prev, next, nbytes, [&](uint64_t x) -> uint32_t { return bytes[x]; }, GlobalMaskSink{masks, counts});
}

// one-pass form: the mask words of ONE 16 KiB block, in LDS; positions of other blocks are their waves' business
struct BlockMaskSink {
    uint32_t* m;
    uint64_t base;
    __device__ bool mine(uint64_t x) const { return x >= base && x - base < kFrameBlock; }
    __device__ void set_delim(uint64_t x) const {
        if (mine(x)) atomicOr(m + ((x - base) >> 4), 1u << (uint32_t)(x & 15u));
    }
    __device__ void put_err(uint64_t x, bool v) const {
        if (!mine(x)) return;
        const uint32_t bit = 0x10000u << (uint32_t)(x & 15u);
        if (v) atomicOr(m + ((x - base) >> 4), bit);
        else atomicAnd(m + ((x - base) >> 4), ~bit);
    }
    __device__ void or_err(uint64_t x) const {
        if (mine(x)) atomicOr(m + ((x - base) >> 4), 0x10000u << (uint32_t)(x & 15u));
    }
};
__device__ __forceinline__ uint64_t wave_uniform(uint64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}
struct Segments {
    static constexpr bool kSegmented = true;
    const uint64_t* c;  // clamped starts, n_segs + 1
    uint64_t n_segs;
    __device__ bool patch(const uint8_t* bytes, uint64_t nbytes, uint64_t base, uint32_t* m, uint32_t lane) const {
        if (n_segs < 2u) return false;
        base = wave_uniform(base);
        bool any = false;
        for (uint64_t kb = wave_uniform(fmulti::block_first_index(c, n_segs, base)); kb < n_segs; kb += kWave) {
            const uint64_t k = kb + lane;
            const bool in = k < n_segs && fmulti::block_touched_by(c[k], base, kFrameBlock);
            if (in) {
                uint64_t prev = 0, next = 0;
                const uint64_t p = fmulti::boundary_at(c, n_segs, nbytes, k, &prev, &next);
                if (p != fmulti::kNoBoundary)
                    fmulti::patch_boundary(p, prev, next, nbytes, [&](uint64_t x) -> uint32_t { return bytes[x]; }, BlockMaskSink{m, base});
            }
            const uint64_t ins = __ballot(in);
            any |= ins != 0ull;
            if (ins != ~0ull) break;  // (the starts are sorted: behind the first one past the block there is nothing for it)
        }
        return any;
    }
};
__global__ __launch_bounds__(kWave* kTileWaves) void k_frame_onepass_seg(const uint8_t* __restrict__ bytes, uint64_t nbytes, uint32_t delim_pat,
                                                                        uint64_t* __restrict__ desc, uint64_t* __restrict__ pref,
                                                                        uint32_t* __restrict__ abort_w, uint64_t* __restrict__ offsets,
                                                                        uint8_t* __restrict__ kind, uint64_t cap, uint64_t nblk,
                                                                        const uint64_t* __restrict__ c, uint64_t n_segs) {
    frame_onepass<false>(bytes, nbytes, delim_pat, desc, pref, abort_w, offsets, kind, cap, (uint64_t)0, nblk, nblk, kWholeStream, (uint8_t*)nullptr,
                         Segments{c, n_segs});
}

// One lane per segment (and one more for seg_first[n_segs]).  res[0] = the delimiter count the framing left (or kFrameAborted),
// res[1] = the slot count.  Nothing is written when the slots do not fit the capacity: the caller learns the need from res[1].
__global__ __launch_bounds__(256) void k_seg_finish(const uint8_t* __restrict__ bytes, uint64_t nbytes, uint32_t delim, const uint64_t* __restrict__ c,
                                                    const uint8_t* __restrict__ seg_final, uint64_t n_segs, const uint64_t* __restrict__ offsets,
                                                    uint8_t* __restrict__ kind, uint64_t cap, const uint64_t* __restrict__ d_total,
                                                    uint64_t* __restrict__ seg_first, uint64_t* __restrict__ seg_consumed, uint64_t* __restrict__ res) {
    const uint64_t k = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    const uint64_t total = *d_total;
    const uint64_t n = total == kFrameAborted ? 0ull : total + (bytes[nbytes - 1u] != delim ? 1u : 0u);  // (nbytes > 0: the launcher's business)
    if (k == 0) {
        res[0] = total;
        res[1] = n;
    }
    if (total == kFrameAborted || n > cap || k > n_segs) return;
    if (k == n_segs) {
        seg_first[k] = n;
        return;
    }
    const fmulti::SegResult r = fmulti::finish_segment(c, k, seg_final, offsets, n, delim, [&](uint64_t x) -> uint32_t { return bytes[x]; });
    seg_first[k] = r.first;
    seg_consumed[k] = r.consumed;
    if (r.carry < n) kind[r.carry] = fmulti::kSlotCarry;
}

}  // namespace fg

// k_seg_clamp for another unit (fg_syslen_multi.hip): c has n_segs + 1 entries
extern "C" int fg_launch_seg_clamp(const uint64_t* d_seg_starts, uint64_t n_segs, uint64_t nbytes, uint64_t* d_c, hipStream_t stream) {
    hipLaunchKernelGGL(fg::k_seg_clamp, dim3(1), dim3(1024), 0, stream, d_seg_starts, n_segs, nbytes, d_c);
    return (int)hipGetLastError();
}

// scratch: the framing's own (fg_frame_scratch_bytes), then the clamped segment starts (n_segs + 1 u64), then the two result words
static inline uint64_t multi_frame_part(uint64_t nbytes) { return (FrameScratch::bytes(frame_blocks(nbytes)) + 255u) & ~255ull; }
extern "C" uint64_t fg_frame_multi_scratch_bytes(uint64_t nbytes, uint64_t n_segs) {
    return multi_frame_part(nbytes) + (((n_segs + 1u) * 8u + 255u) & ~255ull) + 256u;
}
// nbytes > 0, n_segs > 0.  classic != 0: the three-kernel form.  *d_result: two device words -- the delimiter count, or ~0 when the
// one-pass look-back gave up (launch again with classic = 1: everything is rewritten), and the slot count.  d_kind (cap bytes) is
// cleared here; d_offsets has cap + 1 entries, d_seg_first n_segs + 1, d_seg_consumed n_segs.
extern "C" int fg_launch_frame_multi(const uint8_t* d_bytes, uint64_t nbytes, uint32_t delim, const uint64_t* d_seg_starts, const uint8_t* d_seg_final,
                                     uint64_t n_segs, uint8_t* scratch, uint64_t* d_offsets, uint8_t* d_kind, uint64_t cap, uint64_t* d_seg_first,
                                     uint64_t* d_seg_consumed, uint64_t** d_result, hipStream_t stream, int classic) {
    const uint64_t nblk = frame_blocks(nbytes);
    if (nbytes == 0 || n_segs == 0 || nblk > 0x7FFFFFFFull || n_segs > 0x7FFFFFFFull * 256u) return -1;
    uint64_t* c = reinterpret_cast<uint64_t*>(scratch + multi_frame_part(nbytes));
    uint64_t* res = reinterpret_cast<uint64_t*>(scratch + multi_frame_part(nbytes) + (((n_segs + 1u) * 8u + 255u) & ~255ull));
    *d_result = res;
    if (cap) (void)hipMemsetAsync(d_kind, 0, cap, stream);
    hipLaunchKernelGGL(fg::k_seg_clamp, dim3(1), dim3(1024), 0, stream, d_seg_starts, n_segs, nbytes, c);
    uint64_t* d_total = nullptr;
    if (!classic) {
        const FrameScratch sc(scratch, nblk);
        frame_onepass_reset(sc, nblk, nblk, true, stream);
        hipLaunchKernelGGL(fg::k_frame_onepass_seg, dim3((uint32_t)((nblk + fg::kTileWaves - 1) / fg::kTileWaves)), dim3(fg::kWave * fg::kTileWaves), 0, stream,
                           d_bytes, nbytes, delim * 0x01010101u, sc.desc, sc.pref, sc.abort_w, d_offsets, d_kind, cap, nblk, c, n_segs);
        d_total = sc.pref + nblk;
    } else {
        uint32_t *masks = nullptr, *counts = nullptr;
        int rc = fg_launch_frame_classic_scan(d_bytes, nbytes, delim, scratch, &masks, &counts, stream);
        if (rc != 0) return rc;
        if (n_segs > 1u)
            hipLaunchKernelGGL(fg::k_seg_patch, dim3((uint32_t)((n_segs - 1u + 255u) / 256u)), dim3(256), 0, stream, d_bytes, nbytes, c, n_segs, masks, counts);
        if ((rc = fg_launch_frame_classic_emit(nbytes, scratch, d_offsets, d_kind, cap, &d_total, stream)) != 0) return rc;
    }
    hipLaunchKernelGGL(fg::k_seg_finish, dim3((uint32_t)((n_segs + 1u + 255u) / 256u)), dim3(256), 0, stream, d_bytes, nbytes, delim, c, d_seg_final, n_segs,
                       d_offsets, d_kind, cap, d_total, d_seg_first, d_seg_consumed, res);
    return (int)hipGetLastError();
}
