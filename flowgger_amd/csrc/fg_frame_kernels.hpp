// fg_frame_kernels.hpp -- what the two framing units share, fg_frame.hip (one stream per launch) and fg_frame_multi.hip (the chunks of
// many connections per launch), and nobody else: the scan body (a 16 KiB block -> per 16-byte chunk one mask word: delimiter mask |
// error mask << 16), the emit body (a lane's mask words -> offsets and bad-UTF-8 flags), the body of the one-pass chained scan built
// from the two, and the layout of a launch's scratch.  The chunk classifier and the dword-parallel UTF-8 rule are fg_fuse.hpp's
// (fuse::chunk_masks, the ones the fused decoders run; the scalar form of the rule is fg_utf8.hpp).  Include after fg_pipeline.hpp.
#pragma once
#include "fg_fuse.hpp"

namespace fg {

constexpr uint32_t kFrameBlock = 16384;  // bytes per wave-block
constexpr uint32_t kFrameRows = kFrameBlock / (16 * kWave);  // 16

// ---- the scan body --------------------------------------------------------------------------------------------------------
// The wave's 16 KiB block at `base` (a block AT or behind the stream's end is empty: it only carries the "cut off by the end" check)
// through its sixteen rows, 16 B per lane and row: store(k, word) gets the mask word of chunk k * kWave + lane of the block; returns
// the lane's delimiter count.  COPY: the stream is read where the caller has it -- pinned host memory, over the link, once -- and
// written to its place in HBM on the way (copy_to + the same offsets).
template <bool COPY, class Store>
__device__ __forceinline__ uint32_t frame_scan_block(const uint8_t* __restrict__ bytes, uint64_t nbytes, uint32_t delim_pat, uint64_t base, uint32_t lane,
                                                     uint8_t* __restrict__ copy_to, Store&& store) {
    const uint64_t left = base < nbytes ? nbytes - base : 0ull;
    const uint32_t span = left >= kFrameBlock ? kFrameBlock : (uint32_t)((left + 15u) & ~15ull);
    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(bytes + (base < nbytes ? base : 0ull)), (short)0, (int)span, 0x00020000);
    u32x4 v[kFrameRows];
#pragma unroll
    for (int k = 0; k < (int)kFrameRows; ++k)
        v[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(lane * 16u + k * 1024u), 0, COPY ? FG_STREAM_AUX : 0);
    if constexpr (COPY) {
        __amdgpu_buffer_rsrc_t dst = __builtin_amdgcn_make_buffer_rsrc(copy_to + (base < nbytes ? base : 0ull), (short)0, (int)span, 0x00020000);
#pragma unroll
        for (int k = 0; k < (int)kFrameRows; ++k) __builtin_amdgcn_raw_buffer_store_b128(v[k], dst, (int)(lane * 16u + k * 1024u), 0, 0);
    }
    uint32_t before = 0;  // the dword just before this block (row 0, lane 0 needs it)
    if (base != 0 && base <= nbytes) before = *reinterpret_cast<const uint32_t*>(bytes + base - 4);
    uint32_t count = 0;
    uint32_t prev_row_last = before;
    auto row = [&](int k, int32_t rem) {
        // previous dword: lane-1's last dword; lane 0: last dword of the previous row / block.  It is the neighbour's RAW dword, although
        // chunk_masks reads the bytes behind the stream's end as zeros: a chunk with bytes to zero has rem < 16, so the chunk behind
        // it -- the only one this dword reaches -- lies past nbytes and gets 0 whatever pw holds.
        uint32_t pw = __shfl_up(v[k][3], 1, kWave);
        const uint32_t row_last = __shfl(v[k][3], kWave - 1, kWave);
        if (lane == 0) pw = prev_row_last;
        prev_row_last = row_last;
        const uint32_t m = fuse::chunk_masks(v[k][0], v[k][1], v[k][2], v[k][3], pw, delim_pat, rem);
        store(k, m);
        count += (uint32_t)__builtin_popcount(m & 0xFFFFu);
    };
    // (wave-uniform) every chunk of the block lies inside the stream -- all blocks of a stream but its last one or two --: rem is the
    // constant 16 and chunk_masks' end-of-stream handling folds away.  With a per-lane rem in every block the 25 GB scan took
    // 6.77 ms instead of 6.24 (MI355X).
    if (left >= kFrameBlock) {
#pragma unroll
        for (int k = 0; k < (int)kFrameRows; ++k) row(k, 16);
    } else {
        // bytes of a chunk inside the stream: rem of them; position rem (one past the end of the stream) may carry the "sequence cut
        // off by the end" error bit; a chunk behind that position has nothing
#pragma unroll
        for (int k = 0; k < (int)kFrameRows; ++k) {
            const uint64_t cpos = base + (uint64_t)(k * kWave + lane) * 16u;
            row(k, cpos > nbytes ? -1 : nbytes - cpos >= 16u ? 16 : (int32_t)(nbytes - cpos));
        }
    }
    return count;
}

// ---- the emit body --------------------------------------------------------------------------------------------------------
// A lane owns 16 consecutive chunks (256 bytes) of its block: their mask words src[0 .. 16) -> w; returns the lane's delimiter count,
// *any_err = whether one of the words has an error bit
__device__ __forceinline__ uint32_t frame_lane_words(const uint32_t* src, uint32_t (&w)[16], uint32_t* any_err) {
    const uint4* src4 = reinterpret_cast<const uint4*>(src);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint4 m = src4[k];
        w[4 * k] = m.x; w[4 * k + 1] = m.y; w[4 * k + 2] = m.z; w[4 * k + 3] = m.w;
    }
    uint32_t mine = 0, err = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        mine += (uint32_t)__builtin_popcount(w[j] & 0xFFFFu);
        err |= w[j] >> 16;
    }
    *any_err = err;
    return mine;
}
// ... and from them offsets[rank + 1 ...] of the lane's delimiters and bad[frame] of its error positions, against cap.
// rank: delimiters before the lane's first byte, which is stream position lane_base
__device__ __forceinline__ void frame_emit_lane(const uint32_t (&w)[16], uint64_t rank, uint64_t lane_base, uint64_t* __restrict__ offsets,
                                                uint8_t* __restrict__ bad, uint64_t cap) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        uint32_t dm = w[j] & 0xFFFFu, em = w[j] >> 16;
        const uint64_t cpos = lane_base + (uint64_t)j * 16u;
        while (em) {  // rare
            const uint32_t b = (uint32_t)__builtin_ctz(em);
            em &= em - 1u;
            const uint64_t frame = rank + (uint32_t)__builtin_popcount(dm & ((1u << b) - 1u));
            if (frame < cap) bad[frame] = 1;
        }
        while (dm) {
            const uint32_t b = (uint32_t)__builtin_ctz(dm);
            dm &= dm - 1u;
            ++rank;
            if (rank <= cap) offsets[rank] = cpos + b + 1u;
        }
    }
}

// ---- the one-pass form ----------------------------------------------------------------------------------------------------
// desc[tile] = flag << 62 | value: flag 0 nothing yet, 1 the tile's own delimiter count (A), 2 the count of all tiles up to and
// including this one (P).  Zeroed once per stream (fg_launch_frame / the first slice).
constexpr uint64_t kDescA = 1ull << 62, kDescP = 2ull << 62, kDescVal = (1ull << 62) - 1ull;
// polls before a waiting tile gives up: a poll is an s_sleep(2) plus an agent-scope load that goes to L2, ~0.5-1 us, so 2^18 polls are
// a fifth of a second -- against a look-back that normally resolves within a few polls.  (2^22 were SECONDS per waiting tile)
constexpr uint32_t kSpinLimit = 1u << 18;
constexpr uint32_t kWholeStream = 1u, kSelfTestStall = 2u;  // bits of the kernel's `whole` argument
constexpr uint64_t kFrameAborted = ~0ull;  // what pref[blk1] holds when the chain gave up (the caller runs the classic kernels)

// A workgroup of kTileWaves = eight waves takes a 128 KiB tile (a wave = one 16 KiB block of it, as in the classic scan); ONE descriptor per tile:
// the chain moves at most 64 descriptors per look-back step (a trip to L2), so the tile must be large enough for that to outrun
// the memory system -- with one wave per 16 KiB descriptor the scan ran at 2.9 TB/s, bound by exactly that (profiles/r04x_*).
constexpr uint32_t kTileWaves = 8;
// What a launch knows about segment boundaries inside the stream: nothing (fg_frame.hip) ...
struct NoSegments {
    static constexpr bool kSegmented = false;
};
// ... or a type with kSegmented = true and
//   bool patch(const uint8_t* bytes, uint64_t nbytes, uint64_t base, uint32_t* m, uint32_t lane) const
// that rewrites the mask words m[0 .. kFrameBlock / 16) of the wave's block at `base` (LDS, atomics: lanes share words) for the
// boundaries that touch it and says, wave-uniformly, whether there was one (fg_frame_multi.hip).
// The body of the one-pass kernel; a workgroup of kWave * kTileWaves threads.
template <bool COPY, class SEG>
__device__ __forceinline__ void frame_onepass(const uint8_t* __restrict__ bytes, uint64_t nbytes, uint32_t delim_pat,
                                              uint64_t* __restrict__ desc, uint64_t* __restrict__ pref,
                                              uint32_t* __restrict__ abort_w, uint64_t* __restrict__ offsets,
                                              uint8_t* __restrict__ bad, uint64_t cap, uint64_t tile0, uint64_t blk1,
                                              uint64_t nblk, uint32_t whole, uint8_t* __restrict__ copy_to, const SEG seg) {
    __shared__ __attribute__((aligned(16))) uint32_t m_lds[kTileWaves][kFrameBlock / 16u];
    __shared__ uint32_t s_cnt[kTileWaves];
    __shared__ uint64_t s_prefix;
    __shared__ uint32_t s_abort;
    const uint32_t lane = threadIdx.x & (kWave - 1u), wv = threadIdx.x / kWave;
    const uint64_t tile = tile0 + blockIdx.x;
    const uint64_t blk = tile * kTileWaves + wv;  // this wave's 16 KiB block (may lie behind the stream: empty then)
    const uint64_t base = blk * kFrameBlock;
    uint32_t count = frame_scan_block<COPY>(bytes, nbytes, delim_pat, base, lane, copy_to, [&](int k, uint32_t m) { m_lds[wv][k * kWave + lane] = m; });
    if constexpr (SEG::kSegmented) {
        // segment boundaries that touch this block: its masks are patched where they lie, before anything is counted from them
        __syncthreads();
        const bool touched = seg.patch(bytes, nbytes, base, m_lds[wv], lane);
        __syncthreads();
        if (touched) {
            count = 0;
#pragma unroll
            for (int k = 0; k < (int)kFrameRows; ++k) count += (uint32_t)__builtin_popcount(m_lds[wv][k * kWave + lane] & 0xFFFFu);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) count += __shfl_xor(count, d, kWave);
    if (lane == 0) s_cnt[wv] = count;
    if (threadIdx.x == 0) s_abort = 0u;
    __syncthreads();
    uint32_t tile_count = 0, wave_off = 0;
#pragma unroll
    for (uint32_t k = 0; k < kTileWaves; ++k) {
        const uint32_t c = s_cnt[k];
        wave_off += k < wv ? c : 0u;
        tile_count += c;
    }
    // the tile's own count, for the tiles behind it (the first tile of the stream knows its prefix)
    // (self-test, FG_LO_FRAME_SELFTEST_STALL: the second tile of the launch never publishes anything -- every tile behind it must give up
    //  within the spin bound and the caller must fall back to the classic kernels)
    const bool stall = (whole & kSelfTestStall) != 0u && blockIdx.x == 1u;
    if (threadIdx.x == 0 && !stall) __hip_atomic_store(desc + tile, (tile == 0 ? kDescP : kDescA) | (uint64_t)tile_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    // a lane now owns 16 consecutive chunks (256 bytes) of its wave's block: rank of its first delimiter inside the tile
    uint32_t w[16], any_err;
    const uint32_t mine = frame_lane_words(m_lds[wv] + lane * 16u, w, &any_err);
    uint32_t tot;
    const uint32_t ex = wave_exclusive_sum(mine, &tot);
    // ---- look-back (the tile's first wave): the delimiters of all tiles before this one ----
    if (wv == 0) {
        uint64_t prefix = 0;
        bool aborted = false;
        if (tile != 0) {
            int64_t idx = (int64_t)tile - 1;
            uint32_t polls = 0;
            for (;;) {
                const int64_t j = idx - (int64_t)lane;  // lane i looks at tile idx - i; before the stream: a prefix of zero
                uint64_t d = kDescP;
                if (j >= 0) d = __hip_atomic_load(desc + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t fl = (uint32_t)(d >> 62);
                const uint64_t mp = __ballot(fl == 2u), mx = __ballot(fl == 0u);
                const uint32_t p = mp ? (uint32_t)__builtin_ctzll(mp) : 64u;  // the nearest tile that knows its prefix
                const uint64_t upto = p >= 63u ? ~0ull : ((2ull << p) - 1ull);
                if (mx & upto) {  // a tile between here and there has not even counted yet: wait for it
                    ++polls;
                    if (polls > kSpinLimit) {
                        if (lane == 0) __hip_atomic_store(abort_w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        aborted = true;
                    } else if ((polls & 15u) == 0u && __hip_atomic_load(abort_w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {
                        aborted = true;
                    }
                    if (aborted) break;
                    __builtin_amdgcn_s_sleep(2);
                    continue;
                }
                uint32_t a = lane < p ? (uint32_t)d : 0u;  // (a tile's own count fits 17 bits)
#pragma unroll
                for (int s2 = 32; s2 >= 1; s2 >>= 1) a += __shfl_xor(a, s2, kWave);
                prefix += a;
                if (mp) {
                    const uint32_t lo = __shfl((uint32_t)d, (int)p, kWave), hi = __shfl((uint32_t)(d >> 32), (int)p, kWave);
                    prefix += (((uint64_t)hi << 32) | lo) & kDescVal;
                    break;
                }
                idx -= kWave;
            }
            if (!aborted && !stall && lane == 0) __hip_atomic_store(desc + tile, kDescP | (prefix + tile_count), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) {
            s_prefix = prefix;
            s_abort = aborted ? 1u : 0u;
            const uint64_t incl = prefix + tile_count;
            // (the range's total through an atomic MAX over a word the launcher cleared: a tile that gave up leaves the sentinel -- the
            //  largest value -- whichever of the two stores lands last; tiles behind a tile that gave up still finish, on its count)
            if (aborted) {
                atomicMax(reinterpret_cast<unsigned long long*>(pref + blk1), (unsigned long long)kFrameAborted);
            } else {
                if (tile == (blk1 - 1u) / kTileWaves)  // the delimiters up to the end of this launch's range
                    atomicMax(reinterpret_cast<unsigned long long*>(pref + blk1), (unsigned long long)incl);
                if (tile == 0) offsets[0] = 0;
                if ((whole & kWholeStream) && tile == (nblk - 1u) / kTileWaves && incl + 1 <= cap) offsets[incl + 1] = nbytes;  // a final unterminated frame
            }
        }
    }
    __syncthreads();
    if (s_abort) return;
    if (mine == 0 && any_err == 0) return;
    frame_emit_lane(w, s_prefix + wave_off + ex, base + (uint64_t)lane * 256u, offsets, bad, cap);
}

}  // namespace fg

// blocks: one more than needed for the bytes when nbytes is a multiple of the block size, so
// that position `nbytes` itself (where a sequence cut off by the end of the stream is flagged) is
// always covered
static inline uint64_t frame_blocks(uint64_t nbytes) { return nbytes / fg::kFrameBlock + 1; }
// scratch of a launch over nblk blocks, and the only place that knows where its parts lie: the mask words (nblk * 1024 u32; the one-pass
// form keeps its tile descriptors there, nblk u64 of them cleared), counts = nblk u32, pref = (nblk + 1) u64, then the abort word.
struct FrameScratch {
    uint32_t* masks;
    uint64_t* desc;
    uint32_t* counts;
    uint64_t* pref;
    uint32_t* abort_w;
    static uint64_t pref_at(uint64_t nblk) { return nblk * 4096u + ((nblk * 4u + 255u) & ~255ull); }
    static uint64_t bytes(uint64_t nblk) { return pref_at(nblk) + (nblk + 1u) * 8u + 256u; }
    FrameScratch(uint8_t* scratch, uint64_t nblk)
        : masks(reinterpret_cast<uint32_t*>(scratch)), desc(reinterpret_cast<uint64_t*>(scratch)),
          counts(reinterpret_cast<uint32_t*>(scratch + nblk * 4096u)), pref(reinterpret_cast<uint64_t*>(scratch + pref_at(nblk))),
          abort_w(reinterpret_cast<uint32_t*>(scratch + pref_at(nblk) + (nblk + 1u) * 8u + 64u)) {}
};
// what a one-pass launch over the blocks [.., blk1) expects cleared: the word of the range's total -- and, in front of the stream's
// first launch, the descriptors of all its tiles and the abort word
static inline void frame_onepass_reset(const FrameScratch& sc, uint64_t nblk, uint64_t blk1, bool first, hipStream_t stream) {
    if (first) {
        (void)hipMemsetAsync(sc.desc, 0, nblk * 8u, stream);
        (void)hipMemsetAsync(sc.abort_w, 0, 4, stream);
    }
    (void)hipMemsetAsync(sc.pref + blk1, 0, 8, stream);
}

// fg_frame.hip's classic form in two halves, for the segmented framer, which edits the masks and the block counts between them
// (declared here, where fg_frame.hip's definitions are held against them; fg_ctx.hpp has the launchers the host side calls)
extern "C" int fg_launch_frame_classic_scan(const uint8_t* d_bytes, uint64_t nbytes, uint32_t delim, uint8_t* scratch, uint32_t** d_masks,
                                            uint32_t** d_counts, hipStream_t stream);
extern "C" int fg_launch_frame_classic_emit(uint64_t nbytes, uint8_t* scratch, uint64_t* d_offsets, uint8_t* d_bad, uint64_t cap,
                                            uint64_t** d_total_out, hipStream_t stream);
