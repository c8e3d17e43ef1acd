// fg_frame_kernels.hpp -- device code shared by the two framing units, fg_frame.hip (one stream per launch) and fg_frame_multi.hip
// (the chunks of many connections per launch), and by nothing else: the per-chunk UTF-8 rule, the mask layout (per 16-byte chunk one
// word: delimiter mask | error mask << 16) and the body of the one-pass chained scan.  Include after fg_pipeline.hpp.
#pragma once

namespace fg {

constexpr uint32_t kFrameBlock = 16384;  // bytes per wave-block
constexpr uint32_t kFrameRows = kFrameBlock / (16 * kWave);  // 16

// bit7 flags, per byte of a dword
__device__ __forceinline__ uint32_t f_cont(uint32_t b) { return b & ~(b << 1) & 0x80808080u; }          // 80..BF
__device__ __forceinline__ uint32_t f_ge_c0(uint32_t b) { return b & (b << 1) & 0x80808080u; }          // C0..FF
__device__ __forceinline__ uint32_t f_ge_e0(uint32_t b) { return b & (b << 1) & (b << 2) & 0x80808080u; }
__device__ __forceinline__ uint32_t f_ge_f0(uint32_t b) { return b & (b << 1) & (b << 2) & (b << 3) & 0x80808080u; }
__device__ __forceinline__ uint32_t f_eq_hi(uint32_t b, uint32_t pat) {  // byte == pat's byte (pat bytes >= 0x80)
    uint32_t y = b ^ pat;                                                // zero byte <=> equal
    return ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u;
}
// UTF-8 errors of the four bytes in `b`, given the previous dword `p` (bytes just before b):
// bit7 of byte i set <=> the sequence rules are violated AT byte i.
__device__ __forceinline__ uint32_t utf8_err_flags(uint32_t b, uint32_t p) {
    const uint32_t p1 = __builtin_amdgcn_alignbyte(b, p, 3);  // byte i-1 for every i
    const uint32_t p2 = __builtin_amdgcn_alignbyte(b, p, 2);
    const uint32_t p3 = __builtin_amdgcn_alignbyte(b, p, 1);
    // a continuation byte is due here: after a lead, or as the 3rd / 4th byte of a sequence whose
    // earlier bytes WERE continuations (a sequence broken earlier was flagged there and expects
    // nothing more -- so no expectation ever crosses an ASCII byte such as the frame terminator)
    const uint32_t c1 = f_cont(p1), c2 = f_cont(p2);
    const uint32_t must = f_ge_c0(p1) | (f_ge_e0(p2) & c1) | (f_ge_f0(p3) & c2 & c1);
    uint32_t err = (f_cont(b) ^ must);                                   // missing or stray continuation
    // bytes that never appear: C0, C1, F5..FF
    const uint32_t y = (b & 0xFEFEFEFEu) ^ 0xC0C0C0C0u;
    err |= ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u;
    err |= b & ((b & 0x7F7F7F7Fu) + 0x0B0B0B0Bu) & 0x80808080u;          // >= F5
    // second-byte ranges: E0 A0..BF | ED 80..9F | F0 90..BF | F4 80..8F
    const uint32_t b5 = b << 2, b4 = b << 3;                             // bit5 / bit4 of each byte moved to bit7
    err |= f_eq_hi(p1, 0xE0E0E0E0u) & ~b5;
    err |= f_eq_hi(p1, 0xEDEDEDEDu) & b5;
    err |= f_eq_hi(p1, 0xF0F0F0F0u) & ~b5 & ~b4;
    err |= f_eq_hi(p1, 0xF4F4F4F4u) & (b5 | b4);
    return err & 0x80808080u;
}

// the chunk that holds the stream's end: its bytes behind position nv are the caller's memory, readable (nbytes rounded up to 16) and
// nothing more -- read as zeros, so that the error bit AT position nv says "a sequence cut off by the end of the stream" and nothing else
__device__ __forceinline__ uint4 zero_behind(uint4 q, uint32_t nv) {
    if (nv < 16u) {
        // dword d holds chunk bytes 4d .. 4d + 3:  nv >= 4d + 4 -> all four kept;  nv <= 4d -> none;  else its low nv - 4d bytes (1 .. 3)
        auto keep = [&](uint32_t d) -> uint32_t { return nv >= 4u * d + 4u ? 0xFFFFFFFFu : nv <= 4u * d ? 0u : (1u << (8u * (nv - 4u * d))) - 1u; };
        q.x &= keep(0u), q.y &= keep(1u), q.z &= keep(2u), q.w &= keep(3u);
    }
    return q;
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
    const uint64_t left = base < nbytes ? nbytes - base : 0ull;  // (a block AT the end only carries the "cut off by the end" check)
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
#pragma unroll
    for (int k = 0; k < (int)kFrameRows; ++k) {
        const uint64_t cpos = base + (uint64_t)(k * kWave + lane) * 16u;
        const uint32_t nv = cpos >= nbytes ? 0u : (nbytes - cpos >= 16u ? 16u : (uint32_t)(nbytes - cpos));
        const uint4 q = zero_behind(make_uint4(v[k][0], v[k][1], v[k][2], v[k][3]), nv);
        const uint32_t dm = mask16_eq(q, delim_pat) & ((1u << nv) - 1u);
        uint32_t pw = __shfl_up(q.w, 1, kWave);
        const uint32_t row_last = __shfl(q.w, kWave - 1, kWave);
        if (lane == 0) pw = prev_row_last;
        prev_row_last = row_last;
        uint32_t em = 0;
        if (((q.x | q.y | q.z | q.w | pw) & 0x80808080u) != 0u) {
            em = gather16(utf8_err_flags(q.x, pw), utf8_err_flags(q.y, q.x), utf8_err_flags(q.z, q.y), utf8_err_flags(q.w, q.z));
            em &= nv >= 16u ? 0xFFFFu : ((2u << nv) - 1u);  // keep position nv itself (zero_behind: "not a continuation")
            if (cpos > nbytes) em = 0;
        }
        m_lds[wv][k * kWave + lane] = dm | (em << 16);
        count += (uint32_t)__builtin_popcount(dm);
    }
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
    uint32_t w[16];
    {
        const uint4* src = reinterpret_cast<const uint4*>(m_lds[wv] + lane * 16u);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint4 m = src[k];
            w[4 * k] = m.x; w[4 * k + 1] = m.y; w[4 * k + 2] = m.z; w[4 * k + 3] = m.w;
        }
    }
    uint32_t mine = 0, any_err = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        mine += (uint32_t)__builtin_popcount(w[j] & 0xFFFFu);
        any_err |= w[j] >> 16;
    }
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
    uint64_t rank = s_prefix + wave_off + ex;  // delimiters before this lane's first byte
    const uint64_t lane_base = base + (uint64_t)lane * 256u;
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

}  // namespace fg

// scratch of a launch: masks = ceil(nbytes / 16 KiB) * 1024 u32 (one-pass: the tile descriptors lie there), counts = nblk u32,
// pref = (nblk + 1) u64, then the abort word.
// blocks: one more than needed for the bytes when nbytes is a multiple of the block size, so
// that position `nbytes` itself (where a sequence cut off by the end of the stream is flagged) is
// always covered
static inline uint64_t frame_blocks(uint64_t nbytes) { return nbytes / fg::kFrameBlock + 1; }
static inline uint64_t* frame_pref(uint8_t* scratch, uint64_t nblk) {
    return reinterpret_cast<uint64_t*>(scratch + nblk * 4096u + ((nblk * 4u + 255u) & ~255ull));
}
static inline uint32_t* frame_abort_word(uint8_t* scratch, uint64_t nblk) {
    return reinterpret_cast<uint32_t*>(scratch + nblk * 4096u + ((nblk * 4u + 255u) & ~255ull) + (nblk + 1u) * 8u + 64u);
}
