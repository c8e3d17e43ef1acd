// fg_pipeline.hpp -- the HBM -> VGPR -> LDS streaming skeleton shared by the three decode kernels,
// plus the byte-class / bitmap / window primitives their lane-per-line tokenisers are built from.
//
// Execution model (gfx950, 64-lane waves, one wave per workgroup, PERSISTENT grid):
//   * a wave walks line groups g = blockIdx.x, +gridDim.x, ... ; a group = L consecutive lines
//     (L = 64 for ~256-byte lines, smaller powers of two for longer lines) = one contiguous byte
//     range of the packed buffer;
//   * stage A: the group's bytes arrive in NB x 16 B of VGPRs per lane (a register prefetch
//     window filled by bounds-checked buffer loads while the PREVIOUS group was being tokenised),
//     are classified while they sit in registers (one 16-bit mask per 16-byte chunk -> a bitmap
//     of the format's delimiter) and written to the wave's LDS tile;
//   * stage B: every lane tokenises ITS line out of LDS (format-specific, F::decode);
//   * the table row of a group is stored one iteration late (see the comment in the loop).
// HBM sees only coalesced 1 KiB-per-wave-instruction reads, each byte once.
#pragma once
#include "fg_device.hpp"
#include "fg_plan_policy.hpp"
#include "fg_sparse_need.hpp"
#include "fg_wave.hpp"

namespace fg {

using u32x4 = unsigned int __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------
// SWAR byte classes -> 16-bit masks
// ---------------------------------------------------------------------------------------------
// bit7 of each byte set <=> byte == pat's byte (pat bytes < 0x80); exact, no borrow artefacts
__device__ __forceinline__ uint32_t eq_flags(uint32_t x, uint32_t pat) {
    uint32_t s = ((x & 0x7F7F7F7Fu) ^ pat) + 0x7F7F7F7Fu;  // bit7 set <=> low 7 bits != pat
    return ~(s | x) & 0x80808080u;
}
// bit7 of each byte set <=> 33 <= byte <= 126
__device__ __forceinline__ uint32_t range_flags(uint32_t x) {
    uint32_t l = x & 0x7F7F7F7Fu;
    uint32_t ge33 = l + 0x5F5F5F5Fu;   // bit7 set <=> low7 >= 33
    uint32_t le126 = l + 0x01010101u;  // bit7 set <=> low7 == 127
    return ge33 & ~le126 & ~x & 0x80808080u;
}
// bit7 of each byte set <=> byte < 0x20 (control characters)
__device__ __forceinline__ uint32_t ctrl_flags(uint32_t x) {
    uint32_t ge32 = (x & 0x7F7F7F7Fu) + 0x60606060u;  // bit7 set <=> low7 >= 32
    return ~(ge32 | x) & 0x80808080u;
}
// four dwords of byte flags (0x80 per hit) -> 16-bit mask, v_dot4_u32_u8 as the bit gather
__device__ __forceinline__ uint32_t gather16(uint32_t f0, uint32_t f1, uint32_t f2, uint32_t f3) {
    uint32_t lo = __builtin_amdgcn_udot4(f1, 0x80402010u, __builtin_amdgcn_udot4(f0, 0x08040201u, 0u, false), false);
    uint32_t hi = __builtin_amdgcn_udot4(f3, 0x80402010u, __builtin_amdgcn_udot4(f2, 0x08040201u, 0u, false), false);
    return (lo >> 7) | (hi << 1);
}
__device__ __forceinline__ uint32_t mask16_eq(const uint4& v, uint32_t pat) {
    return gather16(eq_flags(v.x, pat), eq_flags(v.y, pat), eq_flags(v.z, pat), eq_flags(v.w, pat));
}

// ---------------------------------------------------------------------------------------------
// The wave's LDS tile: bytes (as dwords) + one bitmap (bit i <=> tile byte i is in the class)
// ---------------------------------------------------------------------------------------------
struct Tile {
    const uint32_t* w;
    const uint32_t* bm;
};
// 8 / 16 consecutive bytes starting at tile byte `a` (unaligned) as little-endian dwords
__device__ __forceinline__ void load8(const Tile& T, uint32_t a, uint32_t* lo, uint32_t* hi) {
    uint32_t d = a >> 2, s = a & 3u;
    uint32_t w0 = T.w[d], w1 = T.w[d + 1], w2 = T.w[d + 2];
    *lo = __builtin_amdgcn_alignbyte(w1, w0, s);
    *hi = __builtin_amdgcn_alignbyte(w2, w1, s);
}
__device__ __forceinline__ void load16(const Tile& T, uint32_t a, uint32_t w[4]) {
    const uint32_t d = a >> 2, s = a & 3u;
    uint32_t r0 = T.w[d], r1 = T.w[d + 1], r2 = T.w[d + 2], r3 = T.w[d + 3], r4 = T.w[d + 4];
    w[0] = __builtin_amdgcn_alignbyte(r1, r0, s);
    w[1] = __builtin_amdgcn_alignbyte(r2, r1, s);
    w[2] = __builtin_amdgcn_alignbyte(r3, r2, s);
    w[3] = __builtin_amdgcn_alignbyte(r4, r3, s);
}
// Byte reader over a line in the tile that keeps 16 bytes in registers: a short forward walk
// (a number, a timestamp) pays ONE LDS round trip instead of one per dword.  Same interface as
// LdsReader (byte(i), i = line-relative index).
struct WinReader {
    const Tile& T;
    uint32_t base;
    uint32_t w0 = 0x80000000u;  // line index of the window's first byte (initially: no index is within 16 of it)
    uint64_t lo = 0, hi = 0;
    __device__ __forceinline__ WinReader(const Tile& t, uint32_t b) : T(t), base(b) {}
    __device__ __forceinline__ uint32_t byte(uint32_t i) {
        uint32_t off = i - w0;
        if (off >= 16u) {
            uint32_t w[4];
            load16(T, base + i, w);
            lo = (uint64_t)w[0] | ((uint64_t)w[1] << 32);
            hi = (uint64_t)w[2] | ((uint64_t)w[3] << 32);
            w0 = i;
            off = 0;
        }
        const uint64_t v = off < 8u ? lo : hi;
        return (uint32_t)(v >> (8u * (off & 7u))) & 0xFFu;
    }
};

// first set bit of a tile bitmap at line index >= q (tile byte base+q), or len; 32 bytes per step
// (compact: for short fields -- names, keys, SD values)
__device__ __forceinline__ uint32_t find_bit(const uint32_t* bm, uint32_t base, uint32_t q, uint32_t len) {
    while (q < len) {
        uint32_t a = base + q;
        uint32_t w = bm[a >> 5] >> (a & 31u);
        if (w) {
            uint32_t r = q + (uint32_t)__builtin_ctz(w);
            return r < len ? r : len;
        }
        q += 32u - (a & 31u);
    }
    return len;
}
// The same for spans that may be long (an 8 KiB message, a JSON text field): the first word is
// handled alone (the usual hit), a long run without the class is then crossed 256 bytes per
// step, eight independent LDS reads per round trip.
__device__ __forceinline__ uint32_t find_bit_long(const uint32_t* bm, uint32_t base, uint32_t q, uint32_t len) {
    if (q >= len) return len;
    {
        const uint32_t a = base + q;
        const uint32_t w = bm[a >> 5] >> (a & 31u);
        if (w) {
            const uint32_t r = q + (uint32_t)__builtin_ctz(w);
            return r < len ? r : len;
        }
        q += 32u - (a & 31u);
    }
    while (q + 256u <= len) {  // base + q is a multiple of 32 from here on
        const uint32_t i = (base + q) >> 5;
        uint32_t w[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) w[k] = bm[i + k];
        if ((w[0] | w[1] | w[2] | w[3] | w[4] | w[5] | w[6] | w[7]) != 0u) {
            uint32_t r = len;
#pragma unroll
            for (int k = 7; k >= 0; --k)
                if (w[k]) r = q + 32u * k + (uint32_t)__builtin_ctz(w[k]);
            return r < len ? r : len;
        }
        q += 256u;
    }
    while (q < len) {
        const uint32_t w = bm[(base + q) >> 5];
        if (w) {
            const uint32_t r = q + (uint32_t)__builtin_ctz(w);
            return r < len ? r : len;
        }
        q += 32u;
    }
    return len;
}
// wave-cooperative: rebuild the bitmap of the staged tile for another byte class (M::mask16)
template <class M>
__device__ __forceinline__ void rebuild_bitmap(const uint8_t* smem, uint16_t* bm16, uint32_t nchunk) {
    const uint4* src = reinterpret_cast<const uint4*>(smem);
    for (uint32_t c = threadIdx.x; c < nchunk; c += kWave) bm16[c] = (uint16_t)M::mask16(src[c]);
}

// ---------------------------------------------------------------------------------------------
// Output row (the fixed 68 bytes of a line) and the per-wave entry stash
// ---------------------------------------------------------------------------------------------
struct RowOut {
    uint32_t meta;
    double ts;
    fg_span span[6];
    uint32_t first, count;
    bool skip = false;  // the format has written what it wants of this row itself (kernels that complete rows of an earlier kernel)
    bool handed = false;  // (SPARSE window) the head of this line was not enough, or would not have been: read by the loop, never stored
};
__device__ __forceinline__ void store_row(const DevTables& t, uint64_t li, const RowOut& o) {
    if (o.skip) return;
    gstore(t.meta, li, o.meta);
    gstore(t.ts, li, o.ts);
#pragma unroll
    for (int k = 0; k < 6; ++k) gstore(t.span[k], li, o.span[k]);
    gstore(t.ent_first, li, o.first);
    gstore(t.ent_count, li, o.count);
}
// Entries found while a line is parsed are parked in the wave's scratch (stash[k * 64 + lane],
// k < kStashEntries, two u64 per entry in the GELF/LTSV kernels, one in the RFC5424 kernel) and
// copied into the entry table once the wave has its slots -- instead of parsing every line twice.
constexpr uint32_t kStashEntries = 48;
constexpr uint32_t kStashWords = 2;  // u64 words per stashed entry (scratch is sized for this)

// Wave-aggregated allocation of entry slots out of the wave's reserved chunk (fg_wave.hpp wave_alloc): returns this lane's
// first slot, or sets *overflow.  ent_state = the wave's two persistent LDS words.
struct EntAlloc {
    uint32_t ex = 0;      // entries of the lanes before this one
    uint32_t total = 0;   // entries of the wave
    wv::Slots s{};        // where they go: [base0, base0 + cut) and [base1, ...) (wv::wave_alloc)
    bool overflow = false;  // THIS lane's entries did not get slots (the table is full)
};
__device__ __forceinline__ EntAlloc alloc_entries_ex(const DevTables& t, uint32_t n_ent, uint32_t* ent_state) {
    EntAlloc a;
    if (!__any(n_ent != 0u)) return a;  // wave-uniform; the common case of the no-SD corpus skips the scan
    a.ex = wv::excl_sum(n_ent, &a.total);
    // lines whose slice still fits what is left of the wave's chunk stay there, the others open the next chunk
    const uint32_t left = wv::wave_left(ent_state);
    const unsigned long long nofit = __ballot(n_ent != 0u && a.ex + n_ent > left);
    const uint32_t cut = nofit ? (uint32_t)__shfl((int)a.ex, (int)__builtin_ctzll(nofit), kWave) : a.total;
    a.s = wv::wave_alloc(t.ent_used, t.ent_cap, ent_state, a.total, cut, t.alloc_chunk);
    a.overflow = a.s.overflow && n_ent != 0u && a.ex >= a.s.cut;
    return a;
}
__device__ __forceinline__ uint32_t alloc_entries(const DevTables& t, uint32_t n_ent, bool* overflow, uint32_t* ent_state) {
    const EntAlloc a = alloc_entries_ex(t, n_ent, ent_state);
    *overflow = a.overflow;
    return (a.overflow || a.total == 0u) ? 0u : a.s.at(a.ex);
}

// ---------------------------------------------------------------------------------------------
// The persistent streaming loop.  F supplies
//     static constexpr uint32_t F::kClasses                                    stage-A class bitmaps kept in LDS (0..5)
//     static void F::classify_store(const uint4& q, uint16_t* bm16, uint32_t chunk, uint32_t stride, uint32_t term4)
//         (term4: the framing's terminator byte in all four bytes of a dword, wv::kNoTerm without framing,
//          wv::kPastSpan for a chunk of zeros behind the last staged byte)
//                                                                              16-bit class masks of a 16-byte chunk -> bm16[c * stride + chunk]
//     RowOut F::decode(const GroupCtx&)  (member, may use its own state; called by all 64 lanes, converged)
// ---------------------------------------------------------------------------------------------
struct GroupCtx {
    const uint8_t* bytes;   // packed buffer (global)
    const uint8_t* smem;    // tile bytes
    uint16_t* bm16;         // tile bitmap (stage A's class; a decoder may rebuild it)
    uint64_t o0, o1;        // this lane's line [o0, o1) in the packed buffer
    uint64_t a0;            // packed-buffer address of tile byte 0
    uint32_t span;          // tile bytes staged
    bool valid;             // this lane owns a line
    uint64_t li;            // its index in the batch
    uint64_t* stash;        // the wave's entry stash (or null)
    uint32_t ablate;        // measurement build only
    uint32_t* ent_state;    // the wave's entry-slot reservation (two LDS words that persist across groups, wv::wave_alloc)
    unsigned long long* phase;  // measurement build only: ten format-specific phase clocks (lane 0 adds), else null
    // HEAD staging (persistent_loop<..., HEAD = true>; else unused): the tile holds only the first bytes of every line
    uint32_t tbase = 0;     // tile byte of this lane's line
    uint32_t tlen = 0;      // bytes of the line that are in the tile, from its first byte (== its length when it is there whole)
    uint32_t last2 = 0;     // the line's last byte | the byte before it << 8 (the trims look there; 0 where the line has none)
    uint32_t tile_cap = 0;  // LDS tile bytes of this launch (the bitmaps and a format's extra block lie behind it)
};

// The entries a wave parked in its stash -> the entry table THROUGH THE TILE: once every lane has parsed its line the tile's
// bytes are dead, so the records are laid out there in slot order and leave with one entry per lane and store instruction --
// consecutive lanes, consecutive addresses (lane-per-line stores are `n_ent` entries apart: every store instruction touched
// every cache line of the wave's range, and the 1-byte columns were read-modify-written at HBM: 2.2x the algorithmic bytes).
// WORDS = u64 words per stashed record (k-major: stash[(k * WORDS + w) * 64 + lane]); un(w0, w1, &name, &val, &type_flags).
// mine = this lane's entries are in the stash.  false = not done (the caller stores lane by lane): some lane's entries are
// not in the stash, the table overflowed, or the wave has more entries than fit the tile.
template <uint32_t WORDS, class Unpack>
__device__ __forceinline__ bool stash_to_table(const GroupCtx& c, const DevTables& t, const EntAlloc& a, uint32_t n_ent, bool mine,
                                               Unpack un) {
    const uint32_t lane = threadIdx.x;
    const uint32_t cap = (c.span / 18u) & ~3u;  // 8 + 8 + 2 bytes per entry
    if (a.total == 0u || a.total > cap || a.s.overflow || c.stash == nullptr || __any(n_ent != 0u && !mine)) return false;  // wave-uniform
    uint64_t* s_name = reinterpret_cast<uint64_t*>(const_cast<uint8_t*>(c.smem));
    uint64_t* s_val = s_name + cap;
    uint16_t* s_tf = reinterpret_cast<uint16_t*>(s_val + cap);
    __syncthreads();  // every lane is done with the tile's bytes
    for (uint32_t k0 = 0; k0 < n_ent; k0 += 4u) {  // (four records in flight per lane)
        uint64_t w0[4], w1[4];
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t k = k0 + j < n_ent ? k0 + j : n_ent - 1u;
            w0[j] = c.stash[(k * WORDS) * kWave + lane];
            w1[j] = WORDS > 1u ? c.stash[(k * WORDS + 1u) * kWave + lane] : 0ull;
        }
#pragma unroll
        for (uint32_t j = 0; j < 4u; ++j) {
            if (k0 + j < n_ent) {
                uint64_t name, val;
                uint32_t tf;
                un(w0[j], w1[j], &name, &val, &tf);
                const uint32_t idx = a.ex + k0 + j;
                s_name[idx] = name;
                s_val[idx] = val;
                s_tf[idx] = (uint16_t)tf;
            }
        }
    }
    __syncthreads();
    for (uint32_t idx = lane; idx < a.total; idx += kWave) {
        const uint32_t slot = a.s.at(idx);
        const uint64_t name = s_name[idx];
        const uint32_t tf = s_tf[idx];
        t.ent_name[slot] = fg_span{(uint32_t)name, (uint32_t)(name >> 32)};
        t.ent_val[slot] = s_val[idx];
        t.ent_type[slot] = (uint8_t)(tf & 0xFFu);
        t.ent_flags[slot] = (uint8_t)(tf >> 8);
    }
    return true;
}


// Framing of the frames handed to the decoders (fg_decode_frames_device): what to strip from the
// end of [offsets[i], offsets[i+1]) before decoding, and which frames to reject as invalid UTF-8.
struct FrameArgs {
    uint32_t strip;           // FG_FRAME_NONE / _LINE ("\n", then one "\r") / _NUL ("\0")
    const uint8_t* line_bad;  // [n] 1 = not valid UTF-8 (or null)
    // Dynamic chunk dispatch (round 5): the launch's ticket counter (one word of a ctx-owned ring) and the value it holds when the
    // launch starts; null = chunks are dealt out round-robin (the form of rounds 3-4, kept for A/B: FG_LO_STATIC_CHUNKS).
    uint32_t* ticket = nullptr;
    uint32_t ticket_base = 0;
    // ... and the chunk indices from which the chunks of a ticket launch shrink (fg_plan_policy.hpp: the taper)
    uint32_t taper0 = kNoTaper, taper1 = kNoTaper, taper2 = kNoTaper;
};
// (host side of the ticket: fg::TicketSlot, fg_tables_view.hpp)

// The input is read ONCE: its loads carry the non-temporal hint (aux bit 1 = nt on gfx950) so that the stream does not push the
// wave's stash, scratch and table lines out of the XCD's L2 between two uses.
#define FG_STREAM_AUX 2
__device__ __forceinline__ uint4 stream_load(const uint4* p) {
    typedef uint32_t nt4 __attribute__((ext_vector_type(4)));
    const nt4 v = __builtin_nontemporal_load(reinterpret_cast<const nt4*>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}

// rows of 1 KiB the tail of stage A loads before it stores the first (a format overrides it with  static constexpr int kTailBatch)
template <class F, class = void>
struct tail_batch { static constexpr int value = 4; };
template <class F>
struct tail_batch<F, decltype((void)F::kTailBatch)> { static constexpr int value = F::kTailBatch; };

// The table row of a group is normally stored one iteration late (see below); a format says  static constexpr bool kDeferRowStore =
// false  when that only keeps 17 registers alive across stage A (and, at the register limit, in scratch memory)
template <class F, class = void>
struct defer_row_store { static constexpr bool value = true; };
template <class F>
struct defer_row_store<F, decltype((void)F::kDeferRowStore)> { static constexpr bool value = F::kDeferRowStore; };

// HEAD = true: LONG lines.  Per-line parse work does not grow with the message, and the lines a CU can have in flight are what its LDS
// holds (these kernels run at lines-in-flight / per-line latency: tools/sweep.py, throughput linear in the waves per CU) -- so a
// format that never looks inside the message (RFC5424: header, structured data, the trims) stages only the HEAD of every line,
// its first kHeadCap bytes, one 1 KiB row per line (coalesced, bounds-checked by a buffer descriptor per row): three to four times
// the lines per tile on the 64 B .. 8 KiB corpus.  The decoder gets the line's last two bytes beside it (the trims) and takes the
// rare line whose structured data runs past its head from global memory.
constexpr uint32_t kHeadCap = 1024;  // bytes of a line staged in HEAD mode, alignment slack included (a multiple of 16)
// (a format whose head holds less says so -- F::kHeadBytes, a multiple of 16 below kHeadCap: more lines per tile at the same occupancy)
template <class F, class = void>
struct head_cap { static constexpr uint32_t value = kHeadCap; };
template <class F>
struct head_cap<F, decltype((void)F::kHeadBytes)> { static constexpr uint32_t value = F::kHeadBytes; };

// SPARSE = H > 0: SHORT lines whose decoder looks at the head and the last byte only (RFC5424 without structured data: two thirds of
// what the whole-line window reads is message text).  The window and the tile stay exactly as they are -- NB coalesced loads, lines
// at their natural tile offsets -- but a lane whose 16-byte chunk overlaps neither the first H bytes nor the last bytes of a line
// of the group (fg_sparse_need.hpp) gets an offset beyond the descriptor's range: it fetches nothing and stages zeros.  HBM moves
// 128-byte pieces, so what is saved are the pieces that lie wholly inside a message.  The decoder gets HEAD-style
// context (tbase, tlen = min(len, H), the last byte) and hands back every line whose result could depend on a byte it did not see;
// a wave whose group handed back more than kSparseHandful lines stages dense (all chunks, tlen = len) from the group after the
// one already in flight on, until a dense group holds no line that would have been handed back.
constexpr uint32_t kSparseHandful = 4;

template <int NB, bool PROF, class F, bool HEAD = false, uint32_t SPARSE = 0>
__device__ __forceinline__ void persistent_loop(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets,
                                                uint64_t n, const DevTables& t, uint32_t tile_cap, uint32_t L, uint64_t chunk_lines,
                                                unsigned long long* prof, uint64_t* stash_base, F& fmt, FrameArgs fr) {
    static_assert(!HEAD || F::kClasses <= 1, "HEAD staging classifies one stage-A byte class at most");
    static_assert(SPARSE == 0 || (!HEAD && F::kClasses == 0), "the sparse window builds its need bitmap where a stage-A class bitmap would lie");
    static_assert(SPARSE % 16u == 0 && SPARSE <= 112u, "a line's run of chunks (at most (H + 4 + 14) / 16 + 1) must fit two bitmap words at any shift");
    const uint64_t kChunkLines = chunk_lines;  // lines a wave takes at a time (LaunchPlan::chunk)
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint16_t* bm16 = reinterpret_cast<uint16_t*>(smem + tile_cap + 64u);
    const uint32_t bm_stride = tile_cap / 16u + 16u;  // u16 entries per class bitmap (F::kClasses of them, back to back)
    uint4* dst = reinterpret_cast<uint4*>(smem);
    const uint32_t lane = threadIdx.x;
    const uint64_t G = gridDim.x;
    uint64_t* stash = stash_base ? stash_base + (uint64_t)blockIdx.x * (kStashEntries * kStashWords * kWave) : nullptr;

    // A wave owns a CONTIGUOUS range of lines [p, hi) and cuts it into groups BY BYTES: a group = as many consecutive lines as
    // fit the tile, at most L of them (one per lane).  (Round 2 cut groups by line count, L lines of AVERAGE length per tile: on
    // the long-tail corpora -- 64 B .. 8 KiB -- a third of the groups overflowed the tile and were finished in further passes over
    // a synchronously restaged tile, which is where those workloads spent their time.)  Short lines give groups of L lines as
    // before; only a single line longer than the whole tile is still parsed from global memory.
    // The ranges are CHUNKS of kChunkLines lines dealt out round-robin (wave b takes chunks b, b + G, ...): the grid as a whole
    // still sweeps the buffer front to back.  (One big range per wave -- 1792 streams spread over 25 GB -- cost the headline
    // configuration 10 %: DRAM pages and TLB entries want neighbours in time to be neighbours in memory.)  The last group of a
    // chunk may be short: 256 lines = 4 full groups of 64 short lines, a dozen or more groups of long ones (small batches get
    // smaller chunks, so that every wave of the grid has one).
    // Round 5: only a wave's FIRST chunk is its block index; every further one is DRAWN from the launch's ticket counter (one atomic
    // per chunk, by lane 0, requested when the chunk BEFORE it is entered, so that a whole chunk hides its round trip).
    // Tickets are handed out in order, so the sweep stays front to back -- and a wave that meets a slow line (a walk through global
    // memory), a slow XCD or a chunk of long lines simply draws fewer tickets instead of keeping the whole grid waiting at the end:
    // what a batch of 10^5 .. 10^6 lines, one or two chunks per wave, needs.  Every wave draws until its first
    // ticket beyond the last chunk, so a launch advances the counter by EXACTLY the number of chunks: the host keeps the count and
    // hands the next launch of the slot its base -- no reset, no memset between launches.
    const bool dyn = fr.ticket != nullptr;  // wave-uniform
    uint32_t tk_raw = 0;      // the ticket drawn ahead (lane 0's return value; read when the chunk in hand runs out)
    bool tk_pending = false;  // wave-uniform
    auto draw_ticket = [&]() {
        if (lane == 0u) tk_raw = __hip_atomic_fetch_add(fr.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tk_pending = true;
    };
    uint64_t chunk = blockIdx.x;
    uint64_t p, hi_line;
    chunk_range(chunk, kChunkLines, fr.taper0, fr.taper1, fr.taper2, n, &p, &hi_line);
    if (dyn && p < n) draw_ticket();

    // the L offsets from line q on (clamped to the wave's range), as o0 = start / o1 = end of lane's line
    auto load_offsets = [&](uint64_t q, uint64_t* o0, uint64_t* o1) {
        const uint64_t li = q + lane;
        const bool in = lane < L && li < hi_line;
        *o0 = offsets[in ? li : hi_line];
        *o1 = offsets[in ? li + 1 : hi_line];
    };
    // group geometry from the lanes' offsets, as SCALARS: lines in the group, tile start (16-byte aligned), staged span
    auto geometry = [&](uint64_t q, uint64_t o0, uint64_t o1, uint32_t* nl, uint64_t* a0, uint32_t* span) {
        const uint64_t left = hi_line - q;
        const uint32_t avail = left < (uint64_t)L ? (uint32_t)left : L;  // >= 1
        // (the builtins return int: widen through uint32_t or bit 31 sign-extends into the high word)
        const uint32_t lo_l = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)o0);
        const uint32_t lo_h = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(o0 >> 32));
        const uint64_t lo = (uint64_t)lo_l | ((uint64_t)lo_h << 32);
        *a0 = lo & ~15ull;
        // leading lanes whose line ends inside the tile; the first line always goes (alone, from global memory, when too long)
        const unsigned long long fit = __ballot(lane < avail && (o1 - *a0) <= (uint64_t)tile_cap);
        uint32_t cnt = fit == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~fit);  // leading ones
        if (cnt == 0u) cnt = 1u;
        *nl = cnt;
        const uint32_t last = cnt - 1u;
        const uint32_t hi_l = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)o1, (int)last);
        const uint32_t hi_h = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(o1 >> 32), (int)last);
        const uint64_t hi = (uint64_t)hi_l | ((uint64_t)hi_h << 32);
        const uint64_t want = hi - *a0;
        *span = want > tile_cap ? tile_cap : (uint32_t)((want + 15ull) & ~15ull);
    };
    // the register window: NB buffer loads of 16 B per lane; the buffer descriptor bounds the
    // tile, so rows past `span` fetch nothing and return zeros -- no per-row predication.  The
    // row offset goes into the VGPR/immediate offset (the part the hardware range-checks; the
    // scalar offset is not checked).
    auto load_window = [&](uint64_t a0, uint32_t span, u32x4* v) {
        __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(bytes + a0), (short)0, (int)span, 0x00020000);
#pragma unroll
        for (int k = 0; k < NB; ++k) v[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(lane * 16u + k * 1024u), 0, FG_STREAM_AUX);
    };
    // ---- SPARSE mode ----
    // The voffsets of the window's loads for a group (a0, span, nl lines, the lanes' lines [lo0, lo1)).  A bitmap with one bit per chunk
    // of the window, SET = not fetched, lives in LDS -- in the bitmap block behind the tile, which stage B of the group BEFORE is done
    // with and stage B of this one has not touched yet: all ones, then every lane clears the run of its line (at most eight chunks, two
    // consecutive words: two ds_and) and the last line's lane the run of its end; a dense group clears the chunks of the span instead.
    // Each lane reads its bit of every row back and puts it into bit 31 of the load's voffset -- lane * 16 alone otherwise: the row's
    // KiB goes into the scalar offset, which the descriptor's range check does not see (every fetched chunk lies inside the span by
    // construction).  No global access, no branch around a load: the NB loads stay unconditional, so stage A's progressive vmcnt(k)
    // waits stay exact.  The wave runs at its instruction issue rate, so this is written to be few instructions: 32-bit tile offsets,
    // two VALU instructions per row.
    const uint32_t sparse_tail = fr.strip != FG_FRAME_NONE ? kSparseTailFramed : kSparseTailPlain;  // wave-uniform
    auto sparse_offsets = [&](uint64_t a0_, uint32_t span_, uint32_t nl_, uint64_t lo0, uint64_t lo1, bool dense, uint32_t* vo) {
        uint32_t* skip = reinterpret_cast<uint32_t*>(bm16);
        const uint32_t nchunk_ = span_ >> 4;
        const uint32_t nwin = nchunk_ < (uint32_t)NB * kWave ? nchunk_ : (uint32_t)NB * kWave;  // chunks the window can hold
        const uint32_t nword = 2u * NB + 2u < tile_cap / 32u + 8u ? 2u * NB + 2u : tile_cap / 32u + 8u;  // (the block's words)
        if (lane < nword) {
            const uint32_t c = lane * 32u;  // the word's first chunk
            skip[lane] = !dense || c >= nchunk_ ? ~0u : nchunk_ - c >= 32u ? 0u : ~0u << (nchunk_ - c);
        }
        __syncthreads();
        if (!dense) {  // wave-uniform
            auto mark = [&](const NeedRange& r, bool on) {
                const bool go = on && r.n != 0u && r.c0 < nwin;  // (a run that starts in the window ends at most a word behind it)
                const uint64_t m = go ? ((1ull << r.n) - 1ull) << (r.c0 & 31u) : 0ull;
                const uint32_t w = go ? r.c0 >> 5 : 0u;
                __hip_atomic_fetch_and(skip + w, ~(uint32_t)m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                __hip_atomic_fetch_and(skip + w + 1u, ~(uint32_t)(m >> 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            };
            const uint32_t t0 = (uint32_t)lo0 - (uint32_t)a0_, t1 = (uint32_t)lo1 - (uint32_t)a0_;  // (tile offsets: the low words do)
            mark(need_head(t0, t1 - t0, SPARSE, sparse_tail, lane == 0u), lane < nl_);
            if (lane + 1u == nl_) mark(need_tail(t1, sparse_tail), true);
            __syncthreads();
        }
        const uint32_t half = lane >> 5, bit = lane & 31u, off = lane * 16u;
#pragma unroll
        for (int k = 0; k < NB; ++k) vo[k] = ((skip[2 * k + (int)half] >> bit) << 31) | off;
    };
    auto load_window_sparse = [&](uint64_t a0_, uint32_t span_, const uint32_t* vo, u32x4* v) {
        __amdgpu_buffer_rsrc_t rsrc =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(bytes + a0_), (short)0, (int)span_, 0x00020000);
#pragma unroll
        for (int k = 0; k < NB; ++k) v[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)vo[k], k * 1024, FG_STREAM_AUX);
    };
    // ---- HEAD mode ----
    // per lane: st = bytes of its line's row in the tile (alignment slack + head, a multiple of 16, <= kHeadCap), tb = the row's tile
    // offset (exclusive prefix sum); a group = the leading lines whose rows fit the tile
    auto geometry_head = [&](uint64_t q, uint64_t o0, uint64_t o1, uint32_t* nl, uint32_t* span, uint32_t* st_out, uint32_t* tb_out) {
        const uint64_t left = hi_line - q;
        const uint32_t avail = left < (uint64_t)L ? (uint32_t)left : L;  // >= 1
        const uint64_t want = (o1 - o0) + (o0 & 15ull);
        uint32_t st = want >= head_cap<F>::value ? head_cap<F>::value : (uint32_t)((want + 15ull) & ~15ull);
        if (lane >= avail) st = 0u;
        uint32_t total;
        const uint32_t tb = wv::excl_sum(st, &total);
        const unsigned long long fit = __ballot(lane < avail && tb + st <= tile_cap);
        uint32_t cnt = fit == ~0ull ? 64u : (uint32_t)__builtin_ctzll(~fit);
        if (cnt == 0u) cnt = 1u;  // (cannot happen: a row is at most kHeadCap <= tile_cap)
        *nl = cnt;
        const uint32_t last = cnt - 1u;
        *span = (uint32_t)__builtin_amdgcn_readlane((int)tb, (int)last) + (uint32_t)__builtin_amdgcn_readlane((int)st, (int)last);
        *st_out = lane < cnt ? st : 0u;
        *tb_out = tb;
    };
    // row k of the window = the head of line k (a buffer descriptor per row: base = the line's first 16-byte boundary, range = its
    // row's bytes; lanes beyond fetch nothing)
    auto load_window_head = [&](uint64_t o0, uint32_t st, u32x4* v) {
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)o0, k);
            const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(o0 >> 32), k);
            const uint32_t sk = (uint32_t)__builtin_amdgcn_readlane((int)st, k);
            const uint64_t b = ((uint64_t)lo | ((uint64_t)hi << 32)) & ~15ull;
            __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(bytes + b), (short)0, (int)sk, 0x00020000);
            v[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(lane * 16u), 0, FG_STREAM_AUX);
        }
    };
    // the line's last two bytes (the trims and the terminator strip look there)
    auto load_last2 = [&](uint64_t o0, uint64_t o1) -> uint32_t {
        const uint64_t len = o1 - o0;
        uint32_t r = 0;
        if (len >= 1u) r = bytes[o1 - 1u];
        if (len >= 2u) r |= (uint32_t)bytes[o1 - 2u] << 8;
        return r;
    };

    // (the last 8 bytes of the 64-byte pad behind the tile: no tile read reaches them)
    uint32_t* ent_state = reinterpret_cast<uint32_t*>(smem + tile_cap + 56u);
    if (lane < 2u) ent_state[lane] = 0u;
    if (p >= hi_line) return;
    uint64_t o0, o1, a0 = 0;
    uint32_t span, nl, st = 0, tb = 0, last2 = 0;
    load_offsets(p, &o0, &o1);
    u32x4 v[NB];
    if constexpr (HEAD) {
        geometry_head(p, o0, o1, &nl, &span, &st, &tb);
        load_window_head(o0, st, v);
        last2 = load_last2(o0, o1);
    } else if constexpr (SPARSE != 0) {
        geometry(p, o0, o1, &nl, &a0, &span);
        uint32_t vo[NB];
        sparse_offsets(a0, span, nl, o0, o1, false, vo);
        load_window_sparse(a0, span, vo, v);
    } else {
        geometry(p, o0, o1, &nl, &a0, &span);
        load_window(a0, span, v);
    }
    // (SPARSE) dense = the group in hand was staged whole; dense_next = so is the one in flight; dense_then = so will be the one after
    bool dense = false, dense_next = false, dense_then = false;  // wave-uniform
    // The table row of a group is normally stored one iteration LATE (after the next group's stage A,
    // before the prefetch after that is issued): vmcnt retires in order, so stores issued
    // behind the window loads would have to be waited for at the top of every iteration.
    RowOut pend{};
    uint64_t pend_li = 0;
    bool pend_valid = false;
    uint64_t acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0, iters = 0, tm0 = 0, tm1 = 0, tm2 = 0, tm3 = 0;
    // measurement build only: prof[5] = ablation flags (1 = no table stores, 2 = no stage B,
    // 4 / 8 = format-specific, see the decoders)
    const uint32_t ablate = PROF ? (uint32_t)prof[5] : 0u;
    // the frame terminator the tile's bytes carry BETWEEN lines (never inside one), for formats whose classes care
    const uint32_t term4 = fr.strip == FG_FRAME_LINE ? 0x0A0A0A0Au : fr.strip == FG_FRAME_NUL ? 0u : wv::kNoTerm;

    for (;;) {
        // the next group starts where this one ends: its offsets are requested NOW (they ride behind the window loads and are
        // needed only after stage A, when the next window is issued)
        uint64_t pn = p + nl;
        if (pn >= hi_line) {  // this chunk is done: on to the wave's next one
            if (dyn) {
                if (!tk_pending) draw_ticket();  // (a chunk of one group: drawn and waited for here)
                const uint32_t tk = (uint32_t)__builtin_amdgcn_readfirstlane((int)tk_raw);
                chunk = (uint64_t)(uint32_t)(tk - fr.ticket_base) + G;  // (beyond the last chunk: pn >= n, the wave is done)
                tk_pending = false;
                // the successor's ticket right away: a whole chunk hides its trip.  (Drawn one group before the end, as the first cut
                // did, the tickets of a batch's FIRST round -- every wave starts at the same moment -- arrived in a burst of 1792 on one
                // word and were waited for: 1 M lines 122 us with tickets, 104 without, profiles/r05c_small_ab.log.)
                chunk_range(chunk, kChunkLines, fr.taper0, fr.taper1, fr.taper2, n, &pn, &hi_line);
                if (pn < n) draw_ticket();
            } else {
                chunk += G;
                chunk_range(chunk, kChunkLines, kNoTaper, kNoTaper, kNoTaper, n, &pn, &hi_line);
            }
        }
        const bool more = pn < n;  // wave-uniform
        uint64_t no0 = 0, no1 = 0;
        if (more) load_offsets(pn, &no0, &no1);
        if (PROF) {
            tm0 = __builtin_amdgcn_s_memtime();
            __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): the window has landed
            tm1 = __builtin_amdgcn_s_memtime();
        }
        // ---- stage A for this group: registers -> LDS, classify on the way ----------------------
        FG_MARK(A);
        const uint32_t nchunk = span >> 4;
        const uint32_t nrow = HEAD ? nl : (nchunk + kWave - 1u) / kWave;  // wave-uniform
        if constexpr (HEAD) {
            // row k = the head of line k: its chunks go to the row's place in the tile
#pragma unroll
            for (int k = 0; k < NB; ++k) {
                if ((uint32_t)k < nl) {  // scalar branch
                    const uint32_t tk = (uint32_t)__builtin_amdgcn_readlane((int)tb, k), sk = (uint32_t)__builtin_amdgcn_readlane((int)st, k);
                    if (lane * 16u < sk) {
                        const uint4 q = make_uint4(v[k][0], v[k][1], v[k][2], v[k][3]);
                        dst[(tk >> 4) + lane] = q;
                        if constexpr (F::kClasses != 0) F::classify_store(q, bm16, (tk >> 4) + lane, bm_stride, term4);
                    }
                }
            }
            // lines beyond the window: HB rows in flight (four; a format whose window is small -- kTailBatch -- takes eight)
            constexpr uint32_t HB = tail_batch<F>::value >= 8 ? 8u : 4u;
            for (uint32_t r0 = NB; r0 < nl; r0 += HB) {
                uint4 w[HB];
                uint32_t tk[HB], sk[HB];
#pragma unroll
                for (uint32_t j = 0; j < HB; ++j) {
                    const uint32_t r = r0 + j < nl ? r0 + j : nl - 1u;
                    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)o0, (int)r);
                    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(o0 >> 32), (int)r);
                    tk[j] = (uint32_t)__builtin_amdgcn_readlane((int)tb, (int)r);
                    sk[j] = (uint32_t)__builtin_amdgcn_readlane((int)st, (int)r);
                    const uint64_t b = ((uint64_t)lo | ((uint64_t)hi << 32)) & ~15ull;
                    __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(bytes + b), (short)0, (int)sk[j], 0x00020000);
                    const u32x4 x = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(lane * 16u), 0, FG_STREAM_AUX);
                    w[j] = make_uint4(x[0], x[1], x[2], x[3]);
                }
#pragma unroll
                for (uint32_t j = 0; j < HB; ++j)
                    if (lane * 16u < sk[j]) {  // (a clamped duplicate row writes the same bytes again)
                        dst[(tk[j] >> 4) + lane] = w[j];
                        if constexpr (F::kClasses != 0) F::classify_store(w[j], bm16, (tk[j] >> 4) + lane, bm_stride, term4);
                    }
            }
        } else {
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            if ((uint32_t)k < nrow) {  // scalar branch; lanes past the span store zeros inside the tile
                uint32_t idx = k * kWave + lane;
                uint4 q = make_uint4(v[k][0], v[k][1], v[k][2], v[k][3]);
                dst[idx] = q;
                F::classify_store(q, bm16, idx, bm_stride, idx < nchunk ? term4 : wv::kPastSpan);
            }
        }
        }
        if (!HEAD && nrow > (uint32_t)NB) {  // bytes beyond the register window
            const uint4* __restrict__ src = reinterpret_cast<const uint4*>(bytes + a0);
            // Loads and stores are UNCONDITIONAL (lanes past the end move the last chunk once more: same bytes, same
            // address): with `if (idx < nchunk)` the compiler kept w[] in scratch memory and waited for each load
            // before issuing the next -- serialised HBM round trips instead of four loads in flight.
            const uint32_t last = nchunk - 1u;
            // (TB loads in flight per lane: a format whose tile is mostly staged HERE -- a 2 KiB window under an 18 KiB tile -- pays
            //  the load latency once per TB KiB, and stage B's registers are dead at this point)
            constexpr int TB = tail_batch<F>::value;
            for (uint32_t c0 = NB * kWave; c0 < nchunk; c0 += kWave * TB) {
                uint4 w[TB];  // (the window registers are dead here)
#pragma unroll
                for (int k = 0; k < TB; ++k) {
                    const uint32_t idx = c0 + k * kWave + lane;
                    w[k] = stream_load(src + (idx < last ? idx : last));
                }
#pragma unroll
                for (int k = 0; k < TB; ++k) {
                    if (k == 0 || c0 + k * kWave < nchunk) {  // (scalar: whole rows past the end are skipped)
                        const uint32_t idx = c0 + k * kWave + lane, ci = idx < last ? idx : last;
                        dst[ci] = w[k];
                        F::classify_store(w[k], bm16, ci, bm_stride, term4);
                    }
                }
            }
            // (sparse kernel: rows of w[] that a scalar branch skipped stay "in flight" as far as the compiler can count, and the first
            //  write to one of their registers on the hot path behind W1 became a full vmcnt wait -- for the whole next window.  Here the
            //  window has landed: waiting for the tail's own loads costs nothing.)
            if constexpr (SPARSE != 0) __builtin_amdgcn_s_waitcnt(0x0F70);
        }
        __builtin_amdgcn_sched_barrier(0);  // keep the old window dead before the new one is loaded
        FG_MARK(S);
        if (PROF) {
            __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0): LDS writes retired
            tm2 = __builtin_amdgcn_s_memtime();
        }
        // ---- the next group's geometry from its offsets, BEFORE the row goes out: the readfirstlane of the offsets is the one vmcnt
        // wait of this stretch, and in front of the stores it covers the two offset loads alone, requested a whole stage A ago (the
        // window has landed, the stores are not issued yet).  Behind the stores -- which sit under an exec-masked branch, so the
        // compiler cannot count them, and gfx950 has no store counter of its own -- the same wait was a vmcnt(0) for ten store
        // acknowledgements, every group, before the first window load went out.
        uint64_t pa0 = 0;
        uint32_t pspan = 0, pnl = 0, pst = 0, ptb = 0, plast2 = 0;
        if (more) {
            if constexpr (HEAD) geometry_head(pn, no0, no1, &pnl, &pspan, &pst, &ptb);
            else geometry(pn, no0, no1, &pnl, &pa0, &pspan);
        }
        uint32_t pvo[SPARSE != 0 ? NB : 1];
        if constexpr (SPARSE != 0) {
            dense_next = dense_then;
            if (more) sparse_offsets(pa0, pspan, pnl, no0, no1, dense_next, pvo);
        }
        FG_MARK(ST);
        if (pend_valid && !(ablate & 1u)) store_row(t, pend_li, pend);
        // ---- prefetch: the next group's bytes into the register window, back to back with the stores (stores first: stage A's
        // progressive vmcnt(k) waits count the loads behind them exactly) ----
        FG_MARK(W0);
        if (more) {
            if constexpr (HEAD) {
                load_window_head(no0, pst, v);
                plast2 = load_last2(no0, no1);
            } else if constexpr (SPARSE != 0) {
                load_window_sparse(pa0, pspan, pvo, v);
            } else {
                load_window(pa0, pspan, v);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        FG_MARK(W1);
        FG_MARK(B);
        if (PROF) tm3 = __builtin_amdgcn_s_memtime();
        __syncthreads();  // single-wave workgroup: orders the LDS writes before stage B's reads
        // ---- stage B for this group ---------------------------------------------------------
        if (!(ablate & 2u)) {
            const uint64_t li = p + lane;
            const bool valid = lane < nl;
            // terminator stripping (BufRead::lines / split(0) semantics, see fg_frame.hip)
            uint64_t e1 = o1;
            uint32_t l2 = last2;  // (HEAD) the last two bytes of the line AS DECODED, i.e. behind its terminator
            if (fr.strip != FG_FRAME_NONE) {  // (wave-uniform)
                // The line's last byte and the one before it (0 where it has none).  Whole lines are read where they lie, in the tile:
                // every line of a group is there by construction.  The one exception, a line longer than the tile, is a group of its own
                // (nl == 1, wave-uniform) and takes its two bytes from global memory in a branch that waits for them itself.  One
                // expression that picked between the tile and global memory per lane was a flat load, and a flat load left stage B with
                // a full vmcnt wait -- for the whole next window -- whatever the framing.
                uint32_t b1 = last2 & 0xFFu, b2 = (last2 >> 8) & 0xFFu;
                if constexpr (!HEAD) {
                    const uint64_t len = o1 - o0;
                    const bool over = nl == 1u && __builtin_amdgcn_readfirstlane((int)((o1 - a0) > (uint64_t)span)) != 0;
                    if (over) {
                        FG_RARE_BEGIN();
                        if (valid && len >= 1u) b1 = bytes[o1 - 1u];
                        if (valid && len >= 2u) b2 = bytes[o1 - 2u];
                        FG_RARE_END();  // (waits for the two bytes here, not where the paths meet again)
                    } else if (valid) {
                        const uint32_t q = (uint32_t)(o1 - a0);  // <= span
                        if (len >= 1u) b1 = smem[q - 1u];
                        if (len >= 2u) b2 = smem[q - 2u];
                    }
                }
                if (valid && e1 > o0) {
                    if (fr.strip == FG_FRAME_LINE) {
                        if (b1 == '\n') {
                            --e1;
                            if (e1 > o0 && b2 == '\r') --e1;
                        }
                    } else if (b1 == 0u) {
                        --e1;
                    }
                    if (HEAD && e1 != o1) {  // (rare in HEAD mode -- long lines come framed by offsets -- so: two plain loads)
                        l2 = 0u;
                        if (e1 - o0 >= 1u) l2 = bytes[e1 - 1];
                        if (e1 - o0 >= 2u) l2 |= (uint32_t)bytes[e1 - 2] << 8;
                    }
                }
            }
            // Every line of the group lies inside the tile by construction -- except a single line longer than the whole tile,
            // which is a group of its own and is parsed straight from global memory (the decoders look at o1 - a0 <= span).
            GroupCtx c{bytes, smem, bm16, o0, e1, a0, span, valid, li, (ablate & 8u) ? nullptr : stash, ablate, ent_state, PROF ? prof + 6 : nullptr};
            c.tile_cap = tile_cap;
            if constexpr (HEAD) {
                const uint32_t al = (uint32_t)(o0 & 15ull), len = (uint32_t)(e1 - o0);
                c.tbase = tb + al;
                c.tlen = st == 0u ? 0u : (st - al < len ? st - al : len);
                c.last2 = l2;
            }
            if constexpr (SPARSE != 0) {
                // the line lies at its natural place in the tile, its first tlen bytes and its last ones staged; the last two bytes of the
                // line AS DECODED (behind its terminator) are read there (the line longer than the tile: not looked at, see decode)
                const uint32_t len = (uint32_t)(e1 - o0);
                c.tbase = (uint32_t)(o0 - a0);
                c.tlen = dense || len < SPARSE ? len : SPARSE;
                c.last2 = 0u;
                if (valid && e1 > o0 && (o1 - a0) <= (uint64_t)span) {
                    const uint32_t q = (uint32_t)(e1 - a0);
                    c.last2 = smem[q - 1u];
                    if (len >= 2u) c.last2 |= (uint32_t)smem[q - 2u] << 8;
                }
            }
            pend = fmt.decode(c, t);
            if constexpr (SPARSE != 0) {
                const uint32_t nh = (uint32_t)__popcll(__ballot(valid && pend.handed));
                dense_then = dense ? nh != 0u : nh > kSparseHandful;
            }
            if (fr.line_bad && valid && fr.line_bad[li]) {  // "Invalid UTF-8 input": the frame never reaches decode()
                pend.meta = FG_ST_BAD_UTF8 | (0xFFu << 8) | (0xFFu << 16);
                pend.ts = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) pend.span[k] = fg_span{0, FG_NONE};
                pend.count = 0;
            }
            pend_li = li;
            pend_valid = valid;
            if (!defer_row_store<F>::value) {  // (a format whose stage A waits for its own loads anyway: nothing to hide behind)
                if (pend_valid && !(ablate & 1u)) store_row(t, pend_li, pend);
                pend_valid = false;
            }
        }
        if (PROF) {
            __builtin_amdgcn_sched_barrier(0);
            __builtin_amdgcn_s_waitcnt(0xC07F);
            uint64_t tm4 = __builtin_amdgcn_s_memtime();
            acc0 += tm1 - tm0;
            acc1 += tm2 - tm1;
            acc2 += tm3 - tm2;
            acc3 += tm4 - tm3;
            iters += 1;
        }
        FG_MARK(Z);
        if (!more) break;
        __syncthreads();  // stage B's LDS reads are done before the next tile overwrites them
        p = pn;
        nl = pnl;
        o0 = no0;
        o1 = no1;
        a0 = pa0;
        span = pspan;
        if constexpr (SPARSE != 0) dense = dense_next;
        if constexpr (HEAD) {
            st = pst;
            tb = ptb;
            last2 = plast2;
        }
    }
    if (pend_valid && !(ablate & 1u)) store_row(t, pend_li, pend);
    if (PROF && lane == 0) {
        atomicAdd(&prof[0], (unsigned long long)acc0);
        atomicAdd(&prof[1], (unsigned long long)acc1);
        atomicAdd(&prof[2], (unsigned long long)acc2);
        atomicAdd(&prof[3], (unsigned long long)acc3);
        atomicAdd(&prof[4], (unsigned long long)iters);
    }
}

}  // namespace fg

// ---------------------------------------------------------------------------------------------
// Host side: plan and launch, shared by the launchers.  The geometry itself -- lines per group, tile, LDS, which instantiation -- is
// arithmetic and lives in fg_plan_policy.hpp (launch_geometry, pick_variant); what needs the device is here.
// ---------------------------------------------------------------------------------------------
#include <cstdio>
#include <cstdlib>

#include "fg_cus.hpp"

namespace fg {
// The LTSV / GELF tokenisers are compute-bound (hundreds of instructions per line) and register
// hungry: they keep only a token window (the rest of a group is staged by the plain tail loop,
// ~2 us of exposed latency against a group time of tens of us) and get the registers instead.
constexpr int kComputeBoundWindow = 2;

// The launch's ticket counter into the kernel's arguments; the host's copy of the counter moves on by what the launch will draw
// (every wave draws until its first ticket beyond the last chunk: chunks - blocks good ones + blocks bad ones = chunks).
inline void take_tickets(FrameArgs* fr, TicketSlot* tk, const LaunchPlan& p) {
    if (!tk || !tk->d_word || !tk->h_val || p.chunks + p.blocks >= 0xFFFFFFFFull || p.blocks > p.chunks) return;  // (static round-robin)
    if (!p.tickets) return;  // (equal shares: nothing to draw)
    fr->ticket = tk->d_word;
    fr->ticket_base = *tk->h_val;
    fr->taper0 = p.taper[0], fr->taper1 = p.taper[1], fr->taper2 = p.taper[2];
    *tk->h_val += (uint32_t)p.chunks;
}

// The geometry of a launch (launch_geometry) and its grid: what the occupancy of `kernel` at that LDS allows on this device, capped by
// the estimate of the groups, the caller's stash and fg_launch_opts.waves_per_cu -- then how the batch is cut into chunks (plan_chunks).
template <class K>
inline int plan_launch(K kernel, uint64_t n, uint64_t avg_len, uint32_t extra_lds, uint32_t max_tile, uint32_t stash_blocks, LaunchPlan* p,
                       const fg_launch_opts& lo, const PlanFormat& pf = PlanFormat()) {
    static_cast<LaunchGeometry&>(*p) = launch_geometry(n, avg_len, extra_lds, max_tile, lo, pf);
    const int cus = device_cus();
    if (cus < 1) return -1;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kWave, p->lds) != hipSuccess || per_cu < 1) per_cu = 1;
    if (lo.waves_per_cu > 0 && per_cu > (int)lo.waves_per_cu) per_cu = (int)lo.waves_per_cu;
    uint64_t blocks = (uint64_t)per_cu * (uint64_t)cus;
    if (blocks > p->groups) blocks = p->groups;
    if (stash_blocks && blocks > stash_blocks) blocks = stash_blocks;
    const ChunkPlan cp = plan_chunks(n, blocks, p->L, p->g, p->full, pf.ticket_from, lo, pf.taper);
    p->chunk = cp.chunk;
    p->chunks = cp.chunks;
    p->tickets = cp.tickets;
    for (int j = 0; j < 3; ++j) p->taper[j] = cp.taper[j];
    p->blocks = cp.blocks;
    return 0;
}

// The measurement build (-DFG_PROF_BUILD, `FG_BUILD_PROF=1 python -m flowgger_amd.build` -> libfg_hip_prof.so) also compiles the
// PROF = true instantiation of each kernel; FG_PROF=1 in the environment then runs it synchronously and prints the per-phase split
// (FG_ABLATE: ablation flags).  The product library has neither the instantiations nor any read of the environment.
#if defined(FG_PROF_BUILD)
inline bool prof_requested() { return getenv("FG_PROF") != nullptr; }
#define FG_PROF_TWIN(...) (__VA_ARGS__)
#else
constexpr bool prof_requested() { return false; }
#define FG_PROF_TWIN(...) nullptr
#endif
struct ProfRun {
    unsigned long long* d = nullptr;
    unsigned long long h[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};  // [6..15]: format-specific phase clocks (GroupCtx::phase)
    bool begin(hipStream_t stream) {
#if defined(FG_PROF_BUILD)
        if (const char* e = getenv("FG_ABLATE")) h[5] = (unsigned long long)atoi(e);
#endif
        if (hipMalloc((void**)&d, sizeof(h)) != hipSuccess) return false;
        (void)hipMemcpyAsync(d, h, sizeof(h), hipMemcpyHostToDevice, stream);
        return true;
    }
    void end(hipStream_t stream, const char* name, const LaunchPlan& p) {
        (void)hipStreamSynchronize(stream);
        (void)hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
        (void)hipFree(d);
        const double it = h[4] ? (double)h[4] : 1.0;
        fprintf(stderr,
                "[fg prof] %s: grid %u x64, L %u, tile %u, iters/wave %.1f | cycles per iteration: wait %.0f, stageA %.0f, "
                "stores+prefetch-issue %.0f, stageB %.0f\n",
                name, p.blocks, p.L, p.tile, it / (double)(p.blocks ? p.blocks : 1), h[0] / it, h[1] / it, h[2] / it, h[3] / it);
        bool any_phase = false;
        for (int k = 6; k < 16; ++k) any_phase = any_phase || h[k] != 0;
        if (any_phase) {
            fprintf(stderr, "[fg prof] %s stage-B phases (cycles per iteration):", name);
            for (int k = 6; k < 16; ++k) fprintf(stderr, " %.0f", h[k] / it);
            fprintf(stderr, "\n");
        }
    }
};

// The instantiation a launcher has picked, named ONCE: the kernel the product runs -- the function plan_launch asks the occupancy of
// and the function that is launched -- and its PROF = true twin (the same signature; FG_PROF_TWIN(k<.., true, ..>): null in the
// product build, which does not compile it), with the name the measurement build prints.
template <class K>
struct Kernels {
    K run, prof;
    const char* name;
};
template <class K>
inline Kernels<K> kernels(K run, typename SameAs<K>::type prof, const char* name) { return Kernels<K>{run, prof, name}; }

// What a decode launcher was handed and passes on
struct DecodeCall {
    uint64_t n;
    const DevTables* t;
    hipStream_t stream;
    FrameArgs fr;
    const fg_launch_opts* lo;
    TicketSlot* tk;
};
// A planned launch: tickets, the entry chunk of THIS grid, the launch -- go(kernel, plan, tables, frame args, prof words) puts the
// format's own arguments around them -- and the launch's error.  Measurement build under FG_PROF: the twin, bracketed by a ProfRun
// (prof_tickets = false: that launch draws no tickets and runs its chunks round-robin).
template <class K, class Go>
inline int launch_planned(const Kernels<K>& k, const LaunchPlan& p, const DecodeCall& c, Go go, bool prof_tickets = true) {
    const bool prof = k.prof != nullptr && prof_requested();
    FrameArgs fr = c.fr;
    if (!prof || prof_tickets) take_tickets(&fr, c.tk, p);
    DevTables tt = *c.t;
    tt.alloc_chunk = entry_chunk(tt.ent_cap, p.blocks, c.n, *c.lo, tt.shares);
    if (prof) {
        ProfRun pr;
        if (!pr.begin(c.stream)) return -1;
        go(k.prof, p, tt, fr, pr.d);
        pr.end(c.stream, k.name, p);
    } else {
        go(k.run, p, tt, fr, (unsigned long long*)nullptr);
    }
    return (int)hipGetLastError();
}
// ... behind its plan (plan_launch's arguments from avg_len on)
template <class K, class Go>
inline int plan_and_launch(const Kernels<K>& k, const DecodeCall& c, uint64_t avg_len, uint32_t extra_lds, uint32_t max_tile, uint32_t stash_blocks,
                           const PlanFormat& pf, Go go) {
    LaunchPlan p;
    if (plan_launch(k.run, c.n, avg_len, extra_lds, max_tile, stash_blocks, &p, *c.lo, pf)) return -1;
    return launch_planned(k, p, c, go);
}
}  // namespace fg
