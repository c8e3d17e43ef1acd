// fg_capnp.hip -- gfx950 kernel for the Cap'n Proto input (input.format = "capnp"): CapnpSplitter's handle_message
// (src/flowgger/splitter/capnp_splitter.rs:65-167) for every message of a batch.
//
// The per-message logic is fg_capnp_parse.hpp (host + device; checked on the CPU against a Python model of the reader).  The
// kernel is a format of the shared streaming pipeline (fg_pipeline.hpp): persistent waves, chunks of messages by ticket, a
// group of up to 64 consecutive messages = one contiguous byte range staged into the wave's LDS tile through the register
// prefetch window, then ONE LANE PER MESSAGE resolves the root struct, the seven texts and the two pair lists out of LDS with
// aligned 8-byte reads (a message starts on a word, the tile on sixteen bytes).  No byte class is needed: stage A classifies
// nothing.  The entries of a message (the element, the kept pairs, the kept extras) are COUNTED by the parse, get their slots
// from the wave's reservation (alloc_entries_ex, FG_ST_OVERFLOW when the table is used up) and are written by a second walk
// over the two lists, which the parse has already resolved.  A message longer than the tile is a group of its own and is read
// from global memory by its one lane, word by word.
// Roofline: HBM -- message bytes + 8 B offset read once, 68 B per row + 18 B per entry written.
#include "fg_pipeline.hpp"
#include "fg_capnp_parse.hpp"

namespace fg {

// words of ONE message: out of the tile when the message lies in it, else from global memory (a branch per read instead of two
// instantiations of the parser)
struct CapnpWords {
    const uint64_t* lds;  // the message's first word in the tile, or null
    const uint64_t* glb;  // ... in the packed buffer
    __device__ __forceinline__ uint64_t word(uint32_t w) const { return lds ? lds[w] : glb[w]; }
};
struct CapnpFormat {
    static constexpr uint32_t kClasses = 0;
    static __device__ __forceinline__ void classify_store(const uint4&, uint16_t*, uint32_t, uint32_t, uint32_t) {}

    __device__ __forceinline__ RowOut decode(const GroupCtx& c, const DevTables& t) const {
        const uint64_t len = c.o1 - c.o0;
        const bool whole = (c.o1 - c.a0) <= (uint64_t)c.span;
        capnp::Row r;
        capnp::Msg m;
        CapnpWords rd{whole ? reinterpret_cast<const uint64_t*>(c.smem + (uint32_t)(c.o0 - c.a0)) : nullptr,
                      reinterpret_cast<const uint64_t*>(c.bytes + c.o0)};
        if (c.valid) {
            if ((c.o0 & 7ull) != 0ull) r.status = capnp::ST_NO_ROOT;  // (a message starts on a word: include/fg_hip.h)
            else capnp::parse_message(rd, len, r, m);
            if (r.status != capnp::ST_OK) r.n_ent = 0;
        }
        const EntAlloc ea = alloc_entries_ex(t, r.n_ent, c.ent_state);
        if (ea.overflow) {
            r.status = FG_ST_OVERFLOW;
            r.n_ent = 0;
        }
        const uint32_t first = (ea.overflow || ea.total == 0u) ? 0u : ea.s.at(ea.ex);
        if (r.n_ent != 0u) {
            // (a message's slice is contiguous: the wave's reservations are cut between lanes, alloc_entries_ex)
            struct Sink {
                const DevTables& t;
                uint32_t first;
                __device__ __forceinline__ void put(uint32_t k, fg_span name, uint64_t val, uint32_t type, uint32_t flags) {
                    gstore(t.ent_name, first + k, name);
                    gstore(t.ent_val, first + k, val);
                    gstore(t.ent_type, first + k, (uint8_t)type);
                    gstore(t.ent_flags, first + k, (uint8_t)flags);
                }
            } sink{t, first};
            capnp::emit_entries(rd, m, r, sink);
        }
        RowOut o;
        const bool ok = r.status == capnp::ST_OK;
        o.meta = r.status | ((ok ? r.fac : 0xFFu) << 8) | ((ok ? r.sev : 0xFFu) << 16);
        o.ts = ok ? __longlong_as_double((long long)r.ts_bits) : 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) o.span[k] = ok ? r.sp[k] : fg_span{0u, FG_NONE};
        o.first = first;
        o.count = r.n_ent;
        return o;
    }
};

template <int NB, bool PROF>
__global__ __launch_bounds__(kWave, 2) void k_capnp(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                                                   DevTables t, uint32_t tile_cap, uint32_t L, uint64_t chunk, unsigned long long* prof,
                                                   FrameArgs fr) {
    // (the pipeline gets an LDS copy of the tables: see k_ltsv)
    __shared__ DevTables t_call;
    if (threadIdx.x == 0) t_call = t;
    __syncthreads();
    CapnpFormat fmt;
    persistent_loop<NB, PROF, CapnpFormat>(bytes, offsets, n, t_call, tile_cap, L, chunk, prof, nullptr, fmt, fr);
}

}  // namespace fg

extern "C" int fg_launch_capnp(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const fg::DevTables* t, uint64_t avg_len,
                               hipStream_t stream, const uint8_t* line_bad, const fg_launch_opts* lo, fg::TicketSlot* tk) {
    if (n == 0) return 0;
    const auto ks = fg::kernels(fg::k_capnp<fg::kWindowKiB, false>, FG_PROF_TWIN(fg::k_capnp<fg::kWindowKiB, true>), "capnp");
    return fg::plan_and_launch(ks, fg::DecodeCall{n, t, stream, fg::FrameArgs{FG_FRAME_NONE, line_bad}, lo, tk}, avg_len, 0u, fg::kMaxTile, 0u,
                               fg::PlanFormat().classes(0u),
                               [&](auto k, const fg::LaunchPlan& p, const fg::DevTables& tt, const fg::FrameArgs& fr, unsigned long long* prof) {
                                   hipLaunchKernelGGL(k, dim3(p.blocks), dim3(fg::kWave), p.lds, stream, d_bytes, d_offsets, n, tt, p.tile, p.L, p.chunk,
                                                      prof, fr);
                               });
}
