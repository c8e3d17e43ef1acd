// C wrappers around flowgger_amd/csrc/fg_plan_policy.hpp for tests/test_plan_policy_cpu.py (the launch policies are host arithmetic)
#include "../../flowgger_amd/csrc/fg_plan_policy.hpp"

extern "C" {
// out[0] chunk, out[1] chunks, out[2] blocks, out[3] tickets, out[4..6] taper
void fgp_plan_chunks(uint64_t n, uint64_t blocks, uint32_t L, uint64_t g, uint64_t full, uint32_t ticket_from, uint32_t flags, uint32_t chunk_lines,
                     uint32_t taper, uint64_t* out) {
    fg_launch_opts lo{};
    lo.flags = flags;
    lo.chunk_lines = chunk_lines;
    const fg::ChunkPlan p = fg::plan_chunks(n, blocks, L, g, full, ticket_from, lo, taper);
    out[0] = p.chunk;
    out[1] = p.chunks;
    out[2] = p.blocks;
    out[3] = p.tickets ? 1 : 0;
    for (int j = 0; j < 3; ++j) out[4 + j] = p.taper[j];
}
void fgp_chunk_range(uint64_t c, uint64_t chunk, uint32_t t0, uint32_t t1, uint32_t t2, uint64_t n, uint64_t* lo_hi) {
    fg::chunk_range(c, chunk, t0, t1, t2, n, &lo_hi[0], &lo_hi[1]);
}
// fg::launch_geometry for a format described by plain numbers (per_line != 0: a format with per-line LDS arrays, of no bytes here).
// out[0] L, out[1] tile, out[2] lds, out[3] groups, out[4] full, out[5] g
static uint32_t no_extra(uint32_t, uint32_t) { return 0u; }
static void put_geometry(const fg::LaunchGeometry& p, uint64_t* out) {
    out[0] = p.L, out[1] = p.tile, out[2] = p.lds, out[3] = p.groups, out[4] = p.full, out[5] = p.g;
}
void fgp_launch_geometry(uint64_t n, uint64_t avg_len, uint32_t extra_lds, uint32_t max_tile, uint32_t tile_cap, uint32_t lines_per_group,
                         uint32_t max_lines, uint32_t classes, uint32_t default_tile, uint32_t default_chunk, int per_line, uint64_t* out) {
    fg_launch_opts lo{};
    lo.tile_cap = tile_cap;
    lo.lines_per_group = lines_per_group;
    fg::PlanFormat pf = fg::PlanFormat().lines(max_lines).classes(classes).tile(default_tile).chunk(default_chunk);
    if (per_line) pf.lds_for(no_extra);
    put_geometry(fg::launch_geometry(n, avg_len, extra_lds, max_tile, lo, pf), out);
}
// ... of the RFC5424 launch without the pair-parallel walk, as fg_launch_rfc5424 plans it; out[6] ticket_from, out[7] taper levels
void fgp_rfc5424_walk_geometry(uint64_t n, uint64_t avg_len, uint32_t tile_cap, uint32_t lines_per_group, uint64_t* out) {
    fg_launch_opts lo{};
    lo.tile_cap = tile_cap;
    lo.lines_per_group = lines_per_group;
    const fg::PlanFormat pf = fg::rfc5424_walk_format(avg_len);
    put_geometry(fg::launch_geometry(n, avg_len, 0u, fg::kMaxTile, lo, pf), out);
    out[6] = pf.ticket_from, out[7] = pf.taper;
}
uint32_t fgp_short_line_tile(void) { return fg::kShortLineTile; }
// bit 0: head staging, bit 1: the pair-parallel structured-data walk
uint32_t fgp_pick_variant(uint64_t avg_len, uint32_t flags) {
    const fg::Variant v = fg::pick_variant(avg_len, flags);
    return (v.head ? 1u : 0u) | (v.pairs ? 2u : 0u);
}
int fgp_gelf_const_3k(uint64_t avg_len, uint32_t tile_cap, uint32_t flags) {
    fg_launch_opts lo{};
    lo.tile_cap = tile_cap;
    lo.flags = flags;
    return fg::gelf_const_3k(avg_len, lo) ? 1 : 0;
}
uint32_t fgp_entry_chunk(uint64_t ent_cap, uint32_t blocks, uint64_t n, uint32_t ent_chunk) {
    fg_launch_opts lo{};
    lo.ent_chunk = ent_chunk;
    return fg::entry_chunk(ent_cap, blocks, n, lo);
}
uint32_t fgp_entry_chunk_shared(uint64_t ent_cap, uint32_t blocks, uint64_t n, uint32_t ent_chunk, uint32_t shares) {
    fg_launch_opts lo{};
    lo.ent_chunk = ent_chunk;
    return fg::entry_chunk(ent_cap, blocks, n, lo, shares);
}
}
