// deflate_driver.hpp -- the passes of fg_deflate.hip as host loops over fg_deflate.hpp on the wave emulation: what a kernel does per
// wave or per lane, a loop does per iteration, with the kernels' arguments (test infrastructure, host only).
#pragma once
#include <vector>

#include "fg_deflate.hpp"

namespace fgd {
namespace df = fg::deflate;

constexpr uint64_t kBadArgs = ~0ull;
// A lane's stack, 0 = the emulation's own size.  The emulation keeps ONE set of lane stacks per thread and process, sized by the first wave
// that runs (across every library loaded into the process: its state is an inline function's static), so only a program that runs
// nothing but these loops may ask for another size -- deflate_san_main.cpp does, because what AddressSanitizer does per context switch
// grows with the stack's size.
inline size_t& lane_stack() {
    static size_t v = 0;
    return v;
}
template <class Body>
inline void run_wave(Body&& body) {
    if (lane_stack()) fg::emu::run_wave(body, lane_stack());
    else fg::emu::run_wave(body);
}

// k_df_count and its scan: blk_first[n_members + 1]; false for cuts the compressor refuses
inline bool count(const uint64_t* cuts, uint64_t n_members, uint64_t nbytes, uint64_t* blk_first) {
    uint64_t nb = 0;
    bool ok = true;
    for (uint64_t m = 0; m < n_members; ++m) {
        blk_first[m] = nb;
        if (df::member_ok(cuts[m], cuts[m + 1], nbytes)) nb += df::blocks_of(cuts[m + 1] - cuts[m]);
        else ok = false;
    }
    blk_first[n_members] = nb;
    return ok;
}
// k_df_blocks: every block into its slot
inline void blocks(const uint8_t* bytes, const uint64_t* cuts, const uint64_t* blk_first, uint64_t n_members, uint8_t* slots, uint32_t* blk_size,
                   uint32_t* blk_crc) {
    std::vector<uint32_t> lds(df::kLdsWords);
    for (uint64_t g = 0; g < blk_first[n_members]; ++g) {
        const uint64_t m = df::member_of(blk_first, n_members, g), j = g - blk_first[m];
        const uint64_t start = cuts[m] + j * df::kBlock;
        const uint32_t len = (uint32_t)(cuts[m + 1] - start < df::kBlock ? cuts[m + 1] - start : df::kBlock);
        const bool last = g + 1u == blk_first[m + 1];
        uint32_t* out32 = reinterpret_cast<uint32_t*>(slots + df::slot_offset(start, g));
        run_wave([&] {
            uint32_t crc;
            const uint32_t size = df::compress_block(bytes + start, len, last, out32, df::lds_of(lds.data()), &crc);
            if (fg::wv::lane() == 0u) {
                blk_size[g] = size;
                blk_crc[g] = crc;
            }
        });
    }
}
// k_df_finish and its scan: z_offsets[n_members + 1]; returns the total
inline uint64_t sizes(const uint64_t* cuts, const uint64_t* blk_first, uint64_t n_members, const uint32_t* blk_size, const uint32_t* blk_crc,
                      uint32_t* blk_rel, uint32_t* member_crc, uint64_t* z_offsets) {
    uint64_t o = 0;
    for (uint64_t m = 0; m < n_members; ++m) {
        z_offsets[m] = o;
        o += df::finish_member(blk_first[m], blk_first[m + 1], cuts[m + 1] - cuts[m], blk_size, blk_crc, blk_rel, &member_crc[m]);
    }
    z_offsets[n_members] = o;
    return o;
}
// k_df_pack
inline void pack(const uint8_t* bytes, const uint64_t* cuts, const uint64_t* blk_first, uint64_t n_members, const uint8_t* slots, const uint32_t* blk_size,
                 const uint32_t* blk_rel, const uint32_t* member_crc, const uint64_t* z_offsets, uint8_t* z, uint64_t z_cap) {
    for (uint64_t g = 0; g < blk_first[n_members]; ++g)
        run_wave([&] { df::pack_block(bytes, cuts, blk_first, n_members, g, slots, blk_size, blk_rel, member_crc, z_offsets, z, z_cap); });
}

// fg_deflate_device: cuts[n_members + 1] over bytes[0 .. nbytes) -> z_offsets[n_members + 1] and, with z != nullptr and the total within
// z_cap, the members in z.  Returns the total, or kBadArgs for cuts the compressor refuses.
inline uint64_t deflate(const uint8_t* bytes, uint64_t nbytes, const uint64_t* cuts, uint64_t n_members, uint8_t* z, uint64_t z_cap,
                        uint64_t* z_offsets) {
    std::vector<uint64_t> blk_first(n_members + 1u);
    if (!count(cuts, n_members, nbytes, blk_first.data())) return kBadArgs;
    const uint64_t nb = blk_first[n_members];
    std::vector<uint32_t> slots(df::slot_bytes(nbytes, nb) / 4u + 1u), blk_size(nb + 1u), blk_crc(nb + 1u), blk_rel(nb + 1u), member_crc(n_members + 1u);
    blocks(bytes, cuts, blk_first.data(), n_members, reinterpret_cast<uint8_t*>(slots.data()), blk_size.data(), blk_crc.data());
    const uint64_t o = sizes(cuts, blk_first.data(), n_members, blk_size.data(), blk_crc.data(), blk_rel.data(), member_crc.data(), z_offsets);
    if (z && o <= z_cap)
        pack(bytes, cuts, blk_first.data(), n_members, reinterpret_cast<const uint8_t*>(slots.data()), blk_size.data(), blk_rel.data(), member_crc.data(), z_offsets,
             z, z_cap);
    return o;
}

// the cut kernels: out_offsets[n + 1] -> member_first / cuts (room for n + 2 entries each); returns the members
inline uint64_t members(const uint64_t* off, uint64_t n, uint64_t coalesce, uint64_t member_bytes, uint64_t* member_first, uint64_t* cuts) {
    if (coalesce >= 1u || n == 0u) {
        const uint64_t c = coalesce >= 1u ? coalesce : 1u, nm = df::coalesce_members(n, c);
        for (uint64_t k = 0; k <= nm; ++k) df::coalesce_cut(off, n, c, k, member_first, cuts);
        return nm;
    }
    const uint64_t b = member_bytes ? member_bytes : df::kBlock;
    uint64_t nm = 0;
    for (uint64_t i = 0; i < n; ++i)  // (the kernels: flags, their exclusive scan, a scatter)
        if (df::bytes_starts(off, i, b)) {
            member_first[nm] = i;
            cuts[nm++] = off[i];
        }
    member_first[nm] = n;
    cuts[nm] = off[n];
    return nm;
}

}  // namespace fgd
