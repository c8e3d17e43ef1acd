// deflate_dyn_driver.hpp -- deflate_driver.hpp's loops for FG_DEFLATE_DYNAMIC: k_df_blocks_dyn as a host loop over
// fg::deflate::compress_block_dyn on the wave emulation, the whole of fg_deflate_device in either mode, and the code builder alone
// (test infrastructure, host only).
#pragma once
#include "deflate_driver.hpp"

namespace fgd {

// k_df_blocks_dyn: every block into its slot; blk_info (may be null): compress_block_dyn's *info per block
inline void blocks_dyn(const uint8_t* bytes, const uint64_t* cuts, const uint64_t* blk_first, uint64_t n_members, uint8_t* slots, uint32_t* blk_size,
                       uint32_t* blk_crc, uint32_t* blk_info) {
    std::vector<uint32_t> lds(df::kDynLdsWords);
    for (uint64_t g = 0; g < blk_first[n_members]; ++g) {
        const uint64_t m = df::member_of(blk_first, n_members, g), j = g - blk_first[m];
        const uint64_t start = cuts[m] + j * df::kBlock;
        const uint32_t len = (uint32_t)(cuts[m + 1] - start < df::kBlock ? cuts[m + 1] - start : df::kBlock);
        const bool last = g + 1u == blk_first[m + 1];
        uint32_t* out32 = reinterpret_cast<uint32_t*>(slots + df::slot_offset(start, g));
        run_wave([&] {
            uint32_t crc, info;
            const uint32_t size = df::compress_block_dyn(bytes + start, len, last, out32, df::dyn_lds_of(lds.data()), &crc, &info);
            if (fg::wv::lane() == 0u) {
                blk_size[g] = size;
                blk_crc[g] = crc;
                if (blk_info) blk_info[g] = info;
            }
        });
    }
}

// deflate() with the mode: 0 fixed, 1 dynamic.  blk_info (may be null) has room for every block.
inline uint64_t deflate_mode(const uint8_t* bytes, uint64_t nbytes, const uint64_t* cuts, uint64_t n_members, int mode, uint8_t* z, uint64_t z_cap,
                             uint64_t* z_offsets, uint32_t* blk_info) {
    std::vector<uint64_t> blk_first(n_members + 1u);
    if (!count(cuts, n_members, nbytes, blk_first.data())) return kBadArgs;
    const uint64_t nb = blk_first[n_members];
    std::vector<uint32_t> slots(df::slot_bytes(nbytes, nb) / 4u + 1u), blk_size(nb + 1u), blk_crc(nb + 1u), blk_rel(nb + 1u), member_crc(n_members + 1u);
    uint8_t* sl = reinterpret_cast<uint8_t*>(slots.data());
    if (mode) blocks_dyn(bytes, cuts, blk_first.data(), n_members, sl, blk_size.data(), blk_crc.data(), blk_info);
    else blocks(bytes, cuts, blk_first.data(), n_members, sl, blk_size.data(), blk_crc.data());
    const uint64_t o = sizes(cuts, blk_first.data(), n_members, blk_size.data(), blk_crc.data(), blk_rel.data(), member_crc.data(), z_offsets);
    if (z && o <= z_cap) pack(bytes, cuts, blk_first.data(), n_members, sl, blk_size.data(), blk_rel.data(), member_crc.data(), z_offsets, z, z_cap);
    return o;
}

// build_lengths alone: freq[n] -> lengths[n]; returns the cost, *limited as the builder reports it
inline uint32_t build(const uint32_t* freq, uint32_t n, uint32_t limit, uint32_t* lengths, uint32_t* limited) {
    std::vector<uint32_t> f(freq, freq + n), ws(df::kWsBuild);
    uint32_t cost = 0;
    run_wave([&] {
        bool lim;
        const uint32_t c = df::build_lengths(f.data(), n, limit, ws.data(), &lim);
        if (fg::wv::lane() == 0u) {
            cost = c;
            *limited = lim ? 1u : 0u;
        }
    });
    for (uint32_t k = 0; k < n; ++k) lengths[k] = f[k];
    return cost;
}

}  // namespace fgd
