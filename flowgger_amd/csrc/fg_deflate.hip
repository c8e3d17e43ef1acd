// fg_deflate.hip -- the output compressor on the device: gzip members over a resident byte buffer (fg_deflate_device), and the member
// cuts over an encoder's offsets.  Everything a wave or a lane decides is fg_deflate.hpp (HIP-free, the CPU suite runs it on the wave
// emulation); this file is the kernels' shells and their launchers.
//
// Sizes are unknown up front, so the shape is the encoders': compress into worst-case slots, scan, pack.
//   k_df_count    one lane per member: its cuts judged, its block count; per-64 sums          -> (scan) blk_first[n_members + 1]
//   k_df_blocks   one wave per block, dealt by ticket (a wave's first block is its workgroup index, every further one is drawn from
//                 one counter: blocks differ in cost by what they hold): fg::deflate::compress_block into the block's slot
//   k_df_blocks_dyn   the same shell around compress_block_dyn (FG_DEFLATE_DYNAMIC): the block's histogram, its codes, the cheapest form
//   k_df_finish   one lane per member: its blocks' offsets, its CRC-32, its size; per-64 sums  -> (scan) z_offsets[n_members + 1]
//   k_df_pack     one wave per block: the slot (or, stored, the input) behind the member's header, the trailer behind the last
// One 64-lane wave per workgroup with 16.3 KiB of LDS (the hash table, the bit buffer): nine workgroups share a CU's 160 KiB.  No loop
// waits on another wave; every loop of compress_block advances its window.
#include <hip/hip_runtime.h>

#include "fg_deflate.hpp"

namespace fg {
namespace deflate {

constexpr uint32_t kWave = 64;
constexpr uint32_t kWavesPerCu = 9;  // what the LDS leaves room for

__global__ __launch_bounds__(64) void k_df_count(const uint64_t* __restrict__ cuts, uint64_t n_members, uint64_t nbytes, uint32_t* __restrict__ nblk,
                                                 uint64_t* __restrict__ block_sums, uint32_t* __restrict__ err) {
    const uint64_t m = (uint64_t)blockIdx.x * kWave + threadIdx.x;
    uint32_t nb = 0;
    if (m < n_members) {
        const uint64_t a = cuts[m], b = cuts[m + 1];
        if (member_ok(a, b, nbytes)) nb = (uint32_t)blocks_of(b - a);
        else atomicOr(err, 1u);
        nblk[m] = nb;
    }
    uint64_t sum = nb;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, kWave);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = sum;
}

// (slots is written here and nowhere read: no __restrict__ needed; the input is only read)
__global__ __launch_bounds__(64) void k_df_blocks(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ cuts,
                                                  const uint64_t* __restrict__ blk_first, uint64_t n_members, uint64_t n_blocks, uint8_t* slots,
                                                  uint64_t slots_cap, uint32_t* __restrict__ blk_size, uint32_t* __restrict__ blk_crc,
                                                  uint32_t* __restrict__ ticket) {
    __shared__ uint32_t s_lds[kLdsWords];
    __shared__ uint32_t s_ticket;
    const Lds s = lds_of(s_lds);
    uint64_t g = blockIdx.x;
    while (g < n_blocks) {  // (wave-uniform)
        const uint64_t m = member_of(blk_first, n_members, g), j = g - blk_first[m];
        const uint64_t start = cuts[m] + j * kBlock, end = cuts[m + 1];
        const uint32_t len = (uint32_t)(end - start < kBlock ? end - start : kBlock);
        const bool last = g + 1u == blk_first[m + 1];
        const uint64_t so = slot_offset(start, g);
        uint32_t size = (len + 5u) | kStored, crc = 0u;
        if (start < end && so + len + kSlotPad <= slots_cap)  // (always: blk_first is the scan of these cuts, the slots were sized by them)
            size = compress_block(bytes + start, len, last, (uint32_t*)(slots + so), s, &crc);
        if (threadIdx.x == 0) {
            blk_size[g] = size;
            blk_crc[g] = crc;
            s_ticket = atomicAdd(ticket, 1u);
        }
        __syncthreads();
        g = (uint64_t)gridDim.x + s_ticket;
        __syncthreads();
    }
}

// k_df_blocks for FG_DEFLATE_DYNAMIC: the same shell around compress_block_dyn (17.6 KiB of LDS: nine workgroups still share a CU)
__global__ __launch_bounds__(64) void k_df_blocks_dyn(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ cuts,
                                                      const uint64_t* __restrict__ blk_first, uint64_t n_members, uint64_t n_blocks, uint8_t* slots,
                                                      uint64_t slots_cap, uint32_t* __restrict__ blk_size, uint32_t* __restrict__ blk_crc,
                                                      uint32_t* __restrict__ ticket) {
    __shared__ uint32_t s_lds[kDynLdsWords];
    __shared__ uint32_t s_ticket;
    const DynLds s = dyn_lds_of(s_lds);
    uint64_t g = blockIdx.x;
    while (g < n_blocks) {  // (wave-uniform)
        const uint64_t m = member_of(blk_first, n_members, g), j = g - blk_first[m];
        const uint64_t start = cuts[m] + j * kBlock, end = cuts[m + 1];
        const uint32_t len = (uint32_t)(end - start < kBlock ? end - start : kBlock);
        const bool last = g + 1u == blk_first[m + 1];
        const uint64_t so = slot_offset(start, g);
        uint32_t size = (len + 5u) | kStored, crc = 0u, info;
        if (start < end && so + len + kSlotPad <= slots_cap)  // (always, as in k_df_blocks)
            size = compress_block_dyn(bytes + start, len, last, (uint32_t*)(slots + so), s, &crc, &info);
        if (threadIdx.x == 0) {
            blk_size[g] = size;
            blk_crc[g] = crc;
            s_ticket = atomicAdd(ticket, 1u);
        }
        __syncthreads();
        g = (uint64_t)gridDim.x + s_ticket;
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void k_df_finish(const uint64_t* __restrict__ cuts, const uint64_t* __restrict__ blk_first, uint64_t n_members,
                                                  const uint32_t* __restrict__ blk_size, const uint32_t* __restrict__ blk_crc,
                                                  uint32_t* __restrict__ blk_rel, uint32_t* __restrict__ member_crc, uint32_t* __restrict__ msize,
                                                  uint64_t* __restrict__ block_sums) {
    const uint64_t m = (uint64_t)blockIdx.x * kWave + threadIdx.x;
    uint32_t size = 0;
    if (m < n_members) {
        uint32_t crc;
        size = finish_member(blk_first[m], blk_first[m + 1], cuts[m + 1] - cuts[m], blk_size, blk_crc, blk_rel, &crc);
        member_crc[m] = crc;
        msize[m] = size;
    }
    uint64_t sum = size;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, kWave);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = sum;
}

__global__ __launch_bounds__(64) void k_df_pack(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ cuts,
                                                const uint64_t* __restrict__ blk_first, uint64_t n_members, uint64_t n_blocks,
                                                const uint8_t* __restrict__ slots, const uint32_t* __restrict__ blk_size,
                                                const uint32_t* __restrict__ blk_rel, const uint32_t* __restrict__ member_crc,
                                                const uint64_t* __restrict__ z_off, uint8_t* __restrict__ z, uint64_t z_cap) {
    for (uint64_t g = blockIdx.x; g < n_blocks; g += gridDim.x)
        pack_block(bytes, cuts, blk_first, n_members, g, slots, blk_size, blk_rel, member_crc, z_off, z, z_cap);
}

// ---- member cuts over out_offsets[n + 1]
__global__ __launch_bounds__(64) void k_df_cut_coalesce(const uint64_t* __restrict__ off, uint64_t n, uint64_t c, uint64_t n_members,
                                                        uint64_t* __restrict__ member_first, uint64_t* __restrict__ cuts,
                                                        uint64_t* __restrict__ d_n_members) {
    const uint64_t k = (uint64_t)blockIdx.x * kWave + threadIdx.x;
    if (k <= n_members) coalesce_cut(off, n, c, k, member_first, cuts);
    if (k == 0) *d_n_members = n_members;
}
__global__ __launch_bounds__(64) void k_df_cut_flags(const uint64_t* __restrict__ off, uint64_t n, uint64_t b, uint32_t* __restrict__ flags,
                                                     uint64_t* __restrict__ block_sums) {
    const uint64_t i = (uint64_t)blockIdx.x * kWave + threadIdx.x;
    uint32_t f = 0;
    if (i < n) flags[i] = f = bytes_starts(off, i, b) ? 1u : 0u;
    const uint32_t cnt = (uint32_t)__popcll(__ballot(f != 0u));
    if (threadIdx.x == 0) block_sums[blockIdx.x] = cnt;
}
__global__ __launch_bounds__(64) void k_df_cut_scatter(const uint64_t* __restrict__ off, uint64_t n, const uint32_t* __restrict__ flags,
                                                       const uint64_t* __restrict__ idx, uint64_t* __restrict__ member_first,
                                                       uint64_t* __restrict__ cuts, uint64_t* __restrict__ d_n_members) {
    const uint64_t i = (uint64_t)blockIdx.x * kWave + threadIdx.x;
    if (i < n && flags[i]) {  // (idx[i] < idx[n] <= n: inside the n + 1 entries)
        member_first[idx[i]] = i;
        cuts[idx[i]] = off[i];
    }
    if (i == 0) {
        const uint64_t nm = idx[n];
        member_first[nm] = n;
        cuts[nm] = off[n];
        *d_n_members = nm;
    }
}

}  // namespace deflate
}  // namespace fg

namespace df = fg::deflate;

extern "C" int fg_launch_encode_scan(const uint32_t* d_sizes, uint64_t* d_block_sums, uint64_t n, uint64_t* d_out_offsets, uint64_t base,
                                     hipStream_t stream);

extern "C" uint32_t fg_deflate_block_bytes(void) { return df::kBlock; }
extern "C" uint64_t fg_deflate_bound(uint64_t nbytes, uint64_t n_members) { return df::bound(nbytes, n_members); }
extern "C" uint64_t fg_deflate_max_member(void) { return df::kMaxMember; }
extern "C" uint64_t fg_deflate_slot_bytes(uint64_t nbytes, uint64_t n_blocks) { return df::slot_bytes(nbytes, n_blocks); }

// d_nblk: n_members u32; d_sums: ceil(n_members / 64) u64; d_blk_first: n_members + 1 u64; *d_err (cleared here) != 0 afterwards: cuts
// that do not ascend, go past nbytes or bound a member of fg_deflate_max_member() bytes or more.  n_members > 0.
extern "C" int fg_launch_deflate_count(const uint64_t* d_cuts, uint64_t n_members, uint64_t nbytes, uint32_t* d_nblk, uint64_t* d_sums,
                                       uint64_t* d_blk_first, uint32_t* d_err, hipStream_t stream) {
    const uint64_t blocks = (n_members + 63u) / 64u;
    if (blocks > 0x7FFFFFFFull) return -1;
    int rc = (int)hipMemsetAsync(d_err, 0, 4, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(df::k_df_count, dim3((uint32_t)blocks), dim3(64), 0, stream, d_cuts, n_members, nbytes, d_nblk, d_sums, d_err);
    rc = (int)hipGetLastError();
    if (rc == 0) rc = fg_launch_encode_scan(d_nblk, d_sums, n_members, d_blk_first, 0ull, stream);
    return rc;
}
// every block into its slot of d_slots[0 .. slots_cap) (slots_cap >= fg_deflate_slot_bytes(nbytes, n_blocks)); d_blk_size, d_blk_crc:
// n_blocks u32 each; d_ticket: one word (cleared here).  n_blocks > 0; cus = the device's compute units.
extern "C" int fg_launch_deflate_blocks(const uint8_t* d_bytes, const uint64_t* d_cuts, const uint64_t* d_blk_first, uint64_t n_members,
                                        uint64_t n_blocks, uint8_t* d_slots, uint64_t slots_cap, uint32_t* d_blk_size, uint32_t* d_blk_crc,
                                        uint32_t* d_ticket, int cus, hipStream_t stream) {
    if (n_blocks > 0x7FFFFFFFull || ((uintptr_t)d_slots & 3u) != 0) return -1;
    const uint64_t resident = (uint64_t)(cus > 0 ? cus : 1) * df::kWavesPerCu;
    const uint32_t grid = (uint32_t)(n_blocks < resident ? n_blocks : resident);
    int rc = (int)hipMemsetAsync(d_ticket, 0, 4, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(df::k_df_blocks, dim3(grid), dim3(64), 0, stream, d_bytes, d_cuts, d_blk_first, n_members, n_blocks, d_slots, slots_cap, d_blk_size,
                       d_blk_crc, d_ticket);
    return (int)hipGetLastError();
}
// fg_launch_deflate_blocks for FG_DEFLATE_DYNAMIC (fg_set_deflate_mode): the same arguments, the same slots
extern "C" int fg_launch_deflate_blocks_dyn(const uint8_t* d_bytes, const uint64_t* d_cuts, const uint64_t* d_blk_first, uint64_t n_members,
                                            uint64_t n_blocks, uint8_t* d_slots, uint64_t slots_cap, uint32_t* d_blk_size, uint32_t* d_blk_crc,
                                            uint32_t* d_ticket, int cus, hipStream_t stream) {
    if (n_blocks > 0x7FFFFFFFull || ((uintptr_t)d_slots & 3u) != 0) return -1;
    const uint64_t resident = (uint64_t)(cus > 0 ? cus : 1) * df::kWavesPerCu;
    const uint32_t grid = (uint32_t)(n_blocks < resident ? n_blocks : resident);
    int rc = (int)hipMemsetAsync(d_ticket, 0, 4, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(df::k_df_blocks_dyn, dim3(grid), dim3(64), 0, stream, d_bytes, d_cuts, d_blk_first, n_members, n_blocks, d_slots, slots_cap,
                       d_blk_size, d_blk_crc, d_ticket);
    return (int)hipGetLastError();
}
// the members' sizes: d_blk_rel n_blocks u32, d_member_crc / d_msize n_members u32, d_sums ceil(n_members / 64) u64 -> d_z_offsets[n_members + 1]
extern "C" int fg_launch_deflate_sizes(const uint64_t* d_cuts, const uint64_t* d_blk_first, uint64_t n_members, const uint32_t* d_blk_size,
                                       const uint32_t* d_blk_crc, uint32_t* d_blk_rel, uint32_t* d_member_crc, uint32_t* d_msize, uint64_t* d_sums,
                                       uint64_t* d_z_offsets, hipStream_t stream) {
    const uint64_t blocks = (n_members + 63u) / 64u;
    if (blocks > 0x7FFFFFFFull) return -1;
    hipLaunchKernelGGL(df::k_df_finish, dim3((uint32_t)blocks), dim3(64), 0, stream, d_cuts, d_blk_first, n_members, d_blk_size, d_blk_crc, d_blk_rel,
                       d_member_crc, d_msize, d_sums);
    int rc = (int)hipGetLastError();
    if (rc == 0) rc = fg_launch_encode_scan(d_msize, d_sums, n_members, d_z_offsets, 0ull, stream);
    return rc;
}
// ... and the members into d_z[0 .. z_cap), z_cap >= d_z_offsets[n_members]
extern "C" int fg_launch_deflate_pack(const uint8_t* d_bytes, const uint64_t* d_cuts, const uint64_t* d_blk_first, uint64_t n_members, uint64_t n_blocks,
                                      const uint8_t* d_slots, const uint32_t* d_blk_size, const uint32_t* d_blk_rel, const uint32_t* d_member_crc,
                                      const uint64_t* d_z_offsets, uint8_t* d_z, uint64_t z_cap, hipStream_t stream) {
    if (n_blocks == 0) return 0;
    const uint32_t grid = (uint32_t)(n_blocks < 0x100000ull ? n_blocks : 0x100000ull);
    hipLaunchKernelGGL(df::k_df_pack, dim3(grid), dim3(64), 0, stream, d_bytes, d_cuts, d_blk_first, n_members, n_blocks, d_slots, d_blk_size, d_blk_rel,
                       d_member_crc, d_z_offsets, d_z, z_cap);
    return (int)hipGetLastError();
}
// out_offsets[n + 1] -> d_member_first / d_cuts (n + 2 u64 each) and *d_n_members, by fg_compress_cfg's two policies.  d_flags: n u32;
// d_sums: ceil(n / 64) u64; d_idx: n + 1 u64 (the three are used by the member_bytes policy only).
extern "C" int fg_launch_deflate_cuts(const uint64_t* d_off, uint64_t n, uint64_t coalesce, uint64_t member_bytes, uint32_t* d_flags, uint64_t* d_sums,
                                      uint64_t* d_idx, uint64_t* d_member_first, uint64_t* d_cuts, uint64_t* d_n_members, hipStream_t stream) {
    if (coalesce >= 1u || n == 0) {
        const uint64_t c = coalesce >= 1u ? coalesce : 1u, nm = df::coalesce_members(n, c), blocks = (nm + 1u + 63u) / 64u;
        if (blocks > 0x7FFFFFFFull) return -1;
        hipLaunchKernelGGL(df::k_df_cut_coalesce, dim3((uint32_t)blocks), dim3(64), 0, stream, d_off, n, c, nm, d_member_first, d_cuts, d_n_members);
        return (int)hipGetLastError();
    }
    const uint64_t blocks = (n + 63u) / 64u, b = member_bytes ? member_bytes : df::kBlock;
    if (blocks > 0x7FFFFFFFull) return -1;
    hipLaunchKernelGGL(df::k_df_cut_flags, dim3((uint32_t)blocks), dim3(64), 0, stream, d_off, n, b, d_flags, d_sums);
    int rc = (int)hipGetLastError();
    if (rc == 0) rc = fg_launch_encode_scan(d_flags, d_sums, n, d_idx, 0ull, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(df::k_df_cut_scatter, dim3((uint32_t)blocks), dim3(64), 0, stream, d_off, n, d_flags, d_idx, d_member_first, d_cuts, d_n_members);
    return (int)hipGetLastError();
}
