// fg_kafka.hip -- Kafka v0 message sets on the device: an encoder's resident output as a message set (fg_kafka_messageset_device) and
// compressed members inside their wrapper messages (fg_kafka_wrap_device).  Everything a wave or a lane decides is fg_kafka.hpp
// (HIP-free, the CPU suite runs it on the wave emulation); this file is the kernels' shells and their launchers.
//
//   k_kf_sizes         one lane per message: its offsets judged, its wire size; per-64 sums        -> (scan) set_offsets[n + 1]
//   k_kf_write         one wave per four messages (a row of sixteen lanes each, the wave for a long one), grid-stride: header, CRC-32
//                      and the value's copy in one pass over the bytes
//   k_kf_cuts          one lane per member: its cut in the set = set_offsets[member_first[k]]
//   k_kf_wrap_sizes    one lane per member: its wrapper's size, its pieces; per-64 sums of both    -> (scans) w_offsets, piece_first
//   k_kf_wrap          one wave per piece of kPiece bytes, grid-stride: the copy behind the header's place, the piece's CRC register
//   k_kf_wrap_finish   one lane per member: the registers folded, the header
// One 64-lane wave per workgroup with 4.4 KiB of LDS (the CRC tables, built by every wave once); the grid is what is resident, each
// wave takes steps blockIdx.x, blockIdx.x + gridDim.x, ...: which wave writes a message changes nothing about its bytes.
#include <hip/hip_runtime.h>

#include "fg_kafka.hpp"

namespace fg {
namespace kafka {

constexpr uint32_t kWave = 64;
constexpr uint32_t kWavesPerCu = 24;  // six a SIMD: what the registers of k_kf_write leave room for

__global__ __launch_bounds__(64) void k_kf_sizes(const uint64_t* __restrict__ off, const uint8_t* __restrict__ skip, uint64_t n, uint64_t nbytes,
                                                 uint32_t* __restrict__ sizes, uint64_t* __restrict__ block_sums, uint32_t* __restrict__ err) {
    const uint64_t i = (uint64_t)blockIdx.x * kWave + threadIdx.x;
    uint32_t sz = 0;
    if (i < n) {
        const uint64_t a = off[i], b = off[i + 1];
        if (!value_ok(a, b, nbytes)) atomicOr(err, 1u);
        else sz = (uint32_t)wire_size(b - a, skip && skip[i]);
        sizes[i] = sz;
    }
    uint64_t sum = sz;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, kWave);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = sum;
}

__global__ __launch_bounds__(64) void k_kf_write(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ off, const uint8_t* __restrict__ skip,
                                                 uint64_t n, const uint64_t* __restrict__ set_off, uint8_t* __restrict__ set, uint64_t set_cap) {
    __shared__ uint32_t s_lds[kLdsWords];
    build_tables(s_lds);
    const Lds s = lds_of(s_lds);
    const uint64_t steps = write_steps(n);
    for (uint64_t k = blockIdx.x; k < steps; k += gridDim.x) write_step(bytes, off, skip, n, k * kRowsPerWave, set_off, set, set_cap, s);
}

__global__ __launch_bounds__(64) void k_kf_cuts(const uint64_t* __restrict__ set_off, const uint64_t* __restrict__ member_first, uint64_t n,
                                                uint64_t n_members, uint64_t* __restrict__ set_cuts) {
    const uint64_t k = (uint64_t)blockIdx.x * kWave + threadIdx.x;
    if (k <= n_members) {
        const uint64_t i = member_first[k];
        set_cuts[k] = set_off[i < n ? i : n];
    }
}

__global__ __launch_bounds__(64) void k_kf_wrap_sizes(const uint64_t* __restrict__ z_off, uint64_t n_members, uint32_t* __restrict__ wsize,
                                                      uint32_t* __restrict__ npiece, uint64_t* __restrict__ w_sums, uint64_t* __restrict__ p_sums,
                                                      uint32_t* __restrict__ err) {
    const uint64_t m = (uint64_t)blockIdx.x * kWave + threadIdx.x;
    uint32_t sz = 0, np = 0;
    if (m < n_members) {
        const uint64_t a = z_off[m], b = z_off[m + 1];
        if (b < a || b - a > kMaxValue) {
            atomicOr(err, 1u);
        } else if (b > a) {
            sz = (uint32_t)wire_size(b - a, false);
            np = (uint32_t)pieces_of(b - a);
        }
        wsize[m] = sz;
        npiece[m] = np;
    }
    uint64_t s0 = sz, s1 = np;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s0 += __shfl_xor(s0, d, kWave);
        s1 += __shfl_xor(s1, d, kWave);
    }
    if (threadIdx.x == 0) {
        w_sums[blockIdx.x] = s0;
        p_sums[blockIdx.x] = s1;
    }
}

// (w is written here and nowhere read; z is only read)
__global__ __launch_bounds__(64) void k_kf_wrap(const uint8_t* __restrict__ z, const uint64_t* __restrict__ z_off, const uint64_t* __restrict__ piece_first,
                                                uint64_t n_members, uint64_t n_pieces, const uint64_t* __restrict__ w_off, uint8_t* __restrict__ w,
                                                uint64_t w_cap, uint32_t* __restrict__ piece_crc) {
    __shared__ uint32_t s_lds[kLdsWords];
    build_tables(s_lds);
    const Lds s = lds_of(s_lds);
    for (uint64_t g = blockIdx.x; g < n_pieces; g += gridDim.x) wrap_piece(z, z_off, piece_first, n_members, g, w_off, w, w_cap, piece_crc, s);
}

__global__ __launch_bounds__(64) void k_kf_wrap_finish(const uint64_t* __restrict__ z_off, const uint64_t* __restrict__ piece_first, uint64_t n_members,
                                                       const uint32_t* __restrict__ piece_crc, const uint64_t* __restrict__ w_off, uint8_t* __restrict__ w,
                                                       uint64_t w_cap) {
    const uint64_t m = (uint64_t)blockIdx.x * kWave + threadIdx.x;
    if (m < n_members) wrap_finish(z_off, piece_first, m, piece_crc, w_off, w, w_cap);
}

}  // namespace kafka
}  // namespace fg

namespace kf = fg::kafka;

extern "C" int fg_launch_encode_scan(const uint32_t* d_sizes, uint64_t* d_block_sums, uint64_t n, uint64_t* d_out_offsets, uint64_t base,
                                     hipStream_t stream);

extern "C" uint32_t fg_kafka_message_overhead(void) { return kf::kOverhead; }
extern "C" uint64_t fg_kafka_bound(uint64_t nbytes, uint64_t n, uint64_t n_members) { return kf::bound(nbytes, n, n_members); }

static uint32_t resident_grid(uint64_t work, int cus) {
    const uint64_t resident = (uint64_t)(cus > 0 ? cus : 1) * kf::kWavesPerCu;
    return (uint32_t)(work < resident ? work : resident);
}

// d_sizes: n u32; d_sums: ceil(n / 64) u64; d_set_offsets: n + 1 u64; *d_err (cleared here) != 0 afterwards: offsets that do not ascend,
// go past nbytes or bound a value whose message does not fit int32.  d_skip: null, or n bytes.  n > 0.
extern "C" int fg_launch_kafka_sizes(const uint64_t* d_off, const uint8_t* d_skip, uint64_t n, uint64_t nbytes, uint32_t* d_sizes, uint64_t* d_sums,
                                     uint64_t* d_set_offsets, uint32_t* d_err, hipStream_t stream) {
    const uint64_t blocks = (n + 63u) / 64u;
    if (blocks > 0x7FFFFFFFull) return -1;
    int rc = (int)hipMemsetAsync(d_err, 0, 4, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(kf::k_kf_sizes, dim3((uint32_t)blocks), dim3(64), 0, stream, d_off, d_skip, n, nbytes, d_sizes, d_sums, d_err);
    rc = (int)hipGetLastError();
    if (rc == 0) rc = fg_launch_encode_scan(d_sizes, d_sums, n, d_set_offsets, 0ull, stream);
    return rc;
}
// the messages into d_set[0 .. set_cap), set_cap >= d_set_offsets[n]; cus = the device's compute units.  n > 0.
extern "C" int fg_launch_kafka_write(const uint8_t* d_bytes, const uint64_t* d_off, const uint8_t* d_skip, uint64_t n, const uint64_t* d_set_offsets,
                                     uint8_t* d_set, uint64_t set_cap, int cus, hipStream_t stream) {
    hipLaunchKernelGGL(kf::k_kf_write, dim3(resident_grid(kf::write_steps(n), cus)), dim3(64), 0, stream, d_bytes, d_off, d_skip, n, d_set_offsets, d_set, set_cap);
    return (int)hipGetLastError();
}
// d_set_cuts[k] = d_set_offsets[d_member_first[k]], k = 0 .. n_members
extern "C" int fg_launch_kafka_cuts(const uint64_t* d_set_offsets, const uint64_t* d_member_first, uint64_t n, uint64_t n_members, uint64_t* d_set_cuts,
                                    hipStream_t stream) {
    const uint64_t blocks = (n_members + 1u + 63u) / 64u;
    if (blocks > 0x7FFFFFFFull) return -1;
    hipLaunchKernelGGL(kf::k_kf_cuts, dim3((uint32_t)blocks), dim3(64), 0, stream, d_set_offsets, d_member_first, n, n_members, d_set_cuts);
    return (int)hipGetLastError();
}
// d_wsize, d_npiece: n_members u32 each; d_sums: 2 * ceil(n_members / 64) u64; d_w_offsets, d_piece_first: n_members + 1 u64 each; *d_err
// (cleared here) != 0 afterwards: offsets that do not ascend or a member whose wrapper does not fit int32.  n_members > 0.
extern "C" int fg_launch_kafka_wrap_sizes(const uint64_t* d_z_offsets, uint64_t n_members, uint32_t* d_wsize, uint32_t* d_npiece, uint64_t* d_sums,
                                          uint64_t* d_w_offsets, uint64_t* d_piece_first, uint32_t* d_err, hipStream_t stream) {
    const uint64_t blocks = (n_members + 63u) / 64u;
    if (blocks > 0x7FFFFFFFull) return -1;
    int rc = (int)hipMemsetAsync(d_err, 0, 4, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(kf::k_kf_wrap_sizes, dim3((uint32_t)blocks), dim3(64), 0, stream, d_z_offsets, n_members, d_wsize, d_npiece, d_sums, d_sums + blocks, d_err);
    rc = (int)hipGetLastError();
    if (rc == 0) rc = fg_launch_encode_scan(d_wsize, d_sums, n_members, d_w_offsets, 0ull, stream);
    if (rc == 0) rc = fg_launch_encode_scan(d_npiece, d_sums + blocks, n_members, d_piece_first, 0ull, stream);
    return rc;
}
// the wrappers into d_w[0 .. w_cap), w_cap >= d_w_offsets[n_members]; d_piece_crc: n_pieces u32.  n_pieces > 0.
extern "C" int fg_launch_kafka_wrap(const uint8_t* d_z, const uint64_t* d_z_offsets, const uint64_t* d_piece_first, uint64_t n_members, uint64_t n_pieces,
                                    const uint64_t* d_w_offsets, uint8_t* d_w, uint64_t w_cap, uint32_t* d_piece_crc, int cus, hipStream_t stream) {
    const uint64_t blocks = (n_members + 63u) / 64u;
    if (blocks > 0x7FFFFFFFull) return -1;
    hipLaunchKernelGGL(kf::k_kf_wrap, dim3(resident_grid(n_pieces, cus)), dim3(64), 0, stream, d_z, d_z_offsets, d_piece_first, n_members, n_pieces, d_w_offsets,
                       d_w, w_cap, d_piece_crc);
    int rc = (int)hipGetLastError();
    if (rc != 0) return rc;
    hipLaunchKernelGGL(kf::k_kf_wrap_finish, dim3((uint32_t)blocks), dim3(64), 0, stream, d_z_offsets, d_piece_first, n_members, d_piece_crc, d_w_offsets, d_w,
                       w_cap);
    return (int)hipGetLastError();
}
