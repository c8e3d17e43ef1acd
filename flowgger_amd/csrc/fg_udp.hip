// fg_udp.hip -- the body of the UDP input on the device: handle_record_maybe_compressed (src/flowgger/input/udp_input.rs:100-143)
// for a batch of datagrams.  Each is a zlib stream, a gzip member or a bare record (the reference's gate); compressed ones are
// inflated, every payload is checked as str::from_utf8 does, and the payloads come out packed (offsets[n + 1]) as everything
// downstream takes them.  The inflater itself is fg_inflate.hpp (HIP-free, the CPU suite runs it); nothing here decides anything
// about a stream.
//
// Inflated sizes are unknown up front, so the shape is the encoders': count, scan, write.
//   k_udp_count    one lane per datagram: the gate, then the symbol stream walked without producing a byte -> the slot's size or a
//                  verdict (malformed, or more than max_inflated).  Per-64-datagram sums for the scan.
//   (scan)         fg_launch_encode_scan of fg_encode.hip: sizes -> d_out_offsets
//   k_udp_write    one lane per datagram: inflate into the slot (back-references read the lane's own earlier bytes in global
//                  memory), Adler-32 / CRC-32 against the trailer
//   k_udp_finish   one wave per 64 datagrams, the whole wave on one datagram at a time: bare records are copied (fg_syslen.hpp's
//                  payload copy, which also judges UTF-8), inflated ones are judged in place
// The one-walk form (fg_udp_unpack_once_device) does not walk a stream twice to learn its size: it guesses.
//   k_udp_stage_sizes  one lane per datagram: the stage its length is given (fg::inflate::stage_capacity, rounded to 16) -> scanned
//                      into stage_off by the same scan
//   k_udp_stage    one lane per datagram: the gate and ONE walk that writes into the lane's stage while the bytes fit it and only
//                  counts from there on -> size, verdict (the trailer's included where everything fitted), `spilled`, sums
//   (scan)         sizes -> d_out_offsets
//   k_udp_write_spilled   k_udp_write for the rows whose bytes did not fit their stage, into their slots
//   k_udp_pack     k_udp_finish with a source per row: the stage for a staged row, the datagram for a bare one, the slot itself for
//                  a spilled one
// One 64-lane wave per workgroup.  The count, stage and write kernels keep every lane's canonical tables in LDS, lane-interleaved:
// 64 * 1020 B = 65 280 B per workgroup, so two waves share a CU's 160 KiB -- the streams are serial, what hides latency is the
// other 63 lanes.  No loop waits on another wave: every one consumes input bits or produces output bytes, both bounded.
#include <hip/hip_runtime.h>

#include "fg_inflate.hpp"
#include "fg_syslen.hpp"

namespace fg {
namespace udp {

namespace inf = fg::inflate;
constexpr uint32_t kWave = 64;

__global__ __launch_bounds__(64) void k_udp_count(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                                                  uint32_t max_inflated, uint32_t* __restrict__ sizes, uint8_t* __restrict__ status,
                                                  uint8_t* __restrict__ drop, uint64_t* __restrict__ block_sums) {
    __shared__ uint16_t s_h[inf::kHalfWords * kWave];
    __shared__ uint8_t s_b[inf::kLenBytes * kWave];
    const uint64_t li = (uint64_t)blockIdx.x * kWave + threadIdx.x;
    uint32_t size = 0;
    if (li < n) {
        const inf::Tabs t{s_h + threadIdx.x, s_b + threadIdx.x, kWave};
        const uint64_t a = offsets[li], b = offsets[li + 1];
        const uint32_t st = inf::count_datagram(bytes + a, b - a, max_inflated, t, &size);
        sizes[li] = size;
        status[li] = (uint8_t)st;
        drop[li] = st > inf::UDP_GZIP ? 1 : 0;
    }
    uint64_t sum = size;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, kWave);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = sum;
}

// The write walk of one lane.  only: null, or one byte per datagram -- zero: not this launch's row.  (out is read back by the lane that
// wrote it: no __restrict__ on it)
static __device__ __forceinline__ void write_row(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                                                 const uint64_t* __restrict__ out_offsets, uint8_t* out, uint64_t out_cap, uint8_t* __restrict__ status,
                                                 uint8_t* __restrict__ drop, const uint8_t* __restrict__ only, uint16_t* s_h, uint8_t* s_b) {
    const uint64_t li = (uint64_t)blockIdx.x * kWave + threadIdx.x;
    if (li >= n) return;
    if (only && only[li] == 0) return;
    const uint32_t st = status[li];
    if (st == inf::UDP_RAW) return;
    const uint64_t o0 = out_offsets[li], o1 = out_offsets[li + 1];
    if (o1 > out_cap || o1 < o0 || o1 - o0 > 0x7FFFFFFFull) return;  // (never: the caller compared the total with out_cap)
    const inf::Tabs t{s_h + threadIdx.x, s_b + threadIdx.x, kWave};
    const uint64_t a = offsets[li], b = offsets[li + 1];
    const uint32_t st2 = inf::write_datagram(bytes + a, b - a, st, (uint32_t)(o1 - o0), t, out + o0);
    if (st2 != st) {
        status[li] = (uint8_t)st2;
        drop[li] = 1;
    }
}

__global__ __launch_bounds__(64) void k_udp_write(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                                                  const uint64_t* __restrict__ out_offsets, uint8_t* out, uint64_t out_cap,
                                                  uint8_t* __restrict__ status, uint8_t* __restrict__ drop) {
    __shared__ uint16_t s_h[inf::kHalfWords * kWave];
    __shared__ uint8_t s_b[inf::kLenBytes * kWave];
    write_row(bytes, offsets, n, out_offsets, out, out_cap, status, drop, nullptr, s_h, s_b);
}

// ... for the rows of the one-walk form that outgrew their stage (spilled[i] != 0)
__global__ __launch_bounds__(64) void k_udp_write_spilled(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                                                          const uint64_t* __restrict__ out_offsets, uint8_t* out, uint64_t out_cap,
                                                          uint8_t* __restrict__ status, uint8_t* __restrict__ drop,
                                                          const uint8_t* __restrict__ spilled) {
    __shared__ uint16_t s_h[inf::kHalfWords * kWave];
    __shared__ uint8_t s_b[inf::kLenBytes * kWave];
    write_row(bytes, offsets, n, out_offsets, out, out_cap, status, drop, spilled, s_h, s_b);
}

// The stage every datagram is given, rounded up to 16 bytes so that the stages start aligned, and the per-64 sums for the scan.
// (Thread 0 also clears the word k_udp_stage counts the spilled rows in: it runs behind this kernel on the same stream.)
__global__ __launch_bounds__(64) void k_udp_stage_sizes(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                                                        uint32_t max_inflated, uint32_t* __restrict__ stage_sizes, uint64_t* __restrict__ block_sums,
                                                        uint32_t* __restrict__ n_spilled) {
    const uint64_t li = (uint64_t)blockIdx.x * kWave + threadIdx.x;
    uint32_t w = 0;
    if (li < n) {
        const uint64_t a = offsets[li], b = offsets[li + 1];
        w = (inf::stage_capacity(bytes + a, b - a, max_inflated) + 15u) & ~15u;
        stage_sizes[li] = w;
    }
    uint64_t sum = w;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, kWave);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = sum;
    if (li == 0) *n_spilled = 0u;
}

// One walk per datagram.  A lane stores stream bytes only inside stage[stage_off[li] .. + its capacity): stage_datagram writes no
// piece that would end beyond the capacity it is handed, and that capacity is cut to what the scan gave the lane and to stage_cap.
// (stage is read back by the lane that wrote it: no __restrict__ on it)
__global__ __launch_bounds__(64) void k_udp_stage(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                                                  uint32_t max_inflated, const uint64_t* __restrict__ stage_off, uint8_t* stage, uint64_t stage_cap,
                                                  uint32_t* __restrict__ sizes, uint8_t* __restrict__ status, uint8_t* __restrict__ drop,
                                                  uint8_t* __restrict__ spilled, uint64_t* __restrict__ block_sums, uint32_t* __restrict__ n_spilled) {
    __shared__ uint16_t s_h[inf::kHalfWords * kWave];
    __shared__ uint8_t s_b[inf::kLenBytes * kWave];
    const uint64_t li = (uint64_t)blockIdx.x * kWave + threadIdx.x;
    uint32_t size = 0, sp = 0;
    if (li < n) {
        const inf::Tabs t{s_h + threadIdx.x, s_b + threadIdx.x, kWave};
        const uint64_t a = offsets[li], b = offsets[li + 1];
        const uint64_t s0 = stage_off[li], s1 = stage_off[li + 1];
        uint32_t w = inf::stage_capacity(bytes + a, b - a, max_inflated);
        if (s1 > stage_cap || s1 < s0 || s1 - s0 < w) w = 0u;  // (never: the offsets are the scan of these capacities; without a stage every row spills)
        const uint32_t st = inf::stage_datagram(bytes + a, b - a, max_inflated, w, t, stage + (w ? s0 : 0ull), &size, &sp);
        sizes[li] = size;
        status[li] = (uint8_t)st;
        drop[li] = st > inf::UDP_GZIP ? 1 : 0;
        spilled[li] = (uint8_t)sp;
    }
    uint64_t sum = size;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, kWave);
    if (threadIdx.x == 0) block_sums[blockIdx.x] = sum;
    const uint32_t cnt = (uint32_t)__popcll(__ballot(sp != 0u));
    if (threadIdx.x == 0 && cnt) atomicAdd(n_spilled, cnt);
}

// whether src[0 .. len) is NOT valid UTF-8, by the whole wave (to every lane that saw an offence); the rule of fg_utf8.hpp
FG_WV bool utf8_bad(const uint8_t* src, uint32_t len) {
    const uint32_t l = wv::lane();
    bool bad = false;
    for (uint32_t i = l * 16u; i <= len; i += wv::kLanes * 16u) {  // (<=: the lane behind the last byte sees a sequence cut off there)
        const uint32_t nb = len - i >= 16u ? 16u : len - i;
        uint32_t q[4] = {0u, 0u, 0u, 0u};
        if (nb == 16u) {
            fg::syslen::load16u(src + i, q);
        } else {
            for (uint32_t k = 0; k < nb; ++k) q[k >> 2] |= (uint32_t)src[i + k] << (8u * (k & 3u));
        }
        const uint32_t before = i >= 1u ? src[i - 1u] : 0u;
        if (((q[0] | q[1] | q[2] | q[3]) & 0x80808080u) | (before & 0x80u)) {
            uint32_t p1 = before, p2 = i >= 2u ? src[i - 2u] : 0u, p3 = i >= 3u ? src[i - 3u] : 0u;
            const uint32_t upto = nb < 16u ? nb + 1u : (i + 16u == len ? 17u : 16u);  // position len itself (when len is a multiple of 16 the next lane, with nb == 0, judges it again: same verdict)
            for (uint32_t k = 0; k < upto; ++k) {
                const uint32_t b = k < nb ? (q[k >> 2] >> (8u * (k & 3u))) & 0xFFu : 0u;
                bad |= fg::utf8::err_at(b, p1, p2, p3);
                p3 = p2; p2 = p1; p1 = b;
            }
        }
    }
    return bad;
}

// The last step for the 64 datagrams of one wave, the whole wave on one datagram at a time.  PACK = false: bare records are copied,
// inflated payloads judged where the write walk left them.  PACK = true (the one-walk form): a row that is not spilled and not
// bare is copied from its stage -- judged on the way when it is kept, only copied when a wrong checksum dropped it with its bytes.
template <bool PACK>
static __device__ __forceinline__ void finish_rows(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                                                   const uint64_t* __restrict__ out_offsets, uint8_t* out, uint64_t out_cap, uint8_t* status, uint8_t* drop,
                                                   const uint8_t* __restrict__ stage, const uint64_t* __restrict__ stage_off, uint64_t stage_cap,
                                                   const uint8_t* __restrict__ spilled) {
    const uint64_t base = (uint64_t)blockIdx.x * kWave;
    for (uint32_t j = 0; j < kWave; ++j) {
        const uint64_t i = base + j;
        if (i >= n) break;  // (wave-uniform)
        const uint32_t st = status[i];
        const bool staged = PACK && st != inf::UDP_RAW && spilled[i] == 0;
        if (st > inf::UDP_GZIP && !staged) continue;
        const uint64_t o0 = out_offsets[i], o1 = out_offsets[i + 1];
        if (o1 > out_cap || o1 < o0 || o1 - o0 > 0x7FFFFFFFull) continue;  // (never, as in k_udp_write)
        const uint32_t len = (uint32_t)(o1 - o0);
        bool bad;
        if (st == inf::UDP_RAW) {
            if (offsets[i + 1] - offsets[i] != len) continue;  // (never: a bare record's slot is its length)
            bad = fg::syslen::copy_check(bytes + offsets[i], out + o0, len);
        } else if (staged) {
            if (len == 0u) continue;
            const uint64_t s0 = stage_off[i], s1 = stage_off[i + 1];
            if (s1 > stage_cap || s1 < s0 || s1 - s0 < len) continue;  // (never: a row that did not spill lies in its stage)
            bad = fg::syslen::copy_check(stage + s0, out + o0, len) && st <= inf::UDP_GZIP;
        } else {
            bad = utf8_bad(out + o0, len);
        }
        if (bad) {  // (every lane that saw an offence stores the same two bytes)
            status[i] = (uint8_t)inf::UDP_BAD_UTF8;
            drop[i] = 1;
        }
    }
}

__global__ __launch_bounds__(64) void k_udp_finish(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                                                   const uint64_t* __restrict__ out_offsets, uint8_t* out, uint64_t out_cap,
                                                   uint8_t* status, uint8_t* drop) {
    finish_rows<false>(bytes, offsets, n, out_offsets, out, out_cap, status, drop, nullptr, nullptr, 0ull, nullptr);
}

__global__ __launch_bounds__(64) void k_udp_pack(const uint8_t* __restrict__ bytes, const uint64_t* __restrict__ offsets, uint64_t n,
                                                 const uint64_t* __restrict__ out_offsets, uint8_t* out, uint64_t out_cap, uint8_t* status,
                                                 uint8_t* drop, const uint8_t* __restrict__ stage, const uint64_t* __restrict__ stage_off,
                                                 uint64_t stage_cap, const uint8_t* __restrict__ spilled) {
    finish_rows<true>(bytes, offsets, n, out_offsets, out, out_cap, status, drop, stage, stage_off, stage_cap, spilled);
}

}  // namespace udp
}  // namespace fg

// d_sizes: n u32; d_block_sums: ceil(n / 64) u64.  max_inflated < 2^31 - 1.
extern "C" int fg_launch_udp_count(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint32_t max_inflated, uint32_t* d_sizes,
                                   uint64_t* d_block_sums, uint8_t* d_status, uint8_t* d_drop, hipStream_t stream) {
    if (n == 0) return 0;
    const uint64_t blocks = (n + 63u) / 64u;
    if (blocks > 0x7FFFFFFFull || max_inflated >= 0x7FFFFFFEu) return -1;
    hipLaunchKernelGGL(fg::udp::k_udp_count, dim3((uint32_t)blocks), dim3(64), 0, stream, d_bytes, d_offsets, n, max_inflated, d_sizes, d_status, d_drop,
                       d_block_sums);
    return (int)hipGetLastError();
}
// after the scan: inflate into the slots and settle the checksums ...
extern "C" int fg_launch_udp_write(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_out_offsets, uint8_t* d_out,
                                   uint64_t out_cap, uint8_t* d_status, uint8_t* d_drop, hipStream_t stream) {
    if (n == 0) return 0;
    const uint64_t blocks = (n + 63u) / 64u;
    if (blocks > 0x7FFFFFFFull) return -1;
    hipLaunchKernelGGL(fg::udp::k_udp_write, dim3((uint32_t)blocks), dim3(64), 0, stream, d_bytes, d_offsets, n, d_out_offsets, d_out, out_cap, d_status, d_drop);
    return (int)hipGetLastError();
}
// ... then copy the bare records and judge every kept payload's UTF-8
extern "C" int fg_launch_udp_finish(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_out_offsets, uint8_t* d_out,
                                    uint64_t out_cap, uint8_t* d_status, uint8_t* d_drop, hipStream_t stream) {
    if (n == 0) return 0;
    const uint64_t blocks = (n + 63u) / 64u;
    if (blocks > 0x7FFFFFFFull) return -1;
    hipLaunchKernelGGL(fg::udp::k_udp_finish, dim3((uint32_t)blocks), dim3(64), 0, stream, d_bytes, d_offsets, n, d_out_offsets, d_out, out_cap, d_status,
                       d_drop);
    return (int)hipGetLastError();
}

extern "C" int fg_launch_encode_scan(const uint32_t* d_sizes, uint64_t* d_block_sums, uint64_t n, uint64_t* d_out_offsets, uint64_t base,
                                     hipStream_t stream);
// The one-walk form.  The front: every datagram staged in d_stage[0 .. stage_cap) (stage_cap >= fg_udp_stage_bytes(nbytes, n)), its
// size, verdict and `spilled` flag, d_out_offsets[0 .. n] = the scan of the sizes, *d_n_spilled = the spilled rows.  d_stage_sizes,
// d_sizes: n u32 each; d_stage_sums, d_block_sums: ceil(n / 64) u64 each; d_stage_off: n + 1 u64.  max_inflated < 2^31 - 1.
extern "C" uint64_t fg_udp_stage_bytes(uint64_t nbytes, uint64_t n) {  // (no stage is larger than K * len + C rounded up twice)
    return (uint64_t)fg::inflate::kStageK * nbytes + n * (uint64_t)(fg::inflate::kStageC + 32u) + 16u;
}
extern "C" int fg_launch_udp_stage(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, uint32_t max_inflated, uint32_t* d_stage_sizes,
                                   uint64_t* d_stage_sums, uint64_t* d_stage_off, uint8_t* d_stage, uint64_t stage_cap, uint32_t* d_sizes,
                                   uint64_t* d_block_sums, uint64_t* d_out_offsets, uint8_t* d_status, uint8_t* d_drop, uint8_t* d_spilled,
                                   uint32_t* d_n_spilled, hipStream_t stream) {
    if (n == 0) return 0;
    const uint64_t blocks = (n + 63u) / 64u;
    if (blocks > 0x7FFFFFFFull || max_inflated >= 0x7FFFFFFEu) return -1;
    hipLaunchKernelGGL(fg::udp::k_udp_stage_sizes, dim3((uint32_t)blocks), dim3(64), 0, stream, d_bytes, d_offsets, n, max_inflated, d_stage_sizes,
                       d_stage_sums, d_n_spilled);
    int rc = (int)hipGetLastError();
    if (rc == 0) rc = fg_launch_encode_scan(d_stage_sizes, d_stage_sums, n, d_stage_off, 0ull, stream);
    if (rc != 0) return rc;
    hipLaunchKernelGGL(fg::udp::k_udp_stage, dim3((uint32_t)blocks), dim3(64), 0, stream, d_bytes, d_offsets, n, max_inflated, d_stage_off, d_stage, stage_cap,
                       d_sizes, d_status, d_drop, d_spilled, d_block_sums, d_n_spilled);
    rc = (int)hipGetLastError();
    if (rc == 0) rc = fg_launch_encode_scan(d_sizes, d_block_sums, n, d_out_offsets, 0ull, stream);
    return rc;
}
// ... the write walk for the spilled rows (launched only when there are any) ...
extern "C" int fg_launch_udp_write_spilled(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_out_offsets, uint8_t* d_out,
                                           uint64_t out_cap, uint8_t* d_status, uint8_t* d_drop, const uint8_t* d_spilled, hipStream_t stream) {
    if (n == 0) return 0;
    const uint64_t blocks = (n + 63u) / 64u;
    if (blocks > 0x7FFFFFFFull) return -1;
    hipLaunchKernelGGL(fg::udp::k_udp_write_spilled, dim3((uint32_t)blocks), dim3(64), 0, stream, d_bytes, d_offsets, n, d_out_offsets, d_out, out_cap,
                       d_status, d_drop, d_spilled);
    return (int)hipGetLastError();
}
// ... then every other row into its slot, and every kept payload's UTF-8
extern "C" int fg_launch_udp_pack(const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_out_offsets, uint8_t* d_out,
                                  uint64_t out_cap, uint8_t* d_status, uint8_t* d_drop, const uint8_t* d_stage, const uint64_t* d_stage_off,
                                  uint64_t stage_cap, const uint8_t* d_spilled, hipStream_t stream) {
    if (n == 0) return 0;
    const uint64_t blocks = (n + 63u) / 64u;
    if (blocks > 0x7FFFFFFFull) return -1;
    hipLaunchKernelGGL(fg::udp::k_udp_pack, dim3((uint32_t)blocks), dim3(64), 0, stream, d_bytes, d_offsets, n, d_out_offsets, d_out, out_cap, d_status, d_drop,
                       d_stage, d_stage_off, stage_cap, d_spilled);
    return (int)hipGetLastError();
}
