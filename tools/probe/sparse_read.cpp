// tools/probe/sparse_read.cpp -- what HBM delivers when the headline kernel's register window leaves lanes out.
// Every wave issues the window's loads as k_rfc5424 does -- raw buffer loads of 16 B per lane, 1 KiB per instruction, NB = 20 per
// group, nt -- over a buffer of 4 GiB, persistent grid, eight waves per CU (20 KiB of LDS per wave, nothing staged).  The loads
// are UNCONDITIONAL: a lane whose 16-byte chunk is not wanted gets an offset beyond the descriptor's range, fetches nothing and
// returns zeros (what load_window relies on for rows past the span).  Wanted = the chunk overlaps [s, s + KEEP) of a period of
// 254 bytes: a line's last two bytes and the head of the next, lines packed back to back.  KEEP = 0 is the dense window.
// Printed per pattern and phase: ms, GB/s of the bytes requested, GB/s of the buffer swept, and the bytes per period that fetch
// granules of 16 / 32 / 64 / 128 B would move (to set against FETCH_SIZE: tools/prof_sparse_read.sh).
// build: hipcc --offload-arch=gfx950 -O3 -o tools/probe/sparse_read tools/probe/sparse_read.cpp
// usage: sparse_read [GiB = 4] [reps = 4]
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define CHECK(x)                                                                  \
    do {                                                                          \
        hipError_t e_ = (x);                                                      \
        if (e_ != hipSuccess) {                                                   \
            fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_));               \
            exit(1);                                                              \
        }                                                                         \
    } while (0)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kPeriod = 254;   // bytes per line of the bench corpus
constexpr int kNB = 20;             // window loads per group
constexpr uint32_t kGroup = kNB * 1024u;
constexpr uint32_t kOut = 0x80000000u;  // beyond every descriptor's range, and kOut + k * 1024 does not wrap back into it

// chunk [b, b + 16) overlaps [s + i * kPeriod, s + i * kPeriod + keep) for some i  (keep + 15 <= kPeriod)
__host__ __device__ inline bool wanted(uint64_t b, uint32_t s, uint32_t keep) {
    return (uint32_t)((b + 15u + kPeriod - s) % kPeriod) < keep + 15u;
}

// SOFF: the row's KiB in the SCALAR offset (which the range check does not see) and the lane's 16 bytes alone in the voffset, bit 31
// set for a lane that is taken out -- the form the kernel uses; else the whole offset in the voffset, kOut for such a lane.
template <uint32_t KEEP, bool SOFF = false>
__global__ __launch_bounds__(64) void k_read(const uint8_t* __restrict__ buf, uint64_t groups, uint32_t s, uint32_t* __restrict__ sink) {
    const uint32_t lane = threadIdx.x;
    u32x4 acc = {0u, 0u, 0u, 0u};
    for (uint64_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const uint64_t a0 = g * kGroup;
        __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(buf + a0), (short)0, (int)kGroup, 0x00020000);
        // (a0 + 15 + kPeriod - s) mod kPeriod once per group, as a scalar; the lanes go on in 32 bits
        const uint32_t m0 = (uint32_t)((a0 + 15u + kPeriod - s) % kPeriod);
        u32x4 v[kNB];
#pragma unroll
        for (int k = 0; k < kNB; ++k) {
            const uint32_t off = lane * 16u + (uint32_t)k * 1024u;
            const bool need = KEEP == 0u || (m0 + off) % kPeriod < KEEP + 15u;
            if (SOFF) v[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(lane * 16u | (need ? 0u : kOut)), k * 1024, 2 /* nt */);
            else v[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, (int)(need ? off : kOut), 0, 2 /* nt */);
        }
        __builtin_amdgcn_sched_barrier(0);  // the whole window in flight before its first register is read
#pragma unroll
        for (int k = 0; k < kNB; ++k) acc ^= v[k];
    }
    if ((acc[0] ^ acc[1] ^ acc[2] ^ acc[3]) == 0x12345678u) sink[0] = 1u;  // (keeps the loads alive; the buffer holds zeros)
}

template <uint32_t KEEP, bool SOFF = false>
static float run(const uint8_t* buf, uint64_t groups, uint32_t s, uint32_t* sink, uint32_t blocks, int reps, hipEvent_t e0, hipEvent_t e1) {
    float best = 1e9f;
    for (int rep = 0; rep < reps; ++rep) {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL((k_read<KEEP, SOFF>), dim3(blocks), dim3(64), kGroup, 0, buf, groups, s, sink);
        CHECK(hipGetLastError());
        CHECK(hipEventRecord(e1));
        CHECK(hipEventSynchronize(e1));
        float ms;
        CHECK(hipEventElapsedTime(&ms, e0, e1));
        if ((rep || reps == 1) && ms < best) best = ms;
    }
    return best;
}

// bytes per period moved by fetch granules of `gran` bytes when the wanted 16-byte chunks are requested (over lcm(254, 128) bytes)
static double granule_bytes(uint32_t s, uint32_t keep, uint32_t gran) {
    const uint64_t span = 16256;  // 64 periods = 127 lines of 128 B
    uint64_t hit = 0;
    for (uint64_t g0 = 0; g0 < span; g0 += gran) {
        bool any = false;
        for (uint64_t b = g0; b < g0 + gran; b += 16u) any = any || keep == 0u || wanted(b, s, keep);
        hit += any ? gran : 0u;
    }
    return (double)hit / 64.0;
}

int main(int argc, char** argv) {
    alarm(240);  // a hung launch ends the program
    const uint64_t gib = argc > 1 ? strtoull(argv[1], nullptr, 10) : 4ull;
    const int reps = argc > 2 ? atoi(argv[2]) : 4;
    const uint64_t bytes = (gib << 30) / kGroup * kGroup;
    const uint64_t groups = bytes / kGroup;
    uint8_t* buf;
    uint32_t* sink;
    CHECK(hipMalloc(&buf, bytes));
    CHECK(hipMalloc(&sink, 64));
    CHECK(hipMemset(buf, 0, bytes));
    CHECK(hipMemset(sink, 0, 64));
    hipDeviceProp_t prop;
    CHECK(hipGetDeviceProperties(&prop, 0));
    CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(k_read<0>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGroup));
    const uint32_t blocks = (uint32_t)prop.multiProcessorCount * 8u;
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0));
    CHECK(hipEventCreate(&e1));
    printf("%.2f GiB swept, %u waves (8 per CU), %d loads of 1 KiB per group, period %u\n", bytes / 1073741824.0, blocks, kNB, kPeriod);
    printf("%5s %5s %9s %10s %10s   bytes per period at granule 16 / 32 / 64 / 128 B\n", "keep", "phase", "ms", "req GB/s", "swept GB/s");
    const uint32_t keeps[6] = {0u, 96u, 112u, 128u, 0u, 97u};  // (97: 96 kept, the row in the scalar offset)
    const uint32_t phases[3] = {0u, 5u, 13u};
    for (int ki = 0; ki < 6; ++ki) {
        const uint32_t keep = keeps[ki];
        for (int pi = 0; pi < (keep ? 3 : 1); ++pi) {
            const uint32_t s = phases[pi];
            float ms;
            if (keep == 97u) {
                ms = run<96, true>(buf, groups, s, sink, blocks, reps, e0, e1);
                const double req = granule_bytes(s, 96u, 16u) / kPeriod * (double)bytes;
                printf("%5s %5u %9.3f %10.1f %10.1f   (96 kept, the row in the scalar offset)\n", "96s", s, ms, req / (ms * 1e-3) / 1e9, bytes / (ms * 1e-3) / 1e9);
                continue;
            }
            switch (keep) {
                case 0: ms = run<0>(buf, groups, s, sink, blocks, reps, e0, e1); break;
                case 96: ms = run<96>(buf, groups, s, sink, blocks, reps, e0, e1); break;
                case 112: ms = run<112>(buf, groups, s, sink, blocks, reps, e0, e1); break;
                default: ms = run<128>(buf, groups, s, sink, blocks, reps, e0, e1); break;
            }
            const double req = granule_bytes(s, keep, 16u) / kPeriod * (double)bytes;
            printf("%5u %5u %9.3f %10.1f %10.1f   %.1f / %.1f / %.1f / %.1f\n", keep, s, ms, req / (ms * 1e-3) / 1e9, bytes / (ms * 1e-3) / 1e9,
                   granule_bytes(s, keep, 16u), granule_bytes(s, keep, 32u), granule_bytes(s, keep, 64u), granule_bytes(s, keep, 128u));
        }
    }
    uint32_t h = 0;
    CHECK(hipMemcpy(&h, sink, 4, hipMemcpyDeviceToHost));
    return h ? 2 : 0;
}
