// fg_host_pipeline.cpp -- the PCIe-inclusive HOST-BUFFER entry points of the C ABI (include/fg_hip.h): fg_decode_batch,
// fg_frame_decode_batch, fg_transcode_batch, the pinned allocator and fg_measure_link.  Everything here is copies, streams, events and
// calls of the device entry points (fg_capi.cpp); no kernel and no launch geometry lives in this file, so editing it does not change
// what a kernel does (flowgger_amd/build.py source_hash: measured HBM traffic is keyed on the kernels' own sources).
// Replaces the per-line `decoder.decode(line)` -> `encoder.encode(..)` -> `tx.send(..)` of handle_line for a whole batch
// (src/flowgger/splitter/line_splitter.rs:44-54).
#include <cstddef>

#include "fg_ctx.hpp"
#include "fg_syslen_parse.hpp"
#include "fg_capnp_next.hpp"

extern "C" {

// ---- the batch buffers' allocator: page-locked memory through a process-wide POOL (a framer pinned max_bytes + 1 MiB per
// run(), i.e. per connection -- a thread-per-connection server with hundreds of clients pinned gigabytes and paid milliseconds of
// pin / unpin per connect).  A freed block is kept (up to `idle_limit` bytes in total) and handed to the next request it fits; the
// bytes pinned through this allocator are capped (`limit`): beyond the cap a request gets PAGEABLE memory -- fg_decode_batch and the
// raw-stream paths take either (pinned: zero-copy / link-speed uploads; pageable: the runtime's staged copies).
}  // extern "C"
#include <map>
#include <mutex>
namespace {
struct PinnedPool {
    std::mutex mu;
    std::map<void*, std::pair<uint64_t, bool>> live;  // block -> (capacity, pinned?)
    std::multimap<uint64_t, void*> idle;              // pinned blocks nobody holds, by capacity
    uint64_t pinned_bytes = 0, idle_bytes = 0;
    uint64_t limit = 8ull << 30, idle_limit = 256ull << 20;
};
PinnedPool& pinned_pool() {
    static PinnedPool* p = new PinnedPool();  // (never destroyed: no HIP calls from static destructors at process exit)
    return *p;
}
}  // namespace
extern "C" {

int fg_alloc_pinned(uint64_t bytes, void** out) {
    if (!out) return FG_ERR_ARG;
    *out = nullptr;
    const uint64_t need = up(bytes ? bytes : 1, 64u << 10);
    PinnedPool& P = pinned_pool();
    std::vector<void*> evict;  // idle blocks to unpin, once the lock is released
    bool pageable = false;
    {
        std::lock_guard<std::mutex> g(P.mu);
        auto it = P.idle.lower_bound(need);
        if (it != P.idle.end() && it->first <= 2u * need + (1u << 20)) {  // (a block of at most twice the size: no 64 MiB block for a 64 KiB request)
            void* p = it->second;
            const uint64_t cap = it->first;
            P.idle.erase(it);
            P.idle_bytes -= cap;
            P.live[p] = {cap, true};
            *out = p;
            return FG_OK;
        }
        if (P.pinned_bytes + need > P.limit) {
            // over the cap: what is idle goes first (unpinned BEHIND the lock: hipHostFree is a millisecond-scale call, and every connection
            // thread's alloc / free waits on this mutex -- ADVICE r5), then pageable memory
            while (!P.idle.empty() && P.pinned_bytes + need > P.limit) {
                auto last = std::prev(P.idle.end());
                evict.push_back(last->second);
                P.pinned_bytes -= last->first;
                P.idle_bytes -= last->first;
                P.idle.erase(last);
            }
            if (P.pinned_bytes + need > P.limit) {
                void* p = aligned_alloc(4096, (size_t)need);
                if (p) {
                    P.live[p] = {need, false};
                    *out = p;
                }
                pageable = true;
            }
        }
        if (!pageable) P.pinned_bytes += need;  // (reserved before the slow call, outside the lock)
    }
    for (void* e : evict) (void)hipHostFree(e);
    if (pageable) return *out ? FG_OK : FG_ERR_NOMEM;
    void* p = nullptr;
    if (hipHostMalloc(&p, need, hipHostMallocDefault) != hipSuccess || !p) {
        (void)hipGetLastError();
        std::lock_guard<std::mutex> g(P.mu);
        P.pinned_bytes -= need;
        return FG_ERR_HIP;
    }
    std::lock_guard<std::mutex> g(P.mu);
    P.live[p] = {need, true};
    *out = p;
    return FG_OK;
}
void fg_free_pinned(void* p) {
    if (!p) return;
    PinnedPool& P = pinned_pool();
    bool unpin = false;
    {
        std::lock_guard<std::mutex> g(P.mu);
        auto it = P.live.find(p);
        if (it == P.live.end()) return;  // (not ours)
        const uint64_t cap = it->second.first;
        const bool pinned = it->second.second;
        P.live.erase(it);
        if (!pinned) {
            free(p);
            return;
        }
        if (P.idle_bytes + cap <= P.idle_limit) {
            P.idle.emplace(cap, p);
            P.idle_bytes += cap;
        } else {
            P.pinned_bytes -= cap;
            unpin = true;
        }
    }
    if (unpin) (void)hipHostFree(p);
}
int fg_set_pinned_limits(uint64_t total_bytes, uint64_t idle_bytes) {
    PinnedPool& P = pinned_pool();
    std::vector<void*> evict;
    {
        std::lock_guard<std::mutex> g(P.mu);
        P.limit = total_bytes;
        P.idle_limit = idle_bytes;
        while (!P.idle.empty() && P.idle_bytes > P.idle_limit) {
            auto last = std::prev(P.idle.end());
            evict.push_back(last->second);
            P.pinned_bytes -= last->first;
            P.idle_bytes -= last->first;
            P.idle.erase(last);
        }
    }
    for (void* e : evict) (void)hipHostFree(e);  // (behind the lock)
    return FG_OK;
}
// 1: p is a block of this allocator that is page-locked; 0: one that fell back to pageable memory (the cap was reached: zero-copy and
// link-speed uploads do not apply to it); -1: not a block of this allocator
int fg_is_pinned(const void* p) {
    PinnedPool& P = pinned_pool();
    std::lock_guard<std::mutex> g(P.mu);
    auto it = P.live.find(const_cast<void*>(p));
    return it == P.live.end() ? -1 : it->second.second ? 1 : 0;
}
int fg_pinned_stats(uint64_t* pinned_bytes, uint64_t* idle_bytes, uint64_t* live_blocks) {
    PinnedPool& P = pinned_pool();
    std::lock_guard<std::mutex> g(P.mu);
    if (pinned_bytes) *pinned_bytes = P.pinned_bytes;
    if (idle_bytes) *idle_bytes = P.idle_bytes;
    if (live_blocks) *live_blocks = P.live.size();
    return FG_OK;
}

// Streams and events of the pipelined host paths (created on first use).  Three roles, each its own stream, chained by events per slice:
//   s_run  = the ctx's OWN stream (the first one it created): kernels, and the 8-byte counter copies that follow them
//   s_up   = stream2: every host -> device copy, back to back, nothing else ever queued between two of them
//   s_down = stream3: every device -> host copy of table columns
// so that the link carries both directions at once.  (Round 2 alternated whole slices -- H2D, kernel, D2H -- between two streams:
// measured, that gave the rate of NO overlap at all, 42 of 57 GB/s.)  One platform observation decides an ORDER below (MI355X /
// ROCm 7.2, tools/probe/stream_pairs.cpp and four orderings of this code): the runtime binds its copy paths to streams as they first
// copy, and with stream2 / stream3 as the first streams of the process to copy, fg_decode_batch ran at 160 M lines/s; with the ctx's
// own stream having copied a few bytes each way BEFORE them, at 198 M (the figure DESIGN.md quotes belongs to this ordering).  Hence
// the probe copy on ctx->stream.  fg_measure_link times its copies on s_up / s_down as assigned here.
static int ensure_pipeline(fg_ctx* ctx, uint32_t slices) {
    if (!ctx->stream2) FG_HIP(ctx, hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
    if (!ctx->ev_ready) FG_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_ready, hipEventDisableTiming));  // (its own check: a failed create is retried)
    if (!ctx->stream3) FG_HIP(ctx, hipStreamCreateWithFlags(&ctx->stream3, hipStreamNonBlocking));
    while (ctx->ev_slice.size() < 2ull * slices) {
        hipEvent_t e = nullptr;
        FG_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        ctx->ev_slice.push_back(e);
    }
    if (!ctx->s_up) {
        // (see above: the ctx's own stream copies a few bytes each way before stream2 / stream3 are ever used)
        uint64_t probe = 0;
        uint64_t* d_probe = nullptr;
        FG_HIP(ctx, hipMalloc((void**)&d_probe, 8));
        (void)hipMemcpyAsync(d_probe, &probe, 8, hipMemcpyHostToDevice, ctx->stream);
        (void)hipMemcpyAsync(&probe, d_probe, 8, hipMemcpyDeviceToHost, ctx->stream);
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(d_probe);
    }
    ctx->s_up = ctx->stream2;
    ctx->s_run = ctx->stream;
    ctx->s_down = ctx->stream3;
    return FG_OK;
}
// wait for everything a pipelined call has queued, on all three streams whatever the first of them reports: -> the first error
static hipError_t drain(fg_ctx* ctx) {
    hipError_t first = ctx->s_up ? hipStreamSynchronize(ctx->s_up) : hipSuccess;
    const hipError_t run = hipStreamSynchronize(ctx->stream);  // (s_run, and the one stream of a batch too small to be sliced)
    const hipError_t down = ctx->s_down ? hipStreamSynchronize(ctx->s_down) : hipSuccess;
    if (first == hipSuccess) first = run;
    return first != hipSuccess ? first : down;
}
// the bytes of a slice: a `parts`-th of the batch, 8 MiB at least, 32 MiB at most
static uint64_t slice_bytes(uint64_t nbytes, uint32_t parts) { return std::min<uint64_t>(std::max<uint64_t>(nbytes / parts, 8ull << 20), 32ull << 20); }
// slices of a host batch: small enough that filling and draining the pipeline costs little (1/8 of the batch at most), large
// enough that a slice's fourteen API calls stay far below its transfer time
static uint32_t slice_count(uint64_t nbytes, uint64_t n) {
    if (nbytes < (32ull << 20)) return 1;  // small batches: one stream, no events (a batch of one line costs what it did)
    const uint64_t slice = slice_bytes(nbytes, 8);
    uint64_t k = (nbytes + slice - 1) / slice;
    if (k < 1) k = 1;
    if (k > kMaxDecodeSlices) k = kMaxDecodeSlices;
    if (n < k) k = n ? n : 1;
    return (uint32_t)k;
}

int fg_measure_link(fg_ctx* ctx, uint64_t nbytes, double gbps[3]) {
    if (!ctx || !gbps || nbytes < 4096) return FG_ERR_ARG;
    DeviceGuard g(ctx->device);
    {   // on the very streams the pipelined host paths copy on: uploads on s_up (stream2), downloads on s_down (stream3)
        const int prc = ensure_pipeline(ctx, 1);
        if (prc != FG_OK) return prc;
    }
    const hipStream_t s_up = ctx->s_up, s_down = ctx->s_down;
    uint8_t *h0 = nullptr, *h1 = nullptr, *d0 = nullptr, *d1 = nullptr;
    hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
    int rc = FG_OK;
    auto fail = [&](hipError_t err) {
        if (err != hipSuccess && rc == FG_OK) {
            ctx->last_hip = (int)err;
            rc = FG_ERR_HIP;
        }
        return err != hipSuccess;
    };
    do {
        if (fail(hipHostMalloc((void**)&h0, nbytes, hipHostMallocDefault)) || fail(hipHostMalloc((void**)&h1, nbytes, hipHostMallocDefault))) break;
        if (fail(hipMalloc((void**)&d0, nbytes)) || fail(hipMalloc((void**)&d1, nbytes))) break;
        memset(h0, 0x5A, nbytes);  // (touch the pages: first use must not be part of the figure)
        memset(h1, 0, nbytes);
        bool bad = false;
        for (auto& ev : e) bad = bad || fail(hipEventCreate(&ev));
        if (bad) break;
        double best[3] = {0, 0, 0};
        for (int rep = 0; rep < 4 && rc == FG_OK; ++rep) {  // (rep 0 warms the path up)
            float ms = 0.f;
            // host -> device
            if (fail(hipEventRecord(e[0], s_up)) || fail(hipMemcpyAsync(d0, h0, nbytes, hipMemcpyHostToDevice, s_up)) ||
                fail(hipEventRecord(e[1], s_up)) || fail(hipEventSynchronize(e[1])) || fail(hipEventElapsedTime(&ms, e[0], e[1])))
                break;
            if (rep && ms > 0.f) best[0] = std::max(best[0], (double)nbytes / (ms * 1e-3) / 1e9);
            // device -> host
            if (fail(hipEventRecord(e[0], s_down)) || fail(hipMemcpyAsync(h1, d1, nbytes, hipMemcpyDeviceToHost, s_down)) ||
                fail(hipEventRecord(e[1], s_down)) || fail(hipEventSynchronize(e[1])) || fail(hipEventElapsedTime(&ms, e[0], e[1])))
                break;
            if (rep && ms > 0.f) best[1] = std::max(best[1], (double)nbytes / (ms * 1e-3) / 1e9);
            // both at once: the slower stream bounds the pair (wall clock around both)
            if (fail(hipStreamSynchronize(s_up)) || fail(hipStreamSynchronize(s_down))) break;
            timespec a, b;
            clock_gettime(CLOCK_MONOTONIC, &a);
            if (fail(hipMemcpyAsync(d0, h0, nbytes, hipMemcpyHostToDevice, s_up)) ||
                fail(hipMemcpyAsync(h1, d1, nbytes, hipMemcpyDeviceToHost, s_down)) || fail(hipStreamSynchronize(s_up)) ||
                fail(hipStreamSynchronize(s_down)))
                break;
            clock_gettime(CLOCK_MONOTONIC, &b);
            const double s = (double)(b.tv_sec - a.tv_sec) + (double)(b.tv_nsec - a.tv_nsec) * 1e-9;
            if (rep && s > 0) best[2] = std::max(best[2], 2.0 * (double)nbytes / s / 1e9);
        }
        for (int k = 0; k < 3; ++k) gbps[k] = best[k];
    } while (false);
    for (auto& ev : e)
        if (ev) (void)hipEventDestroy(ev);
    if (d0) (void)hipFree(d0);
    if (d1) (void)hipFree(d1);
    if (h0) (void)hipHostFree(h0);
    if (h1) (void)hipHostFree(h1);
    return rc;
}

// Is [p, p + n) pinned host memory that the device can address (hipHostMalloc / hipHostRegister)?  -> the device's view of p, else null.
static const void* device_view_of_pinned(const void* p) {
    if (!p) return nullptr;
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof a);
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // (pageable memory: the runtime reports an error and keeps it sticky)
        return nullptr;
    }
    return a.type == hipMemoryTypeHost ? a.devicePointer : nullptr;
}
// ... and is [p, p + bytes) ONE mapping with a constant device-view delta from its first byte to its last?  (the first and
// the last byte of two adjacent registrations both qualify, the bytes between their device views need not be contiguous.)
static const void* pinned_span_device_view(const void* p, uint64_t bytes) {
    const uint8_t* const dv = (const uint8_t*)device_view_of_pinned(p);
    if (!dv || !bytes) return dv;
    const uint8_t* const last = (const uint8_t*)p + bytes - 1u;
    const uint8_t* const dv_last = (const uint8_t*)device_view_of_pinned(last);
    return dv_last && dv_last - dv == last - (const uint8_t*)p ? dv : nullptr;
}

static int pinned_tables_for_kernels(fg_ctx* ctx, const fg_tables& ht, fg_tables* kt);

// ZERO-COPY form of fg_decode_batch: when the caller's bytes and offsets live in PINNED host memory (where a batching framer
// accumulates them: fg_alloc_pinned) the decode kernels read them in place over the link and write every table column straight
// into the ctx's pinned tables -- no hipMemcpy, no slices, no events: ONE launch.  The kernels stream 1 KiB per wave-instruction
// with a 20 KiB prefetch window per wave, far more in flight than the link's latency-bandwidth product needs, so the launch runs at
// link speed in BOTH directions at once (tools/probe/zero_copy.py, profiles/r04b_zero_copy_probe.json: GELF 153 vs 134 M lines/s,
// LTSV 194 vs 170, cfg2 210 vs 196 against the sliced hipMemcpy pipeline below, whose uploads and downloads the runtime of this
// platform queues on ONE copy engine: profiles/r04a_timeline_*.log, an upload and a download never in flight together).  Only the
// entry counter stays in HBM (atomics).  Returns FG_ERR_UNSUPPORTED when the buffers do not qualify: the caller falls through.
// A decode grid whose tables lie in pinned host memory runs at the LINK's pace: its waves mostly wait for their stores to drain.  At full
// occupancy (GELF: twenty waves per CU) that costs throughput -- same box, 4 M GELF lines: fg_frame_decode_batch 105 M lines/s with
// every wave slot taken, 129 M at eight waves per CU; fg_decode_batch 151 -> 161 M (profiles/r04w_frame_overlap.log; the other formats'
// kernels hold eight waves or fewer anyway).  For the duration of a host pipeline the grid is capped at eight, unless the caller set
// its own figure (fg_set_launch_opts).
// the launches of a sliced batch share ONE entry table: fg::entry_chunk gives each of them a 1 / shares part of the table's budget
struct TableShares {
    fg_ctx* ctx;
    TableShares(fg_ctx* c, uint32_t launches) : ctx(c) { ctx->table_shares = launches; }
    ~TableShares() { ctx->table_shares = 0; }
};
struct LinkBoundGrid {  // (a per-call cap beside the caller's launch options, never written into them: ADVICE r4)
    fg_ctx* ctx;
    explicit LinkBoundGrid(fg_ctx* c, uint32_t waves = 8) : ctx(c) { ctx->link_bound_waves = waves; }
    ~LinkBoundGrid() { ctx->link_bound_waves = 0; }
};
// GELF's exact form (k_gelf_general: the lines the fast form hands back) runs ONCE, behind the last slice, over all rows -- it is a
// chain of dependent steps of ~170 us however few lines it gets, and launched per slice it was a quarter of the sliced raw-stream
// path's GPU time
struct DeferGeneral {
    fg_ctx* ctx;
    DeferGeneral(fg_ctx* c, bool on) : ctx(c) {
        ctx->defer_general = on;
        ctx->batch_epoch = 0;
    }
    ~DeferGeneral() {  // (also on every error path: nothing of this batch is left pending in the ctx)
        ctx->defer_general = false;
        ctx->batch_epoch = 0;
    }
};
// Whatever way a pipelined call leaves, it first waits for what it queued: copies of earlier slices may still be in flight into the
// ctx's buffers and out of the caller's bytes.  Constructed where the call may first have queued something (the exits before that pay
// no synchronisation), BEHIND the locals that asynchronous copies read or write, so that those outlive the wait.  The success path
// ends with done(), which reports what the wait reports.
struct DrainGuard {
    fg_ctx* ctx;
    bool armed = true;
    explicit DrainGuard(fg_ctx* c) : ctx(c) {}
    ~DrainGuard() {
        if (armed) (void)drain(ctx);
    }
    int done() {
        FG_HIP(ctx, drain(ctx));  // (a wait that failed is repeated by the destructor)
        armed = false;
        return FG_OK;
    }
};
// The slice loops keep a few slices queued beyond the one they collect: fill(k, issue) calls issue(slice) until `ahead` slices from
// slice k on are out (k = slices: all of them); -> the first result that is not FG_OK.
extern "C++" {  // (a template cannot stand in the extern "C" block around it)
struct LookAhead {
    uint32_t slices, ahead, issued = 0;
    LookAhead(uint32_t slices_, uint32_t ahead_) : slices(slices_), ahead(ahead_) {}
    template <class Issue>
    int fill(uint32_t k, Issue&& issue) {
        for (; issued < slices && issued < k + ahead; ++issued) {
            const int rc = issue(issued);
            if (rc != FG_OK) return rc;
        }
        return FG_OK;
    }
};
}
// a packed batch as fg_decode_batch and fg_transcode_batch take it: n + 1 offsets that lie within the buffer
static int check_packed_batch(fg_format fmt, uint64_t nbytes, const uint64_t* offsets, uint64_t n) {
    if (n == 0) return FG_OK;
    if (!offsets || offsets[n] > nbytes || offsets[0] > offsets[n]) return FG_ERR_ARG;
    if (fmt == FG_CAPNP)  // a message is an array of 8-byte words (include/fg_hip.h)
        for (uint64_t i = 0; i <= n; ++i)
            if (offsets[i] & 7u) return FG_ERR_ARG;
    return FG_OK;
}

static int decode_batch_zero_copy(fg_ctx* ctx, fg_format fmt, const uint8_t* bytes, uint64_t nbytes, const uint64_t* offsets, uint64_t n,
                                  fg_tables* out) {
    if (n == 0 || (ctx->lo.flags & FG_LO_NO_ZERO_COPY)) return FG_ERR_UNSUPPORTED;
    // (reads AND writes cross the link: two waves per CU fill it, and every wave more only queues in front of the dependent reads --
    //  offsets before bytes, GELF's exact form: LTSV 0.81 -> 0.89 of the link, structured data 0.90 -> 0.93, GELF 0.85 -> 0.87 with four,
    //  profiles/r06aa_decode_batch_waves.log)
    LinkBoundGrid grid(ctx, fmt == FG_GELF ? 4u : 2u);
    // one mapping each, up to the last byte the kernels touch: their 16-byte loads reach up to nbytes rounded up to 16 (include/fg_hip.h:
    // the packed buffer must be readable that far)
    const uint8_t* d_bytes = (const uint8_t*)pinned_span_device_view(bytes, up(nbytes, 16));
    const uint64_t* d_offsets = (const uint64_t*)pinned_span_device_view(offsets, (n + 1) * 8);
    if (!d_bytes || !d_offsets || ((uintptr_t)d_bytes & 15u) != 0) return FG_ERR_UNSUPPORTED;
    int rc;
    uint64_t ent_cap = first_ent_cap(fmt, nbytes);
    const hipStream_t s = ctx->stream;
    for (;;) {
        if ((rc = grow_pinned(ctx, (void**)&ctx->h_tab, &ctx->h_tab_cap, carved_bytes(n, ent_cap))) != FG_OK) return rc;
        fg_tables ht;
        carve(ctx->h_tab, n, ent_cap, &ht, nullptr);
        fg_tables kt;  // what the kernels see: the pinned columns (their device view) and the counter in HBM
        if ((rc = pinned_tables_for_kernels(ctx, ht, &kt)) != FG_OK) return rc;
        if ((rc = fg_decode_frames_impl(ctx, fmt, FG_FRAME_NONE, d_bytes, nbytes, d_offsets, n, nullptr, &kt, (void*)s, true,
                                        offsets[n] - offsets[0])) != FG_OK)
            return rc;
        uint64_t used = 0;
        FG_HIP(ctx, hipMemcpyAsync(&used, ctx->d_used, 8, hipMemcpyDeviceToHost, s));
        FG_HIP(ctx, hipStreamSynchronize(s));
        if (used > ent_cap) {
            if (ent_cap >= kEntCapMax) return FG_ERR_ENT_OVERFLOW;
            ent_cap = next_ent_cap(used);
            continue;
        }
        *ht.ent_used = used;
        *out = ht;
        ctx->last_host_path = FG_PATH_DECODE_ZERO_COPY;
        return FG_OK;
    }
}

int fg_decode_batch(fg_ctx* ctx, fg_format fmt, const uint8_t* bytes, uint64_t nbytes, const uint64_t* offsets,
                    uint64_t n, fg_tables* out) {
    if (!ctx || !out || (nbytes && !bytes)) return FG_ERR_ARG;
    if (check_packed_batch(fmt, nbytes, offsets, n) != FG_OK) return FG_ERR_ARG;
    DeviceGuard g(ctx->device);
    int rc;
    if ((rc = decode_batch_zero_copy(ctx, fmt, bytes, nbytes, offsets, n, out)) != FG_ERR_UNSUPPORTED) return rc;
    const uint32_t slices = slice_count(nbytes, n);
    TableShares shares(ctx, slices);
    if (slices > 1 && (rc = ensure_pipeline(ctx, slices)) != FG_OK) return rc;  // (a small batch stays on the ctx's own stream)
    if (slices > 1 && (rc = ensure_h_cnt(ctx)) != FG_OK) return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_bytes, &ctx->d_bytes_cap, up(nbytes, 16) + 16)) != FG_OK) return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_offsets, &ctx->d_offsets_cap, (n + 1) * 8)) != FG_OK) return rc;
    std::vector<uint64_t> cut(slices + 1);
    if (fg_shard_plan(offsets, n, slices, cut.data()) != FG_OK) return FG_ERR_ARG;
    const bool piped = slices > 1;
    const hipStream_t s_down = piped ? ctx->s_down : ctx->stream, s_up = piped ? ctx->s_up : s_down, s_run = piped ? ctx->s_run : s_down;
    uint64_t ent_cap = first_ent_cap(fmt, nbytes);  // grown on overflow
    uint64_t used = 0;
    DrainGuard drained(ctx);
    for (;;) {
        const uint64_t total = carved_bytes(n, ent_cap);
        if ((rc = grow_dev(ctx, (void**)&ctx->d_tab, &ctx->d_tab_cap, total)) != FG_OK) return rc;
        if ((rc = grow_pinned(ctx, (void**)&ctx->h_tab, &ctx->h_tab_cap, total)) != FG_OK) return rc;
        fg_tables dt, ht;
        carve(ctx->d_tab, n, ent_cap, &dt, nullptr);
        carve(ctx->h_tab, n, ent_cap, &ht, nullptr);
        FG_HIP(ctx, hipMemsetAsync(dt.ent_used, 0, 8, s_run));
        // Rows land at their final position, entries share one counter: the result is the same as one monolithic launch.
        // A slice is ISSUED (upload, kernels, the entry counter's value after it into a pinned word) and later COLLECTED (its rows and
        // the entries its kernels appended -- the range between two counter values -- come back on the download stream).  The host
        // issues sixteen slices ahead of the one it collects, so the link has uploads queued at all times and every table, the
        // entry columns included, crosses it while later slices are still going up.
        uint64_t* const ent_cnt = piped ? ctx->h_cnt + kCntEnts : nullptr;
        bool first_issued = false;  // offsets[l0] of a slice belongs to the slice before it -- except for the first slice that has rows
        auto issue = [&](uint32_t k) -> int {
            const uint64_t l0 = cut[k], l1 = cut[k + 1], rows = l1 - l0;
            if (rows == 0) return FG_OK;
            // ---- upload: the slice's offsets (the first slice WITH ROWS also takes its own start: fg_shard_plan gives empty leading
            //      slices when the lines cover fewer bytes than there are slices -- ADVICE r3) and its bytes, copied on 16-byte
            //      boundaries (the neighbouring bytes are the same data)
            const uint64_t o0 = first_issued ? l0 + 1 : l0;
            first_issued = true;
            FG_HIP(ctx, hipMemcpyAsync(ctx->d_offsets + o0, offsets + o0, (l1 + 1 - o0) * 8, hipMemcpyHostToDevice, s_up));
            const uint64_t b0 = offsets[l0] & ~15ull, b1 = offsets[l1];
            if (b1 > b0) FG_HIP(ctx, hipMemcpyAsync(ctx->d_bytes + b0, bytes + b0, b1 - b0, hipMemcpyHostToDevice, s_up));
            if (piped) {
                FG_HIP(ctx, hipEventRecord(ctx->ev_slice[2 * k], s_up));
                FG_HIP(ctx, hipStreamWaitEvent(s_run, ctx->ev_slice[2 * k], 0));
            }
            // ---- decode
            const fg_tables sl = fg::rows_of(dt, l0, rows);  // the slice's rows: same arrays, shifted by l0
            const int drc = fg_decode_frames_impl(ctx, fmt, FG_FRAME_NONE, ctx->d_bytes, nbytes, ctx->d_offsets + l0, rows, nullptr, &sl, (void*)s_run, false,
                                               offsets[l1] - offsets[l0]);
            if (drc != FG_OK) return drc;
            if (piped) {
                FG_HIP(ctx, hipMemcpyAsync(ent_cnt + k, dt.ent_used, 8, hipMemcpyDeviceToHost, s_run));
                FG_HIP(ctx, hipEventRecord(ctx->ev_slice[2 * k + 1], s_run));
            }
            return FG_OK;
        };
        used = 0;
        bool overflow = false;
        LookAhead window(slices, 16);
        for (uint32_t k = 0; k < slices && n; ++k) {
            if ((rc = window.fill(k, issue)) != FG_OK) return rc;
            const uint64_t l0 = cut[k], rows = cut[k + 1] - l0;
            if (rows == 0) continue;
            if (piped) {
                FG_HIP(ctx, hipEventSynchronize(ctx->ev_slice[2 * k + 1]));
                const uint64_t cnt = ent_cnt[k];  // the counter after this slice's kernels: its entries are [used, cnt)
                if (cnt > ent_cap) {
                    overflow = true;
                    break;
                }
                if ((rc = copy_rows(ctx, ht, dt, l0, rows, s_down)) != FG_OK || (rc = copy_entries(ctx, ht, dt, used, cnt, s_down)) != FG_OK) return rc;
                used = cnt;
            } else if ((rc = copy_rows(ctx, ht, dt, l0, rows, s_down)) != FG_OK) {
                return rc;
            }
        }
        if (!piped || overflow) {  // one stream (a small batch), or the entry table ran out: the counter's final value
            if (overflow) {  // (kernels past the capacity still count: the counter then says what the batch needs)
                if ((rc = window.fill(slices, issue)) != FG_OK) return rc;
                FG_HIP(ctx, drain(ctx));
            }
            FG_HIP(ctx, hipMemcpyAsync(&used, dt.ent_used, 8, hipMemcpyDeviceToHost, s_run));
            FG_HIP(ctx, hipStreamSynchronize(s_run));
            overflow = used > ent_cap;
        }
        if (overflow) {  // (nothing is in flight: the tables may be grown)
            if (ent_cap >= kEntCapMax) return FG_ERR_ENT_OVERFLOW;
            ent_cap = next_ent_cap(used);
            continue;
        }
        if (!piped && (rc = copy_entries(ctx, ht, dt, 0, used, s_down)) != FG_OK) return rc;
        *ht.ent_used = used;
        if ((rc = drained.done()) != FG_OK) return rc;
        *out = ht;
        ctx->last_host_path = FG_PATH_DECODE_SLICED;
        return FG_OK;
    }
}

static int frame_stage(fg_ctx* ctx, fg_framing framing, uint64_t nbytes, int final, uint64_t* n_frames, uint64_t* consumed);
static int decode_stage_to_host(fg_ctx* ctx, fg_format fmt, fg_framing framing, uint64_t nbytes, uint64_t n, const uint8_t* d_bad,
                                const uint8_t* d_src, fg_tables* out);

// A framer's capacity is an estimate: call(cap) grows what depends on it and calls the device entry, which answers FG_ERR_ENT_OVERFLOW
// with the count it found in *n -- the whole framer then runs again, sized from that count.
extern "C++" {  // (a template cannot stand in the extern "C" block around it)
template <class Call>
static int frame_with_retry(uint64_t cap, const uint64_t* n, Call&& call) {
    for (;;) {
        const int rc = call(cap);
        if (rc != FG_ERR_ENT_OVERFLOW) return rc;
        cap = *n + 16;
    }
}
}

// The host hop of the octet-counted framing (what fg::BatchingSplitter's Syslen branch does), prefixes of any length: walk() one chunk
// after the other, then upload() the packed batch where the device framer would have left it (ctx->d_sl_packed, d_offsets, d_bad).
struct SyslenHop {
    std::vector<uint64_t> starts, offs{0};  // per frame: where its prefix starts in the buffer; its payload in `packed` (n + 1)
    std::vector<uint8_t> packed, bad;
    // the chunk bytes[at .. at + len): its frames are appended; -> its stop reason, *consumed = the bytes of the chunk they cover
    int walk(const uint8_t* bytes, uint64_t at, uint64_t len, uint64_t* consumed) {
        const uint8_t* const seg = bytes + at;
        return (int)fg::syslen::host_walk(seg, len, ~0ull, consumed, [&](uint64_t pos, uint32_t plen, uint64_t flen) {
            const uint8_t* b = seg + pos + plen;
            starts.push_back(at + pos);
            packed.insert(packed.end(), b, b + flen);
            offs.push_back(packed.size());
            bad.push_back(fg::utf8::payload_bad(b, flen) ? 1 : 0);
        });
    }
    // queued on s, NOT waited for: the caller synchronises before this object goes out of scope
    int upload(fg_ctx* ctx, hipStream_t s) const {
        const uint64_t n = bad.size(), payload = packed.size();
        if (payload) FG_HIP(ctx, hipMemcpyAsync(ctx->d_sl_packed, packed.data(), payload, hipMemcpyHostToDevice, s));
        FG_HIP(ctx, hipMemsetAsync(ctx->d_sl_packed + payload, 0, up(payload, 16) + 16 - payload, s));
        FG_HIP(ctx, hipMemcpyAsync(ctx->d_offsets, offs.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
        if (n) FG_HIP(ctx, hipMemcpyAsync(ctx->d_bad, bad.data(), n, hipMemcpyHostToDevice, s));
        return FG_OK;
    }
};
// ... and of the Cap'n Proto framing: the offsets of the whole messages of the chunk bytes[at .. at + len) are appended
static int capnp_hop(const uint8_t* bytes, uint64_t at, uint64_t len, uint64_t* consumed, std::vector<uint64_t>& offs) {
    return (int)fg::capnpf::host_walk(bytes + at, len, consumed, [&](uint64_t p) { offs.push_back(at + p); });
}

// FG_FRAME_SYSLEN stage shared by fg_frame_decode_batch and fg_transcode_batch (the read_msglen / read_exact loop of
// SyslenSplitter::run, syslen_splitter.rs:42-57, for a chunk): the chunk goes up as it is (one copy; from a pinned
// chunk the copy engine reads it in place at link speed and no payload byte is touched by the host's cores) and is framed + packed in HBM.  When the device
// framer declines (fg_frame_syslen_device: FG_ERR_UNSUPPORTED) or meets a prefix beyond its bound, the prefixes are hopped on the host
// over the caller's bytes and the packed batch is uploaded: the same results either way.  Leaves the payloads in ctx->d_sl_packed,
// their offsets in ctx->d_offsets, the verdicts in ctx->d_bad, the frame starts in ctx->h_off (host, n + 1 entries).
static int syslen_stage(fg_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, int final, uint64_t* n_frames, uint64_t* consumed, uint64_t* payload) {
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_bytes, &ctx->d_bytes_cap, up(nbytes, 16) + 16)) != FG_OK) return rc;
    FG_HIP(ctx, hipMemcpyAsync(ctx->d_bytes, bytes, nbytes, hipMemcpyHostToDevice, s));
    FG_HIP(ctx, hipMemsetAsync(ctx->d_bytes + nbytes, 0, up(nbytes, 16) + 16 - nbytes, s));
    const uint8_t* const d_src = ctx->d_bytes;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_sl_packed, &ctx->d_sl_packed_cap, up(nbytes, 16) + 16)) != FG_OK) return rc;
    auto ensure = [&](uint64_t cap) -> int {
        int r;
        if ((r = grow_dev(ctx, (void**)&ctx->d_offsets, &ctx->d_offsets_cap, (cap + 2) * 8)) != FG_OK) return r;
        if ((r = grow_dev(ctx, (void**)&ctx->d_sl_starts, &ctx->d_sl_starts_cap, (cap + 2) * 8)) != FG_OK) return r;
        if ((r = grow_dev(ctx, (void**)&ctx->d_bad, &ctx->d_bad_cap, cap + 1)) != FG_OK) return r;
        return grow_pinned(ctx, (void**)&ctx->h_off, &ctx->h_off_cap, (cap + 2) * 8);
    };
    uint64_t cap = (uint64_t)((double)nbytes * ctx->frames_per_byte * 1.25) + 1024, n = 0;
    int stop = FG_SYSLEN_CLEAN;
    // (two deliberate simplifications: a cap_frames that turns out too small runs the whole framer again with the count it reported --
    //  the next chunk is sized from this one's frames per byte --, and a prefix beyond the device parser's bound sends the WHOLE chunk
    //  through the host hop below, not just that one frame: leading zeros by the dozen are legal and never seen)
    rc = frame_with_retry(cap, &n, [&](uint64_t c) {
        const int r = ensure(c);
        return r != FG_OK ? r : fg_frame_syslen_device(ctx, d_src, nbytes, final, ctx->d_sl_packed, ctx->d_offsets, ctx->d_sl_starts, ctx->d_bad, c, &n,
                                                       consumed, &stop, FG_STREAM_OWN);
    });
    if (rc == FG_OK && stop != FG_SYSLEN_LONG_PREFIX) {
        ctx->last_host_path = FG_PATH_FRAME_SYSLEN_DEVICE;
        *payload = ctx->last_syslen_payload;
        // (the decoders load 16 bytes at a time: the pad behind the last payload is zero, as behind an uploaded batch)
        FG_HIP(ctx, hipMemsetAsync(ctx->d_sl_packed + *payload, 0, up(*payload, 16) + 16 - *payload, s));
        FG_HIP(ctx, hipMemcpyAsync(ctx->h_off, ctx->d_sl_starts, (n + 1) * 8, hipMemcpyDeviceToHost, s));
        FG_HIP(ctx, hipStreamSynchronize(s));
    } else if (rc == FG_OK || rc == FG_ERR_UNSUPPORTED) {
        SyslenHop hop;
        stop = hop.walk(bytes, 0, nbytes, consumed);
        n = hop.starts.size();
        hop.starts.push_back(*consumed);
        if ((rc = ensure(n)) != FG_OK) return rc;
        memcpy(ctx->h_off, hop.starts.data(), (n + 1) * 8);
        if ((rc = hop.upload(ctx, s)) != FG_OK) return rc;
        FG_HIP(ctx, hipStreamSynchronize(s));  // (the vectors go out of scope)
        *payload = hop.packed.size();
        ctx->last_host_path = FG_PATH_FRAME_SYSLEN_HOST;
    } else {
        return rc;
    }
    ctx->last_syslen_stop = stop;
    *n_frames = n;
    return FG_OK;
}

// FG_FRAME_CAPNP stage shared by fg_frame_decode_batch and fg_transcode_batch (the read_message loop of CapnpSplitter::run,
// capnp_splitter.rs:24-46, for a chunk): the chunk is already in ctx->d_bytes (zero padded) and is framed where it lies; the decoders
// then read the messages from the same buffer.  When the device framer declines (fg_frame_capnp_device: FG_ERR_UNSUPPORTED) the segment
// tables are walked on the host over the caller's bytes and the offsets are uploaded: the same results either way.  Leaves the message
// offsets in ctx->d_offsets (n + 1 entries).
static int capnp_stage(fg_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, int final, uint64_t* n_frames, uint64_t* consumed) {
    hipStream_t s = ctx->stream;
    int rc, stop = FG_CAPNP_CLEAN;
    // (a message of the record schema is a few hundred bytes; a cap_frames that turns out too small runs the framer again with the
    //  count it reported, like syslen_stage)
    uint64_t n = 0;
    rc = frame_with_retry(nbytes / 64 + 1024, &n, [&](uint64_t cap) {
        const int r = grow_dev(ctx, (void**)&ctx->d_offsets, &ctx->d_offsets_cap, (cap + 2) * 8);
        return r != FG_OK ? r : fg_frame_capnp_device(ctx, ctx->d_bytes, nbytes, final, ctx->d_offsets, cap, &n, consumed, &stop, FG_STREAM_OWN);
    });
    if (rc == FG_OK) {
        ctx->last_host_path = FG_PATH_FRAME_CAPNP_DEVICE;
    } else if (rc == FG_ERR_UNSUPPORTED) {
        std::vector<uint64_t> offs;
        stop = capnp_hop(bytes, 0, nbytes, consumed, offs);
        offs.push_back(*consumed);
        n = offs.size() - 1;
        if ((rc = grow_dev(ctx, (void**)&ctx->d_offsets, &ctx->d_offsets_cap, (n + 2) * 8)) != FG_OK) return rc;
        FG_HIP(ctx, hipMemcpyAsync(ctx->d_offsets, offs.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
        FG_HIP(ctx, hipStreamSynchronize(s));  // (the vector goes out of scope)
        ctx->last_host_path = FG_PATH_FRAME_CAPNP_HOST;
    } else {
        return rc;
    }
    ctx->last_capnp_stop = stop;
    *n_frames = n;
    return FG_OK;
}

static int frame_decode_one_piece(fg_ctx* ctx, fg_format fmt, fg_framing framing, const uint8_t* bytes, uint64_t nbytes, int final,
                                  fg_tables* out, const uint64_t** out_offsets, uint64_t* n_frames, uint64_t* consumed) {
    if (!ctx || !out || !out_offsets || !n_frames || !consumed || (nbytes && !bytes)) return FG_ERR_ARG;
    if ((fmt == FG_CAPNP) != (framing == FG_FRAME_CAPNP)) return FG_ERR_ARG;  // (a capnp stream has its own framing, and nothing else has it)
    if (framing != FG_FRAME_LINE && framing != FG_FRAME_NUL && framing != FG_FRAME_SYSLEN && framing != FG_FRAME_CAPNP) return FG_ERR_UNSUPPORTED;
    const bool syslen = framing == FG_FRAME_SYSLEN, capnp = framing == FG_FRAME_CAPNP;
    *n_frames = 0;
    *consumed = 0;
    *out_offsets = nullptr;
    if (syslen) ctx->last_syslen_stop = FG_SYSLEN_CLEAN;
    if (capnp) ctx->last_capnp_stop = FG_CAPNP_CLEAN;
    if (nbytes == 0) return FG_OK;
    DeviceGuard g(ctx->device);
    hipStream_t s = ctx->stream;
    int rc;
    uint64_t n = 0, payload = 0;
    if (syslen) {
        // 1. frame + pack where the chunk lies; what is decoded is the packed batch (FG_FRAME_NONE), what goes back are the frame starts
        if ((rc = syslen_stage(ctx, bytes, nbytes, final, &n, consumed, &payload)) != FG_OK) return rc;
    } else {
        if ((rc = grow_dev(ctx, (void**)&ctx->d_bytes, &ctx->d_bytes_cap, up(nbytes, 16) + 16)) != FG_OK) return rc;
        FG_HIP(ctx, hipMemcpyAsync(ctx->d_bytes, bytes, nbytes, hipMemcpyHostToDevice, s));
        FG_HIP(ctx, hipMemsetAsync(ctx->d_bytes + nbytes, 0, up(nbytes, 16) + 16 - nbytes, s));
        // 1. frame: offsets + UTF-8 verdicts (a capnp stream: offsets only, Text is checked by the decoder)
        if (capnp) rc = capnp_stage(ctx, bytes, nbytes, final, &n, consumed);
        else rc = frame_stage(ctx, framing, nbytes, final, &n, consumed);
        if (rc != FG_OK) return rc;
    }
    *n_frames = n;
    if (n && nbytes >= (1u << 20)) ctx->frames_per_byte = (double)n / (double)nbytes;
    if (!syslen) {
        if ((rc = grow_pinned(ctx, (void**)&ctx->h_off, &ctx->h_off_cap, (n + 1) * 8)) != FG_OK) return rc;
        FG_HIP(ctx, hipMemcpyAsync(ctx->h_off, ctx->d_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    }
    *out_offsets = ctx->h_off;
    if (n == 0) {
        FG_HIP(ctx, hipStreamSynchronize(s));
        fg_tables empty{};
        *out = empty;
        return FG_OK;
    }
    // 2. decode the frames in place (terminators stripped in-kernel, invalid UTF-8 -> FG_ST_BAD_UTF8)
    const uint64_t used_bytes = syslen ? payload : *consumed;
    const uint8_t* const dec_bytes = syslen ? ctx->d_sl_packed : ctx->d_bytes;
    const fg_framing dec_framing = syslen || capnp ? FG_FRAME_NONE : framing;
    return decode_stage_to_host(ctx, fmt, dec_framing, used_bytes, n, capnp ? nullptr : ctx->d_bad, dec_bytes, out);
}

// the kernels' view of tables carved from the ctx's PINNED host block (zero-copy output): every column pointer translated to the
// device's view of that memory, the entry counter in HBM (atomics)
static int pinned_tables_for_kernels(fg_ctx* ctx, const fg_tables& ht, fg_tables* kt) {
    const uint8_t* dv = (const uint8_t*)device_view_of_pinned(ctx->h_tab);
    if (!dv) return FG_ERR_UNSUPPORTED;
    if (!ctx->d_used) FG_HIP(ctx, hipMalloc((void**)&ctx->d_used, 256));
    *kt = fg::shifted(ht, dv - ctx->h_tab);  // (by 0 under unified addressing)
    kt->ent_used = ctx->d_used;
    return FG_OK;
}

// fg_frame_decode_batch for a LARGE raw chunk: the chunk crosses the link in slices (multiples of the framing kernels' 16 KiB
// block) on the upload stream; as soon as a slice is there it is framed (delimiter ranks continue where the slice before stopped),
// its frame count comes back to the host through a pinned word, and the frames that END in it are decoded -- all while the next
// slices are still on the link.  The host never frames, never uploads offsets.  Round 4: the decode kernels write the table
// columns STRAIGHT INTO THE PINNED HOST TABLES (zero-copy output) and the per-slice counters come back by a one-thread kernel, so
// the copy engine carries nothing but the uploads -- on this platform a device -> host hipMemcpy queues behind every upload issued
// before it (profiles/r04a_timeline_*: an upload and a download were never in flight together), which is what held the GELF and
// LTSV corpora at the SUM of their two directions.  Only the frame offsets (8 bytes per frame) are still copied.
// Tables are sized from what the ctx's last chunk held; a chunk that outgrows the estimate (or the entry table) returns
// FG_ERR_UNSUPPORTED and takes the one-piece path, which counts first.
static int frame_decode_sliced(fg_ctx* ctx, fg_format fmt, fg_framing framing, const uint8_t* bytes, uint64_t nbytes, int final,
                               fg_tables* out, const uint64_t** out_offsets, uint64_t* n_frames, uint64_t* consumed) {
    int rc;
    LinkBoundGrid grid(ctx);
    DeferGeneral defer(ctx, fmt == FG_GELF);
    const uint64_t blk = fg_frame_block_bytes();
    // (sixteen slices or more: the first upload and the last decode + download run alone -- a sixteenth of the batch each, not an eighth;
    //  whole 64 KiB tiles of the one-pass scan)
    const uint64_t slice = slice_bytes(nbytes, 16) / fg_frame_slice_align() * fg_frame_slice_align();
    const uint32_t slices = (uint32_t)((nbytes + slice - 1) / slice);
    TableShares shares(ctx, slices);
    const uint64_t nblk_total = nbytes / blk + 1;
    if ((rc = ensure_pipeline(ctx, slices)) != FG_OK) return rc;
    const hipStream_t s_up = ctx->s_up, s_run = ctx->s_run, s_down = ctx->s_down;
    // capacities from the ctx's experience: frames, rows, entries
    const uint64_t cap = (uint64_t)((double)nbytes * ctx->frames_per_byte * 1.25) + 4096;
    const uint64_t ent_cap = first_ent_cap(fmt, nbytes);
    if ((rc = grow_dev(ctx, (void**)&ctx->d_bytes, &ctx->d_bytes_cap, up(nbytes, 16) + 16)) != FG_OK) return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_offsets, &ctx->d_offsets_cap, (cap + 2) * 8)) != FG_OK) return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_bad, &ctx->d_bad_cap, cap + 1)) != FG_OK) return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_frame, &ctx->d_frame_cap, fg_frame_scratch_bytes(nbytes))) != FG_OK) return rc;
    if ((rc = grow_pinned(ctx, (void**)&ctx->h_off, &ctx->h_off_cap, (cap + 2) * 8)) != FG_OK) return rc;
    if ((rc = ensure_h_cnt(ctx)) != FG_OK) return rc;
    if (slices + 2 > kMaxFrameSlices) return FG_ERR_UNSUPPORTED;
    uint64_t* const h_slice_cnt = ctx->h_cnt + kCntSlices;
    uint64_t* const cnt_dv = (uint64_t*)const_cast<void*>(device_view_of_pinned(h_slice_cnt));
    if (!cnt_dv) return FG_ERR_UNSUPPORTED;
    if ((rc = grow_pinned(ctx, (void**)&ctx->h_tab, &ctx->h_tab_cap, carved_bytes(cap, ent_cap))) != FG_OK) return rc;
    fg_tables ht, kt;
    carve(ctx->h_tab, cap, ent_cap, &ht, nullptr);
    if ((rc = pinned_tables_for_kernels(ctx, ht, &kt)) != FG_OK) return rc;
    uint64_t last_end = 0, used = 0;  // (read back from the device)
    DrainGuard drained(ctx);
    FG_HIP(ctx, hipMemsetAsync(kt.ent_used, 0, 8, s_run));
    FG_HIP(ctx, hipMemsetAsync(ctx->d_bad, 0, cap + 1, s_run));
    FG_HIP(ctx, hipEventRecord(ctx->ev_ready, s_run));
    FG_HIP(ctx, hipStreamWaitEvent(s_up, ctx->ev_ready, 0));  // (the framing kernels below write d_bad on the upload stream)
    const uint32_t delim = framing == FG_FRAME_LINE ? 0x0Au : 0x00u;
    std::vector<hipEvent_t>& ev = ctx->ev_slice;
    // A raw chunk in PINNED memory is not uploaded at all: the framing scan reads it where it is, over the link, and stores it to
    // HBM on the way (k_frame_scan<COPY>) -- the copy engine stays out of it, and the kernels of slice k + 1 (reads over the link, on
    // the upload stream) run beside the decode kernels of slice k (writes over the link).  Pageable memory: hipMemcpy per slice.
    // MEASURED (profiles/r04l_*): slower than the copy engine's uploads on this platform -- cfg2 91 vs 184 M lines/s, GELF 73 vs 96,
    // LTSV 84 vs 122 -- the framing kernels of slice k + 1 do not run beside the persistent decode grid of slice k, so the two
    // directions of the link take turns again.  Off by default (FG_LO_FRAME_KERNEL_UPLOAD turns it on for further work).
    const uint8_t* src_dv = ((ctx->lo.flags & FG_LO_FRAME_KERNEL_UPLOAD) && ((uintptr_t)bytes & 15u) == 0 && device_view_of_pinned(bytes + nbytes - 1))
                                ? (const uint8_t*)device_view_of_pinned(bytes) : nullptr;
    // Copy-engine uploads: EVERY upload is queued now, back to back on the upload stream (they depend on nothing: the link never waits
    // for the host, and nothing else is ever queued between two of them -- framing kernels on the same stream held the next upload
    // up for their whole duration: GELF 96 -> 69 M lines/s, profiles/r04y_e2e_*); slice k is framed on the kernel stream once its
    // event fires.  Kernel upload: the scan IS the upload, on the upload stream, a few slices ahead of the decodes.
    if (!src_dv) {
        for (uint32_t k = 0; k < slices; ++k) {
            const uint64_t b0 = (uint64_t)k * slice, b1 = k + 1 == slices ? nbytes : b0 + slice;
            FG_HIP(ctx, hipMemcpyAsync(ctx->d_bytes + b0, bytes + b0, b1 - b0, hipMemcpyHostToDevice, s_up));
            if (k + 1 == slices) FG_HIP(ctx, hipMemsetAsync(ctx->d_bytes + nbytes, 0, up(nbytes, 16) + 16 - nbytes, s_up));
            FG_HIP(ctx, hipEventRecord(ev[2 * k], s_up));
        }
    }
    // framing of slice k; its cumulative frame count lands in a pinned word (all asynchronous)
    auto enqueue = [&](uint32_t k) -> int {
        const uint64_t b0 = (uint64_t)k * slice, b1 = k + 1 == slices ? nbytes : b0 + slice;
        const hipStream_t s_frame = src_dv ? s_up : s_run;
        if (!src_dv) FG_HIP(ctx, hipStreamWaitEvent(s_run, ev[2 * k], 0));
        else if (k + 1 == slices) FG_HIP(ctx, hipMemsetAsync(ctx->d_bytes + up(nbytes, 16), 0, 16, s_up));
        uint64_t* d_total = nullptr;
        const uint64_t blk0 = b0 / blk, blk1 = k + 1 == slices ? nblk_total : b1 / blk;
        FG_LAUNCH(ctx, fg_launch_frame_slice(ctx->d_bytes, nbytes, delim, ctx->d_frame, ctx->d_offsets, ctx->d_bad, cap, blk0, blk1, &d_total, s_frame, src_dv,
                                             (ctx->lo.flags & FG_LO_FRAME_CLASSIC) ? 1 : (ctx->lo.flags & FG_LO_FRAME_SELFTEST_STALL) ? 2 : 0));
        FG_LAUNCH(ctx, fg_launch_poke64(d_total, cnt_dv + k, s_frame));
        FG_HIP(ctx, hipEventRecord(ev[2 * k + 1], s_frame));
        if (src_dv) FG_HIP(ctx, hipStreamWaitEvent(s_run, ev[2 * k + 1], 0));
        return FG_OK;
    };
    uint64_t done = 0;  // frames decoded so far
    auto decode_rows = [&](uint64_t f0, uint64_t f1, uint64_t span_bytes) -> int {  // frames [f0, f1): decode into the pinned tables
        if (f1 == f0) return FG_OK;
        const uint64_t rows = f1 - f0;
        const fg_tables sl = fg::rows_of(kt, f0, rows);
        int r = fg_decode_frames_impl(ctx, fmt, framing, ctx->d_bytes, nbytes, ctx->d_offsets + f0, rows, ctx->d_bad + f0, &sl, (void*)s_run, false, span_bytes);
        if (r != FG_OK) return r;
        // the frames' offsets (8 bytes per frame) are the one thing still copied: behind the uploads on the copy engine, i.e. at the end
        FG_HIP(ctx, hipEventRecord(ctx->ev_ready, s_run));
        FG_HIP(ctx, hipStreamWaitEvent(s_down, ctx->ev_ready, 0));
        FG_HIP(ctx, hipMemcpyAsync(ctx->h_off + f0 + (f0 ? 1 : 0), ctx->d_offsets + f0 + (f0 ? 1 : 0), (rows + (f0 ? 0 : 1)) * 8, hipMemcpyDeviceToHost, s_down));
        return FG_OK;
    };
    LookAhead window(slices, src_dv ? 4u : 2u);  // framing queued ahead of the decode being issued
    for (uint32_t k = 0; k < slices; ++k) {
        if ((rc = window.fill(k, enqueue)) != FG_OK) return rc;
        FG_HIP(ctx, hipEventSynchronize(ev[2 * k + 1]));
        const uint64_t total = h_slice_cnt[k];  // delimiters up to the end of slice k = frames that are complete
        if (total == FG_FRAME_ABORTED) return FG_ERR_UNSUPPORTED;  // the one-pass scan gave up waiting on a tile (never seen): the one-piece path frames classically
        if (total + 1 > cap) {
            ctx->frames_per_byte = (double)(total + 1) / (double)(((uint64_t)k + 1) * slice);
            return FG_ERR_UNSUPPORTED;
        }
        const uint64_t b1 = k + 1 == slices ? nbytes : ((uint64_t)k + 1) * slice;
        if (k + 1 < slices) {
            if ((rc = decode_rows(done, total, b1 - (uint64_t)k * slice)) != FG_OK) return rc;
            done = total;
            continue;
        }
        // the last slice: an unterminated tail is one more frame when the stream ends here, else it stays with the caller
        FG_HIP(ctx, hipMemcpyAsync(&last_end, ctx->d_offsets + total, 8, hipMemcpyDeviceToHost, s_run));
        FG_HIP(ctx, hipStreamSynchronize(s_run));
        const bool tail = last_end != nbytes;
        uint64_t n = total;
        if (tail && final) {
            h_slice_cnt[slices] = nbytes;
            FG_HIP(ctx, hipMemcpyAsync(ctx->d_offsets + total + 1, h_slice_cnt + slices, 8, hipMemcpyHostToDevice, s_run));
            n = total + 1;
        }
        *consumed = (tail && !final) ? last_end : nbytes;
        if ((rc = decode_rows(done, n, *consumed > (uint64_t)k * slice ? *consumed - (uint64_t)k * slice : 1)) != FG_OK) return rc;
        done = n;
    }
    {
        fg_tables all = kt;
        all.n = done;
        if ((rc = fg_finish_deferred_general(ctx, framing, ctx->d_bytes, ctx->d_offsets, done, ctx->d_bad, &all, (void*)s_run)) != FG_OK) return rc;
    }
    FG_HIP(ctx, hipMemcpyAsync(&used, kt.ent_used, 8, hipMemcpyDeviceToHost, s_run));
    FG_HIP(ctx, hipStreamSynchronize(s_run));
    if (done) ctx->frames_per_byte = (double)done / (double)nbytes;
    if ((rc = drained.done()) != FG_OK) return rc;
    if (used > ent_cap) return FG_ERR_UNSUPPORTED;
    *ht.ent_used = used;
    ht.n = done;
    *out = ht;
    *out_offsets = ctx->h_off;
    *n_frames = done;
    if (done == 0) {
        fg_tables empty{};
        *out = empty;
    }
    return FG_OK;
}

// fg_frame_decode_batch as ONE LAUNCH (round 6): a raw chunk in PINNED memory is neither uploaded nor framed by a pass of its own -- the
// decode kernel reads it in place over the link, frames its tiles itself (fg_fused.hpp) and writes rows, entries AND the frame offsets
// straight into the ctx's pinned tables: what fg_decode_batch's zero-copy form does for framed lines, now for the raw stream -- the path a
// flowgger input really has (LineSplitter::run over a socket's bytes).  Until round 5 this path was an upload + a framing scan + a capped
// decode grid per slice and ran at 0.55-0.87 of the link where the zero-copy form did 0.80-0.97.
// FG_ERR_UNSUPPORTED: the chunk does not qualify (pageable memory, long lines, a table estimate that turned out too small, the
// look-back's bounded wait ran out): the caller takes the paths below.
static int frame_decode_fused(fg_ctx* ctx, fg_format fmt, fg_framing framing, const uint8_t* bytes, uint64_t nbytes, int final, fg_tables* out,
                              const uint64_t** out_offsets, uint64_t* n_frames, uint64_t* consumed) {
    if (nbytes == 0 || (ctx->lo.flags & (FG_LO_NO_FUSED_FRAMING | FG_LO_NO_ZERO_COPY | FG_LO_FRAME_CLASSIC | FG_LO_FRAME_SELFTEST_STALL | FG_LO_FRAME_KERNEL_UPLOAD))) return FG_ERR_UNSUPPORTED;
    if (fmt != FG_RFC5424 && fmt != FG_LTSV && fmt != FG_GELF) return FG_ERR_UNSUPPORTED;
    const uint8_t* d_bytes = (const uint8_t*)pinned_span_device_view(bytes, up(nbytes, 16));  // (ONE mapping up to the last byte the kernels load)
    if (!d_bytes || ((uintptr_t)d_bytes & 15u) != 0) return FG_ERR_UNSUPPORTED;
    LinkBoundGrid grid(ctx);
    int rc;
    // tables from the ctx's experience (frames per byte of its last chunk) and one entry per 16 / 8 input bytes; a chunk that holds more
    // of either says how many, and the launch is repeated ONCE PER TABLE with what it needs (another pass over the link -- the price
    // of the older forms' count-first as well -- and the next chunk is sized from this one)
    uint64_t cap = (uint64_t)((double)nbytes * ctx->frames_per_byte * 1.25) + 4096;
    uint64_t ent_cap = first_ent_cap(fmt, nbytes);
    if ((rc = ensure_h_cnt(ctx)) != FG_OK) return rc;
    const hipStream_t s = ctx->stream;
    fg_tables ht;
    uint64_t total = 0, used = 0;
    for (int attempt = 0;; ++attempt) {
        if ((rc = grow_pinned(ctx, (void**)&ctx->h_tab, &ctx->h_tab_cap, carved_bytes(cap, ent_cap))) != FG_OK) return rc;
        if ((rc = grow_pinned(ctx, (void**)&ctx->h_off, &ctx->h_off_cap, (cap + 2) * 8)) != FG_OK) return rc;
        fg_tables kt;
        carve(ctx->h_tab, cap, ent_cap, &ht, nullptr);
        if ((rc = pinned_tables_for_kernels(ctx, ht, &kt)) != FG_OK) return rc;
        uint64_t* const off_dv = (uint64_t*)const_cast<void*>(device_view_of_pinned(ctx->h_off));
        if (!off_dv) return FG_ERR_UNSUPPORTED;
        unsigned long long* d_total = nullptr;
        if ((rc = fg_frame_decode_impl(ctx, fmt, framing, d_bytes, nbytes, final, off_dv, cap, &kt, 0, (void*)s, &d_total)) != FG_OK) return rc;
        uint64_t* const res = ctx->h_cnt + kCntFused;  // [0] frames [1] abort [2] entries
        FG_HIP(ctx, hipMemcpyAsync(res, d_total, 16, hipMemcpyDeviceToHost, s));
        FG_HIP(ctx, hipMemcpyAsync(res + 2, kt.ent_used, 8, hipMemcpyDeviceToHost, s));
        FG_HIP(ctx, hipStreamSynchronize(s));
        total = res[0], used = res[2];
        if (res[1] != 0) return FG_ERR_UNSUPPORTED;  // (the look-back's bounded wait ran out: never seen)
        const bool rows_short = total > cap, ents_short = used > ent_cap;
        if (!rows_short && !ents_short) break;
        if (rows_short) ctx->frames_per_byte = (double)(total + 1) / (double)nbytes;
        if (attempt >= 2 || (ents_short && ent_cap >= kEntCapMax)) return FG_ERR_UNSUPPORTED;
        if (rows_short) cap = total + total / 16 + 1024;
        if (ents_short) ent_cap = next_ent_cap(used);  // (rows beyond the old capacity had no entries yet: a third launch may follow)
    }
    if (total && nbytes >= (1u << 20)) ctx->frames_per_byte = (double)total / (double)nbytes;
    *n_frames = total;
    ctx->last_host_path = FG_PATH_FRAME_FUSED;
    if (total == 0) {
        fg_tables empty{};
        *out = empty;
        ctx->h_off[0] = 0;
        *out_offsets = ctx->h_off;
        *consumed = 0;
        return FG_OK;
    }
    *ht.ent_used = used;
    ht.n = total;
    *out = ht;
    *out_offsets = ctx->h_off;
    *consumed = ctx->h_off[total];
    return FG_OK;
}

// The UDP input for a batch of datagrams in host memory (handle_record_maybe_compressed, input/udp_input.rs:100-143): one upload,
// fg_udp_unpack_device into ctx-owned HBM (counted first, so the buffer is sized by what the batch inflates to), the decode of the
// packed payloads as FG_FRAME_NONE with the drop flags as its UTF-8 verdicts, and the tables, the payloads, their offsets and the
// per-datagram status back into pinned memory.  One piece: a datagram batch is small beside the chunks the sliced forms are for.
int fg_udp_decode_batch(fg_ctx* ctx, fg_format fmt, const uint8_t* bytes, uint64_t nbytes, const uint64_t* offsets, uint64_t n,
                        uint64_t max_inflated, fg_tables* out, const uint8_t** out_lines, const uint64_t** out_line_offsets,
                        const uint8_t** udp_status) {
    if (!ctx || !out || !out_lines || !out_line_offsets || !udp_status || !offsets || (nbytes && !bytes)) return FG_ERR_ARG;
    if (fmt == FG_CAPNP) return FG_ERR_ARG;  // (the reference has no Decoder for it: config.rs picks the capnp splitter, not a decoder)
    if (fmt != FG_RFC5424 && fmt != FG_LTSV && fmt != FG_GELF && fmt != FG_RFC3164) return FG_ERR_ARG;
    if (n && (offsets[0] != 0 || offsets[n] != nbytes)) return FG_ERR_ARG;
    for (uint64_t i = 0; i < n; ++i)  // (one pass over host memory: an offset that runs backwards would reach the kernels as a huge length)
        if (offsets[i] > offsets[i + 1]) return FG_ERR_ARG;
    *out_lines = nullptr;
    *out_line_offsets = nullptr;
    *udp_status = nullptr;
    fg_tables empty{};
    *out = empty;
    if (n == 0) return FG_OK;
    DeviceGuard g(ctx->device);
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_bytes, &ctx->d_bytes_cap, up(nbytes, 16) + 16)) != FG_OK) return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_udp_off, &ctx->d_udp_off_cap, (n + 2) * 8)) != FG_OK) return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_offsets, &ctx->d_offsets_cap, (n + 2) * 8)) != FG_OK) return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_bad, &ctx->d_bad_cap, n + 1)) != FG_OK) return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_udp_st, &ctx->d_udp_st_cap, n + 1)) != FG_OK) return rc;
    if (nbytes) FG_HIP(ctx, hipMemcpyAsync(ctx->d_bytes, bytes, nbytes, hipMemcpyHostToDevice, s));
    FG_HIP(ctx, hipMemsetAsync(ctx->d_bytes + nbytes, 0, up(nbytes, 16) + 16 - nbytes, s));
    FG_HIP(ctx, hipMemcpyAsync(ctx->d_udp_off, offsets, (n + 1) * 8, hipMemcpyHostToDevice, s));
    // 1. unpack: the sizing call first, then into a buffer of that size (the count pass runs twice; it is the cheap half only for
    //    batches of bare records -- the price of not guessing a compression ratio)
    uint64_t total = 0;
    if ((rc = fg_udp_unpack_device(ctx, ctx->d_bytes, nbytes, ctx->d_udp_off, n, max_inflated, nullptr, 0, ctx->d_offsets, ctx->d_bad, ctx->d_udp_st,
                                   &total, FG_STREAM_OWN)) != FG_OK)
        return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_sl_packed, &ctx->d_sl_packed_cap, up(total, 16) + 16)) != FG_OK) return rc;
    if ((rc = fg_udp_unpack_device(ctx, ctx->d_bytes, nbytes, ctx->d_udp_off, n, max_inflated, ctx->d_sl_packed, total, ctx->d_offsets, ctx->d_bad,
                                   ctx->d_udp_st, &total, FG_STREAM_OWN)) != FG_OK)
        return rc;
    // (the decoders load 16 bytes at a time: the pad behind the last payload is zero, as behind an uploaded batch)
    FG_HIP(ctx, hipMemsetAsync(ctx->d_sl_packed + total, 0, up(total, 16) + 16 - total, s));
    // 2. the payloads, their offsets and the status back to the host
    const uint64_t lines_sz = up(total, 16) + 16, offs_sz = up((n + 1) * 8, 16), need = lines_sz + offs_sz + up(n, 16);
    if (need > ctx->h_udp_cap) {
        if (ctx->h_udp) FG_HIP(ctx, hipHostFree(ctx->h_udp));
        ctx->h_udp = nullptr;
        ctx->h_udp_cap = 0;
        const uint64_t want = up(need + need / 4, 1 << 16);
        FG_HIP(ctx, hipHostMalloc((void**)&ctx->h_udp, want, hipHostMallocDefault));
        ctx->h_udp_cap = want;
    }
    uint8_t* const h_lines = ctx->h_udp;
    uint64_t* const h_offs = (uint64_t*)(ctx->h_udp + lines_sz);
    uint8_t* const h_st = ctx->h_udp + lines_sz + offs_sz;
    if (total) FG_HIP(ctx, hipMemcpyAsync(h_lines, ctx->d_sl_packed, total, hipMemcpyDeviceToHost, s));
    FG_HIP(ctx, hipMemcpyAsync(h_offs, ctx->d_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    FG_HIP(ctx, hipMemcpyAsync(h_st, ctx->d_udp_st, n, hipMemcpyDeviceToHost, s));
    // 3. decode the payloads where they lie (as the second half of frame_decode_one_piece; the entry table is sized from what the batch
    //    inflated to)
    if ((rc = decode_stage_to_host(ctx, fmt, FG_FRAME_NONE, total, n, ctx->d_bad, ctx->d_sl_packed, out)) != FG_OK) return rc;
    *out_lines = h_lines;
    *out_line_offsets = h_offs;
    *udp_status = h_st;
    return FG_OK;
}

int fg_frame_decode_batch(fg_ctx* ctx, fg_format fmt, fg_framing framing, const uint8_t* bytes, uint64_t nbytes, int final,
                          fg_tables* out, const uint64_t** out_offsets, uint64_t* n_frames, uint64_t* consumed) {
    if (!ctx || !out || !out_offsets || !n_frames || !consumed || (nbytes && !bytes)) return FG_ERR_ARG;
    if (framing != FG_FRAME_LINE && framing != FG_FRAME_NUL && framing != FG_FRAME_SYSLEN && framing != FG_FRAME_CAPNP) return FG_ERR_UNSUPPORTED;
    if (framing == FG_FRAME_CAPNP && fmt != FG_CAPNP) return FG_ERR_ARG;
    if (framing == FG_FRAME_SYSLEN || framing == FG_FRAME_CAPNP) {  // (one piece: framed where the chunk lies -- syslen: and packed --, then decoded)
        const int rc = frame_decode_one_piece(ctx, fmt, framing, bytes, nbytes, final, out, out_offsets, n_frames, consumed);
        if (rc != FG_OK) ctx->last_host_path = 0;
        return rc;
    }
    {
        DeviceGuard g(ctx->device);
        *n_frames = 0;
        *consumed = 0;
        *out_offsets = nullptr;
        const int rc = frame_decode_fused(ctx, fmt, framing, bytes, nbytes, final, out, out_offsets, n_frames, consumed);
        if (rc != FG_ERR_UNSUPPORTED) return rc;
    }
    if (nbytes >= (48ull << 20) && !(ctx->lo.flags & FG_LO_TRANSCODE_ONE_PIECE)) {
        DeviceGuard g(ctx->device);
        *n_frames = 0;
        *consumed = 0;
        *out_offsets = nullptr;
        const int rc = frame_decode_sliced(ctx, fmt, framing, bytes, nbytes, final, out, out_offsets, n_frames, consumed);
        if (rc == FG_OK) ctx->last_host_path = FG_PATH_FRAME_SLICED;
        if (rc != FG_ERR_UNSUPPORTED) return rc;
    }
    const int rc1 = frame_decode_one_piece(ctx, fmt, framing, bytes, nbytes, final, out, out_offsets, n_frames, consumed);
    if (rc1 == FG_OK) ctx->last_host_path = FG_PATH_FRAME_ONE_PIECE;
    return rc1;
}

// Framing stage shared by fg_frame_decode_batch and fg_transcode_batch: the raw chunk is already in ctx->d_bytes
// (zero padded); fills ctx->d_offsets / ctx->d_bad and says how many frames the chunk holds and how many of its bytes
// they cover (an unterminated tail is a frame only when `final`).
static int frame_stage(fg_ctx* ctx, fg_framing framing, uint64_t nbytes, int final, uint64_t* n_frames, uint64_t* consumed) {
    uint64_t total = 0, last_end = 0;
    // capacity: one frame per 32 bytes to start with, exact on retry
    const int rc = frame_with_retry(nbytes / 32 + 1024, &total, [&](uint64_t cap) {
        int r;
        if ((r = grow_dev(ctx, (void**)&ctx->d_offsets, &ctx->d_offsets_cap, (cap + 2) * 8)) != FG_OK) return r;
        if ((r = grow_dev(ctx, (void**)&ctx->d_bad, &ctx->d_bad_cap, cap + 1)) != FG_OK) return r;
        return frame_scan(ctx, framing, ctx->d_bytes, nbytes, ctx->d_offsets, ctx->d_bad, cap, ctx->stream, &total, &last_end);
    });
    if (rc != FG_OK) return rc;
    const bool tail = last_end != nbytes;  // terminated frames = total
    *n_frames = total + ((tail && final) ? 1 : 0);
    *consumed = (tail && !final) ? last_end : nbytes;
    return FG_OK;
}

// Decode ctx->d_bytes / ctx->d_offsets into tables carved from ctx->d_tab, growing the entry table until it fits.
static int decode_stage(fg_ctx* ctx, fg_format fmt, fg_framing framing, uint64_t nbytes, uint64_t n, const uint8_t* d_bad,
                        fg_tables* dt, uint64_t* ent_used, const uint8_t* d_src = nullptr) {
    if (!d_src) d_src = ctx->d_bytes;
    hipStream_t s = ctx->stream;
    int rc;
    uint64_t ent_cap = first_ent_cap(fmt, nbytes);
    for (;;) {
        if ((rc = grow_dev(ctx, (void**)&ctx->d_tab, &ctx->d_tab_cap, carved_bytes(n, ent_cap))) != FG_OK) return rc;
        carve(ctx->d_tab, n, ent_cap, dt, nullptr);
        rc = fg_decode_frames_device(ctx, fmt, framing, d_src, nbytes, ctx->d_offsets, n, d_bad, dt, FG_STREAM_OWN);
        if (rc != FG_OK) return rc;
        uint64_t used = 0;
        FG_HIP(ctx, hipMemcpyAsync(&used, dt->ent_used, 8, hipMemcpyDeviceToHost, s));
        FG_HIP(ctx, hipStreamSynchronize(s));
        if (used > ent_cap) {
            if (ent_cap >= kEntCapMax) return FG_ERR_ENT_OVERFLOW;
            ent_cap = next_ent_cap(used);
            continue;
        }
        *ent_used = used;
        return FG_OK;
    }
}
// ... and the whole table into the ctx's pinned mirror: *out (host pointers) is complete when the call returns
static int decode_stage_to_host(fg_ctx* ctx, fg_format fmt, fg_framing framing, uint64_t nbytes, uint64_t n, const uint8_t* d_bad,
                                const uint8_t* d_src, fg_tables* out) {
    int rc;
    fg_tables dt, ht;
    uint64_t used = 0;
    if ((rc = decode_stage(ctx, fmt, framing, nbytes, n, d_bad, &dt, &used, d_src)) != FG_OK) return rc;
    if ((rc = grow_pinned(ctx, (void**)&ctx->h_tab, &ctx->h_tab_cap, carved_bytes(n, dt.ent_cap))) != FG_OK) return rc;
    carve(ctx->h_tab, n, dt.ent_cap, &ht, nullptr);
    if ((rc = copy_table(ctx, ht, dt, n, used, ctx->stream)) != FG_OK) return rc;
    FG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *out = ht;
    return FG_OK;
}

// ---- The chunks of MANY connections in one buffer (fg_frame_decode_multi_batch and its syslen / capnp siblings): upload once, frame every
// segment as its own stream, decode every slot, tables and per-segment / per-slot lists back.  One piece: a batch of connection chunks is
// far below the sizes from which the sliced forms pay.  What the three entries share lives here; each keeps its format check, its
// first capacity, its device call, its host hop and what its decode reads.
//   ctx->d_ms: seg_starts | seg_first | seg_consumed | a byte per segment (seg_final going in, or seg_stop coming out) | the cut's words
//   ctx->h_ms: seg_first | seg_consumed | seg_stop | a u64 per slot (n + 1) | a byte per slot (n)     <- what the out_* pointers name
// A front half (upload, device framer with retry, host hop on decline, the mirror) leaves a SegFramed; SegBatch::finish decodes it into
// host tables (the fg_frame_decode_*multi_batch entries), SegBatch::finish_transcode runs the transcode tail on it
// (fg_transcode_multi_batch).
static int transcode_tail(fg_ctx* ctx, fg_format fmt, fg_framing dec_framing, const fg_encode_cfg* ecfg, const uint8_t* d_src, uint64_t src_bytes,
                          uint64_t n, const uint8_t* d_bad, uint64_t in_bytes, bool frames, fg_transcoded* res);
static uint64_t transcoded_arrays(uint8_t* h, uint64_t base, uint64_t n, bool frames, fg_transcoded* out);
// what is to be decoded: n slots, ctx->d_offsets in d_src[0 .. used), ctx->d_bad nonzero -> FG_ST_BAD_UTF8 (not decoded)
struct SegFramed {
    uint64_t n = 0, used = 0;
    const uint8_t* d_src = nullptr;
    fg_framing framing = FG_FRAME_NONE;  // what the decode strips
    int path = 0;                        // FG_PATH_*
};
struct SegBatch {
    fg_ctx* ctx;
    uint64_t n_segs;
    // the caller's outputs; o_stop / o_slot8 null: the entry has no such column, and the mirror then has none either
    fg_tables* out;
    uint64_t* n_out;
    const uint64_t **o_first, **o_cons;
    const uint8_t** o_stop;
    const uint64_t** o_slot64;
    const uint8_t** o_slot8;
    hipStream_t s = nullptr;
    uint64_t *d_starts = nullptr, *d_first = nullptr, *d_cons = nullptr;
    uint8_t* d_seg8 = nullptr;
    uint32_t* d_cut = nullptr;  // n_segs + 1 words (fg_launch_syslen_cut)
    uint64_t *h_first = nullptr, *h_cons = nullptr, *h_slot64 = nullptr;
    uint8_t *h_stop = nullptr, *h_slot8 = nullptr;

    // seg_starts tiles [0, nbytes]: starts at 0, ends at nbytes, never steps back, every start but the last clear of `mask`
    static bool list_ok(const uint64_t* seg_starts, uint64_t n_segs, uint64_t nbytes, uint64_t mask) {
        if (n_segs && !seg_starts) return false;
        if (n_segs ? (seg_starts[0] != 0 || seg_starts[n_segs] != nbytes) : nbytes != 0) return false;
        for (uint64_t k = 0; k < n_segs; ++k)
            if (seg_starts[k] > seg_starts[k + 1] || (seg_starts[k] & mask) != 0) return false;
        return true;
    }
    void publish(uint64_t n) const {
        *n_out = n;
        *o_first = h_first;
        *o_cons = h_cons;
        *o_slot64 = h_slot64;
        if (o_stop) *o_stop = h_stop;
        if (o_slot8) *o_slot8 = h_slot8;
    }
    // clears the outputs; the bytes (zero padded), the starts and seg_final go up
    int upload(const uint8_t* bytes, uint64_t nbytes, const uint64_t* seg_starts, const uint8_t* seg_final) {
        *out = fg_tables{};
        publish(0);
        ctx->last_host_path = 0;
        s = ctx->stream;
        int rc;
        const uint64_t w = up((n_segs + 1) * 8, 256);
        if ((rc = grow_dev(ctx, (void**)&ctx->d_ms, &ctx->d_ms_cap, 3 * w + up(n_segs + 1, 256) + up((n_segs + 1) * 4, 256))) != FG_OK) return rc;
        if ((rc = grow_dev(ctx, (void**)&ctx->d_bytes, &ctx->d_bytes_cap, up(nbytes, 16) + 16)) != FG_OK) return rc;
        d_starts = reinterpret_cast<uint64_t*>(ctx->d_ms);
        d_first = reinterpret_cast<uint64_t*>(ctx->d_ms + w);
        d_cons = reinterpret_cast<uint64_t*>(ctx->d_ms + 2 * w);
        d_seg8 = ctx->d_ms + 3 * w;
        d_cut = reinterpret_cast<uint32_t*>(d_seg8 + up(n_segs + 1, 256));
        if (nbytes) FG_HIP(ctx, hipMemcpyAsync(ctx->d_bytes, bytes, nbytes, hipMemcpyHostToDevice, s));
        FG_HIP(ctx, hipMemsetAsync(ctx->d_bytes + nbytes, 0, up(nbytes, 16) + 16 - nbytes, s));
        if (n_segs) FG_HIP(ctx, hipMemcpyAsync(d_starts, seg_starts, (n_segs + 1) * 8, hipMemcpyHostToDevice, s));
        if (n_segs && seg_final) FG_HIP(ctx, hipMemcpyAsync(d_seg8, seg_final, n_segs, hipMemcpyHostToDevice, s));
        return FG_OK;
    }
    // Lays the mirror out for n slots and fills every column from its source: `device` -- device columns, copied on s and NOT waited
    // for --, else host arrays.  n64: the entries of the u64-per-slot column the source holds (the column has room for n + 1).
    int mirror(uint64_t n, uint64_t n64, const uint64_t* first, const uint64_t* cons, const uint8_t* stop, const uint64_t* slot64, const uint8_t* slot8,
               bool device) {
        const uint64_t w = up((n_segs + 1) * 8, 256), at64 = 2 * w + (o_stop ? up(n_segs + 1, 256) : 0), at8 = at64 + up((n + 1) * 8, 256);
        int rc;
        if ((rc = grow_pinned(ctx, (void**)&ctx->h_ms, &ctx->h_ms_cap, at8 + (o_slot8 ? up(n + 1, 256) : 0))) != FG_OK) return rc;
        uint8_t* const h = ctx->h_ms;
        h_first = reinterpret_cast<uint64_t*>(h);
        h_cons = reinterpret_cast<uint64_t*>(h + w);
        h_stop = o_stop ? h + 2 * w : nullptr;
        h_slot64 = reinterpret_cast<uint64_t*>(h + at64);
        h_slot8 = o_slot8 ? h + at8 : nullptr;
        auto put = [&](void* dst, const void* src, uint64_t bytes) -> int {
            if (bytes && device) FG_HIP(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
            else if (bytes) memcpy(dst, src, bytes);
            return FG_OK;
        };
        h_first[0] = h_slot64[0] = 0;  // (what a call without segments / a column nobody filled reads as)
        if ((rc = put(h_first, first, n_segs ? (n_segs + 1) * 8 : 0)) != FG_OK || (rc = put(h_cons, cons, n_segs * 8)) != FG_OK) return rc;
        if (o_stop && (rc = put(h_stop, stop, n_segs)) != FG_OK) return rc;
        if ((rc = put(h_slot64, slot64, n64 * 8)) != FG_OK) return rc;
        return o_slot8 ? put(h_slot8, slot8, n) : FG_OK;
    }
    // the mirror goes out, and the slots are decoded into host tables
    int finish(const SegFramed& f, fg_format fmt) {
        publish(f.n);
        ctx->last_host_path = f.path;
        if (f.n == 0) {
            FG_HIP(ctx, hipStreamSynchronize(s));  // (the mirror's copies)
            return FG_OK;
        }
        const int rc = decode_stage_to_host(ctx, fmt, f.framing, f.used, f.n, ctx->d_bad, f.d_src, out);
        if (rc != FG_OK) ctx->last_host_path = 0;
        return rc;
    }
    // ... or decoded into HBM and encoded from there: *res = the stream and the verdicts in ctx->h_tout, complete when the call returns
    // (in_bytes: the buffer's size, from which the first output buffer of a ctx is sized)
    int finish_transcode(const SegFramed& f, fg_format fmt, const fg_encode_cfg* ecfg, uint64_t in_bytes, fg_transcoded* res) {
        publish(f.n);
        ctx->last_host_path = f.path;
        *res = fg_transcoded{};
        res->n = f.n;
        int rc;
        if (f.n == 0) {  // an empty stream: out_offsets[0] = 0
            if ((rc = grow_pinned(ctx, (void**)&ctx->h_tout, &ctx->h_tout_cap, transcoded_arrays(nullptr, 0, 0, false, res))) == FG_OK) {
                transcoded_arrays(ctx->h_tout, 0, 0, false, res);
                *reinterpret_cast<uint64_t*>(ctx->h_tout) = 0;
                res->out = ctx->h_tout;
            }
        } else {
            rc = transcode_tail(ctx, fmt, f.framing, ecfg, f.d_src, f.used, f.n, ctx->d_bad, in_bytes, false, res);
        }
        if (rc == FG_OK) {
            const hipError_t e = hipStreamSynchronize(s);  // (the mirror's copies, the tail's downloads)
            if (e != hipSuccess) {
                ctx->last_hip = (int)e;
                rc = FG_ERR_HIP;
            }
        }
        if (rc != FG_OK) ctx->last_host_path = 0;
        return rc;
    }
};
static bool text_format(fg_format fmt) { return fmt == FG_RFC5424 || fmt == FG_LTSV || fmt == FG_GELF || fmt == FG_RFC3164; }

// Lines / NUL: CARRY and BAD_UTF8 slots are skipped rows; the slots are decoded where they lie (terminators stripped in-kernel).
static int lines_multi_args(fg_format fmt, fg_framing framing, uint64_t nbytes, const uint64_t* seg_starts, uint64_t n_segs) {
    if ((framing != FG_FRAME_LINE && framing != FG_FRAME_NUL) || !text_format(fmt)) return FG_ERR_ARG;
    return SegBatch::list_ok(seg_starts, n_segs, nbytes, 0) ? FG_OK : FG_ERR_ARG;
}
static int lines_multi_front(SegBatch& b, fg_framing framing, const uint8_t* bytes, uint64_t nbytes, const uint64_t* seg_starts, const uint8_t* seg_final,
                             SegFramed* f) {
    fg_ctx* const ctx = b.ctx;
    const uint64_t n_segs = b.n_segs;
    int rc;
    if ((rc = b.upload(bytes, nbytes, seg_starts, seg_final)) != FG_OK) return rc;
    // capacity: one slot per 32 bytes and one tail per segment to start with (as frame_stage)
    uint64_t n = 0;
    rc = frame_with_retry(nbytes / 32 + n_segs + 1024, &n, [&](uint64_t cap) {
        int r;
        if ((r = grow_dev(ctx, (void**)&ctx->d_offsets, &ctx->d_offsets_cap, (cap + 2) * 8)) != FG_OK) return r;
        if ((r = grow_dev(ctx, (void**)&ctx->d_bad, &ctx->d_bad_cap, cap + 1)) != FG_OK) return r;
        return fg_frame_multi_device(ctx, framing, ctx->d_bytes, nbytes, b.d_starts, seg_final ? b.d_seg8 : nullptr, n_segs, ctx->d_offsets, ctx->d_bad, cap,
                                     b.d_first, b.d_cons, &n, FG_STREAM_OWN);
    });
    if (rc != FG_OK) return rc;
    // (an empty buffer: the device entry leaves the offsets alone)
    if ((rc = b.mirror(n, nbytes && n_segs ? n + 1 : 0, b.d_first, b.d_cons, nullptr, ctx->d_offsets, ctx->d_bad, true)) != FG_OK) return rc;
    *f = SegFramed{n, nbytes, ctx->d_bytes, framing, FG_PATH_FRAME_MULTI};
    return FG_OK;
}
extern "C" int fg_frame_decode_multi_batch(fg_ctx* ctx, fg_format fmt, fg_framing framing, const uint8_t* bytes, uint64_t nbytes,
                                           const uint64_t* seg_starts, const uint8_t* seg_final, uint64_t n_segs, fg_tables* out,
                                           const uint64_t** out_offsets, const uint8_t** out_kind, const uint64_t** out_seg_first,
                                           const uint64_t** out_seg_consumed, uint64_t* n_slots) {
    if (!ctx || !out || !out_offsets || !out_kind || !out_seg_first || !out_seg_consumed || !n_slots || (nbytes && !bytes)) return FG_ERR_ARG;
    if (lines_multi_args(fmt, framing, nbytes, seg_starts, n_segs) != FG_OK) return FG_ERR_ARG;
    SegBatch b{ctx, n_segs, out, n_slots, out_seg_first, out_seg_consumed, nullptr, out_offsets, out_kind};
    DeviceGuard g(ctx->device);
    SegFramed f;
    const int rc = lines_multi_front(b, framing, bytes, nbytes, seg_starts, seg_final, &f);
    return rc != FG_OK ? rc : b.finish(f, fmt);
}

// OCTET-COUNTED chunks (a SyslenSplitter per connection, syslen_splitter.rs:42-57): framed AND packed on the device; what is decoded is the
// packed batch (FG_FRAME_NONE, with the UTF-8 flags).  When the device framer declines (fg_frame_syslen_multi_device: FG_ERR_UNSUPPORTED)
// or a segment meets a prefix beyond the device parser's bound, the whole buffer is hopped on the host, segment by segment, and the
// packed batch is uploaded: the same results either way (the two simplifications of syslen_stage hold here too).
// THE CUT (fg_transcode_multi_batch, whose mirror has the byte per slot; the decode entry flags every bad payload and leaves the rest to
// its caller): SyslenSplitter::run unwraps String::from_utf8 (syslen_splitter.rs:33), so a segment's first payload that is not UTF-8 ends
// its connection -- it stays FG_SLOT_BAD_UTF8 and every frame of the segment behind it becomes FG_SLOT_UNREACHED, a skipped row like it.
// On the device between the framer and the mirror (fg_launch_syslen_cut), on the host in the hop.
static void syslen_cut_host(uint8_t* bad, const uint64_t* first, uint64_t n_segs) {
    for (uint64_t k = 0; k < n_segs; ++k) {
        bool over = false;
        for (uint64_t i = first[k]; i < first[k + 1]; ++i) {
            if (over) bad[i] = FG_SLOT_UNREACHED;
            else over = bad[i] != 0;
        }
    }
}
static int syslen_multi_args(fg_format fmt, uint64_t nbytes, const uint64_t* seg_starts, uint64_t n_segs) {
    return text_format(fmt) && SegBatch::list_ok(seg_starts, n_segs, nbytes, 0) ? FG_OK : FG_ERR_ARG;
}
static int syslen_multi_front(SegBatch& b, const uint8_t* bytes, uint64_t nbytes, const uint64_t* seg_starts, SegFramed* f) {
    fg_ctx* const ctx = b.ctx;
    const uint64_t n_segs = b.n_segs;
    const bool cut = b.o_slot8 != nullptr;
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_sl_packed, &ctx->d_sl_packed_cap, up(nbytes, 16) + 16)) != FG_OK) return rc;
    if ((rc = b.upload(bytes, nbytes, seg_starts, nullptr)) != FG_OK) return rc;
    auto ensure = [&](uint64_t cap) -> int {
        int r;
        if ((r = grow_dev(ctx, (void**)&ctx->d_offsets, &ctx->d_offsets_cap, (cap + 2) * 8)) != FG_OK) return r;
        if ((r = grow_dev(ctx, (void**)&ctx->d_sl_starts, &ctx->d_sl_starts_cap, (cap + 2) * 8)) != FG_OK) return r;
        return grow_dev(ctx, (void**)&ctx->d_bad, &ctx->d_bad_cap, cap + 1);
    };
    // capacity from the frames per byte this ctx last saw (as syslen_stage)
    uint64_t n = 0, payload = 0;
    rc = frame_with_retry((uint64_t)((double)nbytes * ctx->frames_per_byte * 1.25) + 1024, &n, [&](uint64_t cap) {
        const int r = ensure(cap);
        return r != FG_OK ? r : fg_frame_syslen_multi_device(ctx, ctx->d_bytes, nbytes, b.d_starts, n_segs, ctx->d_sl_packed, ctx->d_offsets, ctx->d_sl_starts,
                                                             ctx->d_bad, cap, b.d_first, b.d_cons, b.d_seg8, &n, &payload, FG_STREAM_OWN);
    });
    if (rc != FG_OK && rc != FG_ERR_UNSUPPORTED) return rc;
    bool device = rc == FG_OK;
    if (device) {
        const bool cut_here = cut && fg_launch_syslen_cut;  // (on the ctx's stream, in front of the mirror's copy of the verdicts)
        if (cut_here) FG_LAUNCH(ctx, fg_launch_syslen_cut(ctx->d_bad, n, b.d_first, n_segs, b.d_cut, s));
        if ((rc = b.mirror(n, n, b.d_first, b.d_cons, b.d_seg8, ctx->d_sl_starts, cut ? ctx->d_bad : nullptr, true)) != FG_OK) return rc;
        // (the decoders load 16 bytes at a time: the pad behind the last payload is zero, as behind an uploaded batch)
        FG_HIP(ctx, hipMemsetAsync(ctx->d_sl_packed + payload, 0, up(payload, 16) + 16 - payload, s));
        FG_HIP(ctx, hipStreamSynchronize(s));
        for (uint64_t k = 0; k < n_segs && device; ++k) device = b.h_stop[k] != FG_SYSLEN_LONG_PREFIX;
        if (device && cut && !cut_here && n) {  // a build without the kernel: from the mirrored verdicts, and back (pinned: may stay in flight)
            syslen_cut_host(b.h_slot8, b.h_first, n_segs);
            FG_HIP(ctx, hipMemcpyAsync(ctx->d_bad, b.h_slot8, n, hipMemcpyHostToDevice, s));
        }
    }
    if (!device) {
        SyslenHop hop;
        std::vector<uint64_t> first{0}, cons(n_segs);
        std::vector<uint8_t> stop;
        for (uint64_t k = 0; k < n_segs; ++k) {
            stop.push_back((uint8_t)hop.walk(bytes, seg_starts[k], seg_starts[k + 1] - seg_starts[k], &cons[k]));
            first.push_back(hop.starts.size());
        }
        n = hop.starts.size();
        payload = hop.packed.size();
        if (cut) syslen_cut_host(hop.bad.data(), first.data(), n_segs);  // (before the verdicts are mirrored and uploaded)
        if ((rc = ensure(n)) != FG_OK) return rc;
        if ((rc = b.mirror(n, n, first.data(), cons.data(), stop.data(), hop.starts.data(), cut ? hop.bad.data() : nullptr, false)) != FG_OK) return rc;
        if ((rc = hop.upload(ctx, s)) != FG_OK) return rc;
        FG_HIP(ctx, hipStreamSynchronize(s));  // (the vectors go out of scope)
    }
    if (n && nbytes >= (1u << 20)) ctx->frames_per_byte = (double)n / (double)nbytes;
    *f = SegFramed{n, payload, ctx->d_sl_packed, FG_FRAME_NONE, device ? FG_PATH_FRAME_SYSLEN_MULTI_DEVICE : FG_PATH_FRAME_SYSLEN_MULTI_HOST};
    return FG_OK;
}
extern "C" int fg_frame_decode_syslen_multi_batch(fg_ctx* ctx, fg_format fmt, const uint8_t* bytes, uint64_t nbytes, const uint64_t* seg_starts,
                                                  uint64_t n_segs, fg_tables* out, const uint64_t** out_frame_starts,
                                                  const uint64_t** out_seg_first, const uint64_t** out_seg_consumed,
                                                  const uint8_t** out_seg_stop, uint64_t* n_frames) {
    if (!ctx || !out || !out_frame_starts || !out_seg_first || !out_seg_consumed || !out_seg_stop || !n_frames || (nbytes && !bytes)) return FG_ERR_ARG;
    if (syslen_multi_args(fmt, nbytes, seg_starts, n_segs) != FG_OK) return FG_ERR_ARG;
    SegBatch b{ctx, n_segs, out, n_frames, out_seg_first, out_seg_consumed, out_seg_stop, out_frame_starts, nullptr};
    DeviceGuard g(ctx->device);
    SegFramed f;
    const int rc = syslen_multi_front(b, bytes, nbytes, seg_starts, &f);
    return rc != FG_OK ? rc : b.finish(f, fmt);
}

// CAP'N PROTO chunks (a CapnpSplitter per connection, capnp_splitter.rs:24-46): the messages are decoded where they lie, with the slot
// kinds as the skip array (a CARRY slot is a skipped row).  When the device framer declines (fg_frame_capnp_multi_device:
// FG_ERR_UNSUPPORTED) the segments are walked on the host over the caller's bytes and the slots are uploaded: the same results either way.
static int capnp_multi_args(uint64_t nbytes, const uint64_t* seg_starts, uint64_t n_segs) {
    if (!SegBatch::list_ok(seg_starts, n_segs, nbytes, 7)) return FG_ERR_ARG;  // (the framer works on words of the buffer)
    return nbytes > FG_CAPNP_FRAME_MAX_BYTES || n_segs > (1ull << 24) ? FG_ERR_ARG : FG_OK;
}
static int capnp_multi_front(SegBatch& b, const uint8_t* bytes, uint64_t nbytes, const uint64_t* seg_starts, SegFramed* f) {
    fg_ctx* const ctx = b.ctx;
    const uint64_t n_segs = b.n_segs;
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = b.upload(bytes, nbytes, seg_starts, nullptr)) != FG_OK) return rc;
    auto ensure = [&](uint64_t cap) -> int {
        const int r = grow_dev(ctx, (void**)&ctx->d_offsets, &ctx->d_offsets_cap, (cap + 2) * 8);
        return r != FG_OK ? r : grow_dev(ctx, (void**)&ctx->d_bad, &ctx->d_bad_cap, cap + 1);
    };
    // capacity: a message of the record schema is a few hundred bytes (as capnp_stage), one tail per segment
    uint64_t n = 0;
    rc = frame_with_retry(nbytes / 64 + n_segs + 1024, &n, [&](uint64_t cap) {
        const int r = ensure(cap);
        return r != FG_OK ? r : fg_frame_capnp_multi_device(ctx, ctx->d_bytes, nbytes, b.d_starts, n_segs, ctx->d_offsets, ctx->d_bad, cap, b.d_first, b.d_cons,
                                                            b.d_seg8, &n, FG_STREAM_OWN);
    });
    if (rc == FG_OK) {
        if ((rc = b.mirror(n, n + 1, b.d_first, b.d_cons, b.d_seg8, ctx->d_offsets, ctx->d_bad, true)) != FG_OK) return rc;
        *f = SegFramed{n, nbytes, ctx->d_bytes, FG_FRAME_NONE, FG_PATH_FRAME_CAPNP_MULTI_DEVICE};
        return FG_OK;
    }
    if (rc != FG_ERR_UNSUPPORTED) return rc;
    std::vector<uint64_t> offs, first{0}, cons(n_segs);
    std::vector<uint8_t> kind, stop;
    for (uint64_t k = 0; k < n_segs; ++k) {
        const uint64_t at = seg_starts[k], len = seg_starts[k + 1] - at;
        stop.push_back((uint8_t)capnp_hop(bytes, at, len, &cons[k], offs));
        kind.resize(offs.size(), FG_SLOT_FRAME);
        if (cons[k] < len) {
            offs.push_back(at + cons[k]);
            kind.push_back(FG_SLOT_CARRY);
        }
        first.push_back(kind.size());
    }
    offs.push_back(nbytes);
    n = kind.size();
    if ((rc = ensure(n)) != FG_OK) return rc;
    if ((rc = b.mirror(n, n + 1, first.data(), cons.data(), stop.data(), offs.data(), kind.data(), false)) != FG_OK) return rc;
    // (from the pinned mirror: the vectors may go out of scope while these are in flight)
    FG_HIP(ctx, hipMemcpyAsync(ctx->d_offsets, b.h_slot64, (n + 1) * 8, hipMemcpyHostToDevice, s));
    if (n) FG_HIP(ctx, hipMemcpyAsync(ctx->d_bad, b.h_slot8, n, hipMemcpyHostToDevice, s));
    *f = SegFramed{n, nbytes, ctx->d_bytes, FG_FRAME_NONE, FG_PATH_FRAME_CAPNP_MULTI_HOST};
    return FG_OK;
}
extern "C" int fg_frame_decode_capnp_multi_batch(fg_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, const uint64_t* seg_starts, uint64_t n_segs,
                                                 fg_tables* out, const uint64_t** out_offsets, const uint8_t** out_kind,
                                                 const uint64_t** out_seg_first, const uint64_t** out_seg_consumed, const uint8_t** out_seg_stop,
                                                 uint64_t* n_slots) {
    if (!ctx || !out || !out_offsets || !out_kind || !out_seg_first || !out_seg_consumed || !out_seg_stop || !n_slots || (nbytes && !bytes))
        return FG_ERR_ARG;
    if (capnp_multi_args(nbytes, seg_starts, n_segs) != FG_OK) return FG_ERR_ARG;
    SegBatch b{ctx, n_segs, out, n_slots, out_seg_first, out_seg_consumed, out_seg_stop, out_offsets, out_kind};
    DeviceGuard g(ctx->device);
    SegFramed f;
    const int rc = capnp_multi_front(b, bytes, nbytes, seg_starts, &f);
    return rc != FG_OK ? rc : b.finish(f, FG_CAPNP);
}

// The fixed arrays of an fg_transcoded -- out_offsets | meta | enc_status [| frame offsets] -- from byte `base` of the pinned block h:
// *out's pointers name them (h null: only their size is asked for); -> the byte behind them.  The messages lie in front of them in
// the one-piece form and behind them in the sliced one, where they grow slice by slice.
static uint64_t transcoded_arrays(uint8_t* h, uint64_t base, uint64_t n, bool frames, fg_transcoded* out) {
    const uint64_t offs_bytes = up((n + 1) * 8, 256);
    const uint64_t o_meta = base + offs_bytes, o_st = o_meta + up(n * 4, 256), o_frames = o_st + up(n, 256);
    if (h) {
        out->out_offsets = reinterpret_cast<const uint64_t*>(h + base);
        out->meta = reinterpret_cast<const uint32_t*>(h + o_meta);
        out->enc_status = h + o_st;
        out->frame_offsets = frames ? reinterpret_cast<const uint64_t*>(h + o_frames) : nullptr;
    }
    return o_frames + (frames ? offs_bytes : 0);
}

// fg_transcode_batch for a LARGE batch of framed lines: the batch goes through H2D -> decode -> encode -> D2H as slices of ~32 MiB
// on the ctx's two streams, so that the upload of slice k+1 and the (2-3x larger) download of slice k's messages share the
// full-duplex link, and the kernels hide behind both.  The host only waits for one small number per slice (its encoded size:
// the next slice's messages start there).  Returns FG_ERR_UNSUPPORTED when the batch must take the one-piece path (an output
// estimate that turned out too small): nothing has been returned to the caller by then.
static int transcode_sliced(fg_ctx* ctx, fg_format fmt, const fg_encode_cfg* ecfg, const uint8_t* bytes, uint64_t nbytes,
                            const uint64_t* offsets, uint64_t n, fg_transcoded* out) {
    int rc;
    if (n < 64) return FG_ERR_UNSUPPORTED;
    // Slices that GROW: 4, 8, 16, 32 MiB, then 64 MiB each (a sixtieth of the batch beyond 4 GiB).  The download direction is the bound (the
    // GELF text is 2.4x the input) and it cannot start before the first slice is uploaded, decoded, counted, scanned and written:
    // 1.7 ms of a 13 ms call with a 32 MiB first slice, a quarter of a millisecond with 4 MiB.
    std::vector<uint64_t> cut{0};
    {
        const uint64_t steady = nbytes / 60u > (64ull << 20) ? nbytes / 60u : (64ull << 20);
        uint64_t piece = 4ull << 20, at = offsets[0];
        while (cut.back() < n) {
            at += piece;
            uint64_t line = (uint64_t)(std::upper_bound(offsets, offsets + n + 1, at) - offsets);
            line = line ? line - 1 : 0;  // the last line that starts at or before `at`
            if (line <= cut.back()) line = cut.back() + 1;
            if (line >= n || offsets[n] - offsets[line] < piece / 2u) line = n;
            cut.push_back(line);
            at = offsets[line];
            if (piece < steady) piece = piece * 2u < steady ? piece * 2u : steady;
        }
    }
    const uint32_t slices = (uint32_t)(cut.size() - 1);
    // One stream per direction of the link (round 6; rounds 3-5 ran two lanes, each with its own upload, kernels and download).  The
    // timeline of one call (profiles/r06ae_transcode_timeline.json) showed what two lanes cost: whenever both lanes had a copy of the
    // SAME direction in flight the runtime moved the second with a blit KERNEL, copies and kernels of a lane waited for each other, and
    // the two directions were never busy together.  Now:
    //   s_up    upload k, decode k, count k, upload k + 1, ... -- all queued at once, nothing on it waits for the host; the upload
    //           direction has time to spare (the text is 2.4x the input), so the kernels may sit between two uploads
    //   s_run   what hangs on the host's one number per slice: scan k -> the slice's size -> write k.  A write never queues behind the
    //           decode of a later slice: kernels crawl while a download saturates the link's write queue (k_rfc5424 0.03 -> 0.6-1.0 ms
    //           per slice), and only the write is on the download's critical path
    //   s_down  every download, in slice order
    // (three streams, not four: with a fourth the runtime put it on the hardware queue of s_down and every download waited for the
    //  last upload -- profiles/r06ai_transcode_timeline.json)
    if ((rc = ensure_pipeline(ctx, slices * 2u)) != FG_OK) return rc;  // (four events per slice)
    const hipStream_t s_up = ctx->s_up, s_run = ctx->s_run, s_down = ctx->s_down;
    if ((rc = ensure_h_cnt(ctx)) != FG_OK) return rc;
    std::vector<hipEvent_t>& ev = ctx->ev_slice;  // [4k + 1] slice k is decoded and counted, [4k + 2] its messages are written
    TableShares shares(ctx, slices);
    // ---- device buffers: input, tables (whole batch), out_offsets / enc_status, encoder scratch ----
    if ((rc = grow_dev(ctx, (void**)&ctx->d_bytes, &ctx->d_bytes_cap, up(nbytes, 16) + 16)) != FG_OK) return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_offsets, &ctx->d_offsets_cap, (n + 1) * 8)) != FG_OK) return rc;
    const uint64_t ent_cap = first_ent_cap(fmt, nbytes);
    if ((rc = grow_dev(ctx, (void**)&ctx->d_tab, &ctx->d_tab_cap, carved_bytes(n, ent_cap))) != FG_OK) return rc;
    fg_tables dt{};
    carve(ctx->d_tab, n, ent_cap, &dt, nullptr);
    const uint64_t offs_bytes = up((n + 1) * 8, 256);
    if ((rc = grow_dev(ctx, (void**)&ctx->d_tmeta, &ctx->d_tmeta_cap, offs_bytes + up(n, 256))) != FG_OK) return rc;
    uint64_t* d_out_offsets = reinterpret_cast<uint64_t*>(ctx->d_tmeta);
    uint8_t* d_enc_status = ctx->d_tmeta + offs_bytes;
    EncStage enc;  // (a run of block sums per slice: one word more each)
    if ((rc = stage_encoder(ctx, fmt, ecfg, n, n / 64 + slices + 2, &enc)) != FG_OK) return rc;
    std::vector<uint8_t> image(enc.image_bytes);
    enc.write_image(image.data());
    uint64_t first_used = ~0ull, used = 0;  // (read back from the device)
    DrainGuard drained(ctx);
    FG_HIP(ctx, hipMemcpyAsync(ctx->d_enc, image.data(), image.size(), hipMemcpyHostToDevice, s_run));
    FG_HIP(ctx, hipMemcpyAsync(ctx->d_offsets, offsets, (n + 1) * 8, hipMemcpyHostToDevice, s_run));
    FG_HIP(ctx, hipMemsetAsync(dt.ent_used, 0, 8, s_run));
    FG_HIP(ctx, hipStreamSynchronize(s_run));  // (the decodes on s_up read the offsets)
    fg::EncCfg& cfg = enc.cfg;
    const uint32_t cfg_lds = enc.cfg_lds;
    uint32_t* const d_sizes = enc.d_sizes;
    uint64_t* const d_block_sums = enc.d_block_sums;
    const uint32_t tile_cap = pick_tile_cap(ctx, nbytes, n, 40 * 1024, 1);
    fg::DevTables ddt = to_dev(dt);
    // ---- host buffer: fixed-size arrays first, the messages behind them (they grow slice by slice) ----
    fg_transcoded res{};
    const uint64_t o_msgs = transcoded_arrays(nullptr, 0, n, false, &res);
    uint64_t base = 0;  // encoded bytes of the slices finished so far
    auto sl_tables = [&](uint64_t l0, uint64_t l1) { return fg::rows_of(dt, l0, l1 - l0); };
    auto blocks_before = [&](uint32_t k) { return cut[k] / 64 + k; };  // first scratch sum of slice k (disjoint per slice)
    // queue a slice's upload, decode and count kernel (sixteen-byte aligned cuts: a slice starts with the sixteen bytes its first line begins in)
    auto enqueue = [&](uint32_t k) -> int {
        const uint64_t l0 = cut[k], l1 = cut[k + 1];
        if (l1 == l0) return FG_OK;
        const uint64_t b0 = offsets[l0] & ~15ull, b1 = offsets[l1];
        if (b1 > b0) FG_HIP(ctx, hipMemcpyAsync(ctx->d_bytes + b0, bytes + b0, b1 - b0, hipMemcpyHostToDevice, s_up));
        const fg_tables sl = sl_tables(l0, l1);
        int r = fg_decode_frames_impl(ctx, fmt, FG_FRAME_NONE, ctx->d_bytes, nbytes, ctx->d_offsets + l0, l1 - l0, nullptr, &sl, (void*)s_up, false,
                                   offsets[l1] - offsets[l0], k & 1u);
        if (r != FG_OK) return r;
        if (k == 0 && ecfg->encoder == FG_ENC_GELF) {  // the GELF ranking scratch is sized by the pairs per line: look at the first slice
            FG_HIP(ctx, hipMemcpyAsync(&first_used, dt.ent_used, 8, hipMemcpyDeviceToHost, s_up));
            FG_HIP(ctx, hipStreamSynchronize(s_up));
            pick_sort_slots(&cfg, first_used, l1 - l0);
        }
        fg::DevTables sdt = to_dev(sl);
        sdt.ent_cap = ddt.ent_cap;
        FG_LAUNCH(ctx, fg_launch_encode_count(ctx->d_bytes, ctx->d_offsets + l0, l1 - l0, &sdt, &cfg, tile_cap, cfg_lds, d_sizes + l0,
                                              d_block_sums + blocks_before(k), d_enc_status + l0, s_up));
        FG_HIP(ctx, hipEventRecord(ev[4 * k + 1], s_up));
        return FG_OK;
    };
    // (a few slices ahead of the one being finished, not all at once: the forty API calls of a slice take the host a tenth of a
    //  millisecond, and thirty slices queued before the first scan kept the first download waiting for four)
    LookAhead window(slices, 3);
    for (uint32_t k = 0; k < slices; ++k) {
        if ((rc = window.fill(k, enqueue)) != FG_OK) return rc;

        // ---- finish slice k: offsets from `base`, its size (the host waits for that one number), the write kernel, the download ----
        const uint64_t l0 = cut[k], l1 = cut[k + 1], rows = l1 - l0;
        if (rows == 0) continue;
        FG_HIP(ctx, hipStreamWaitEvent(s_run, ev[4 * k + 1], 0));
        FG_LAUNCH(ctx, fg_launch_encode_scan(d_sizes + l0, d_block_sums + blocks_before(k), rows, d_out_offsets + l0, base, s_run));
        uint64_t* const h_end = ctx->h_cnt + kCntEnd;
        FG_HIP(ctx, hipMemcpyAsync(h_end, d_out_offsets + l1, 8, hipMemcpyDeviceToHost, s_run));
        FG_HIP(ctx, hipEventRecord(ctx->ev_ready, s_run));
        FG_HIP(ctx, hipEventSynchronize(ctx->ev_ready));
        const uint64_t end = *h_end;
        if (k == 0) {
            // size the output buffers from the first slice (+ 12 %); a batch that outgrows the estimate takes the one-piece path
            const uint64_t in0 = offsets[l1] - offsets[l0];
            const uint64_t est = (uint64_t)((double)end * ((double)nbytes / (double)(in0 ? in0 : 1)) * 1.12) + (4ull << 20);
            if ((rc = grow_dev(ctx, (void**)&ctx->d_tout, &ctx->d_tout_cap, est)) != FG_OK) return rc;
            if ((rc = grow_pinned(ctx, (void**)&ctx->h_tout, &ctx->h_tout_cap, o_msgs + est)) != FG_OK) return rc;
        }
        if (end > ctx->d_tout_cap || o_msgs + end > ctx->h_tout_cap) return FG_ERR_UNSUPPORTED;
        const fg_tables sl = sl_tables(l0, l1);
        fg::DevTables sdt = to_dev(sl);
        sdt.ent_cap = ddt.ent_cap;
        FG_LAUNCH(ctx, fg_launch_encode_write(ctx->d_bytes, ctx->d_offsets + l0, rows, &sdt, &cfg, tile_cap, cfg_lds, d_out_offsets + l0, ctx->d_tout, d_sizes + l0, s_run));
        // (the downloads stay with hipMemcpyAsync: a copy kernel of the library's own through the buffer's device view -- one wave per
        //  CU, eight 16-byte accesses in flight per lane -- moved a slice no faster than the runtime's blit kernel, 50 vs 52 GB/s, and
        //  slowed the kernels beside it just the same: it is the link's write queue that holds them up, not the CUs the copy takes)
        // at most three downloads queued: a stream's packets share a hardware queue with another stream's, and two dozen downloads
        // queued ahead held the uploads behind them up for 45 ms (4 M lines, profiles/r06al_transcode_host_trace.log)
        if (k >= 3u) FG_HIP(ctx, hipEventSynchronize(ev[4 * (k - 3u) + 3]));
        FG_HIP(ctx, hipEventRecord(ev[4 * k + 2], s_run));
        FG_HIP(ctx, hipStreamWaitEvent(s_down, ev[4 * k + 2], 0));
        if (end > base) FG_HIP(ctx, hipMemcpyAsync(ctx->h_tout + o_msgs + base, ctx->d_tout + base, end - base, hipMemcpyDeviceToHost, s_down));
        FG_HIP(ctx, hipEventRecord(ev[4 * k + 3], s_down));
        base = end;
    }
    // the fixed-size arrays -- offsets, meta, status of every line -- in three copies behind the last slice's messages (per slice they
    // were three more launches between two downloads: a tenth of a millisecond of an idle link per slice)
    uint8_t* const hh = ctx->h_tout;
    transcoded_arrays(hh, 0, n, false, &res);
    FG_HIP(ctx, hipStreamWaitEvent(s_down, ev[4 * (slices - 1u) + 2], 0));
    FG_HIP(ctx, hipMemcpyAsync((void*)res.out_offsets, d_out_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, s_down));
    FG_HIP(ctx, hipMemcpyAsync((void*)res.meta, dt.meta, n * 4, hipMemcpyDeviceToHost, s_down));
    FG_HIP(ctx, hipMemcpyAsync((void*)res.enc_status, d_enc_status, n, hipMemcpyDeviceToHost, s_down));
    if ((rc = drained.done()) != FG_OK) return rc;
    // an entry table that was too small shows up as FG_ST_OVERFLOW rows: the one-piece path sizes it exactly
    FG_HIP(ctx, hipMemcpy(&used, dt.ent_used, 8, hipMemcpyDeviceToHost));
    if (used > ent_cap) return FG_ERR_UNSUPPORTED;
    res.n = n;
    res.consumed = nbytes;
    res.out = hh + o_msgs;
    res.out_bytes = base;
    *out = res;
    return FG_OK;
}

namespace {
// ctx->d_df_cut, for n messages: start flags | sums | ranks[n + 1] | member_first[n + 2] | cuts[n + 2] | z_offsets[n + 2] | the member count
struct MemberCuts {
    uint32_t* d_flags;
    uint64_t *d_sums, *d_idx, *d_first, *d_cuts, *d_zoff, *d_count, bytes;
    MemberCuts(uint8_t* b, uint64_t n) {
        Carver c{b};
        d_flags = c.take<uint32_t>(n);
        d_sums = c.take<uint64_t>((n + 63) / 64);
        d_idx = c.take<uint64_t>(n + 2, 8);
        d_first = c.take<uint64_t>(n + 2, 8);
        d_cuts = c.take<uint64_t>(n + 2, 8);
        d_zoff = c.take<uint64_t>(n + 2, 8);
        d_count = c.take<uint64_t>(1);
        bytes = c.off;
    }
};
// ctx->d_kf_off (FG_WIRE_KAFKA_V0), for n messages: three lists of n + 2 words each -- set_offsets (n + 1 of them written) | set_cuts |
// w_offsets (n_members + 1 <= n + 1 written of either)
struct KfOffsets {
    uint64_t *d_set_off, *d_set_cuts, *d_woff, bytes;
    KfOffsets(uint8_t* b, uint64_t n) {
        Carver c{b};
        d_set_off = c.take<uint64_t>(n + 2, 8);
        d_set_cuts = c.take<uint64_t>(n + 2, 8);
        d_woff = c.take<uint64_t>(n + 2, 8);
        bytes = c.off;
    }
};
}  // namespace

// The member stage of a transcode, behind the encoder whenever the wire is not FG_WIRE_RAW or a codec is set (fg_set_output_wire,
// fg_set_output_compression): members in the place of the messages.  The `total` bytes of ctx->d_tout, whose n messages d_out_offsets
// bounds (d_enc_status nonzero: a row that is in no message set), become
//   1. members, cut by the ctx's policy over the messages' offsets -- whatever follows, member_first is the same;
//   2. FG_WIRE_KAFKA_V0: the message set built from ctx->d_tout, the members' byte cuts in it set_offsets[member_first[k]] (the cuts[]
//      of step 1 are the plain stream's and unused then);
//   3. FG_COMP_GZIP: what step 2 left -- the set, else the plain stream -- deflated member by member, and with Kafka every non-empty
//      member wrapped in its message;
//   4. the bytes, their bounds and member_first downloaded into ctx->h_zout, which ctx->last_comp names.
// Synchronises for the member count and for every size a buffer is grown to (the set's, the members', the wrappers'); the downloads
// are queued on the ctx's stream and NOT waited for.  n > 0.
static int member_stage(fg_ctx* ctx, const uint64_t* d_out_offsets, const uint8_t* d_enc_status, uint64_t n, uint64_t total) {
    hipStream_t s = ctx->stream;
    const bool kafka = ctx->wire == FG_WIRE_KAFKA_V0, gzip = ctx->compress.codec == FG_COMP_GZIP;
    if (!fg_launch_deflate_cuts || (kafka && !fg_launch_kafka_cuts)) return FG_ERR_UNSUPPORTED;  // (only in a build without the kernels: fg_ctx.hpp)
    int rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_df_cut, &ctx->d_df_cut_cap, MemberCuts(nullptr, n).bytes)) != FG_OK) return rc;
    if (kafka && (rc = grow_dev(ctx, (void**)&ctx->d_kf_off, &ctx->d_kf_off_cap, KfOffsets(nullptr, n).bytes)) != FG_OK) return rc;
    const MemberCuts m(ctx->d_df_cut, n);
    const KfOffsets k(kafka ? ctx->d_kf_off : nullptr, n);
    FG_LAUNCH(ctx, fg_launch_deflate_cuts(d_out_offsets, n, ctx->compress.coalesce, ctx->compress.member_bytes, m.d_flags, m.d_sums, m.d_idx, m.d_first,
                                          m.d_cuts, m.d_count, s));
    ctx->df_members = 0;
    FG_HIP(ctx, hipMemcpyAsync(&ctx->df_members, m.d_count, 8, hipMemcpyDeviceToHost, s));
    FG_HIP(ctx, hipStreamSynchronize(s));
    const uint64_t nm = ctx->df_members;
    if (nm == 0 || nm > n) return FG_ERR_ARG;  // (never: message 0 starts a member, and no member is without a first message)
    // what goes to the host: wt bytes at d_wire, the members' bounds in them d_wire_off[0 .. nm]
    const uint8_t* d_wire = ctx->d_tout;
    const uint64_t* d_wire_off = m.d_cuts;
    uint64_t wt = total;
    if (kafka) {
        if ((rc = fg_kafka_set_front(ctx, d_out_offsets, d_enc_status, n, total, k.d_set_off, &wt, s)) != FG_OK) return rc;
        if ((rc = grow_dev(ctx, (void**)&ctx->d_kf_set, &ctx->d_kf_set_cap, wt + 16)) != FG_OK) return rc;
        if (wt && (rc = fg_kafka_set_write(ctx, ctx->d_tout, d_out_offsets, d_enc_status, n, k.d_set_off, ctx->d_kf_set, ctx->d_kf_set_cap, s)) != FG_OK) return rc;
        FG_LAUNCH(ctx, fg_launch_kafka_cuts(k.d_set_off, m.d_first, n, nm, k.d_set_cuts, s));
        d_wire = ctx->d_kf_set;
        d_wire_off = k.d_set_cuts;
    }
    if (gzip) {
        uint64_t zt = 0;
        if ((rc = fg_deflate_front(ctx, d_wire, wt, d_wire_off, nm, m.d_zoff, &zt, s)) != FG_OK) return rc;
        if ((rc = grow_dev(ctx, (void**)&ctx->d_zout, &ctx->d_zout_cap, zt + 16)) != FG_OK) return rc;
        if ((rc = fg_deflate_pack(ctx, d_wire, d_wire_off, nm, m.d_zoff, ctx->d_zout, ctx->d_zout_cap, s)) != FG_OK) return rc;
        d_wire = ctx->d_zout;
        d_wire_off = m.d_zoff;
        wt = zt;
        if (kafka) {
            if ((rc = fg_kafka_wrap_front(ctx, m.d_zoff, nm, k.d_woff, &wt, s)) != FG_OK) return rc;
            if ((rc = grow_dev(ctx, (void**)&ctx->d_kf_w, &ctx->d_kf_w_cap, wt + 16)) != FG_OK) return rc;
            if ((rc = fg_kafka_wrap_write(ctx, ctx->d_zout, m.d_zoff, nm, k.d_woff, ctx->d_kf_w, ctx->d_kf_w_cap, s)) != FG_OK) return rc;
            d_wire = ctx->d_kf_w;
            d_wire_off = k.d_woff;
        }
    }
    const uint64_t zb = up(wt, 256), lb = up((nm + 1) * 8, 256);
    if ((rc = grow_pinned(ctx, (void**)&ctx->h_zout, &ctx->h_zout_cap, zb + 2 * lb)) != FG_OK) return rc;
    uint8_t* h = ctx->h_zout;
    if (wt) FG_HIP(ctx, hipMemcpyAsync(h, d_wire, wt, hipMemcpyDeviceToHost, s));
    FG_HIP(ctx, hipMemcpyAsync(h + zb, d_wire_off, (nm + 1) * 8, hipMemcpyDeviceToHost, s));
    FG_HIP(ctx, hipMemcpyAsync(h + zb + lb, m.d_first, (nm + 1) * 8, hipMemcpyDeviceToHost, s));
    ctx->last_comp = fg_compressed{h, wt, reinterpret_cast<const uint64_t*>(h + zb), reinterpret_cast<const uint64_t*>(h + zb + lb), nm, total};
    return FG_OK;
}

// Steps 2 - 4 of a one-piece transcode, shared by fg_transcode_batch and fg_transcode_multi_batch -- nothing here depends on where the
// frames came from: the n frames ctx->d_offsets names in d_src[0 .. src_bytes) (d_bad nonzero: a skipped row) are decoded into tables
// that stay in HBM, encoded + framed from them (the output buffer grows to the batch: steady state is one count + one write; sized from
// in_bytes the first time), and the stream and the per-line verdicts are downloaded into ctx->h_tout: the messages, the fixed arrays
// behind them (`frames`: with room for frame offsets, which the caller fills).  *res gets the pointers and out_bytes; the downloads
// are queued on the ctx's stream and NOT waited for.
static int transcode_tail(fg_ctx* ctx, fg_format fmt, fg_framing dec_framing, const fg_encode_cfg* ecfg, const uint8_t* d_src, uint64_t src_bytes,
                          uint64_t n, const uint8_t* d_bad, uint64_t in_bytes, bool frames, fg_transcoded* res) {
    hipStream_t s = ctx->stream;
    int rc;
    // 2. decode (tables stay in HBM)
    fg_tables dt{};
    uint64_t ent_used = 0;
    if ((rc = decode_stage(ctx, fmt, dec_framing, src_bytes, n, d_bad, &dt, &ent_used, d_src)) != FG_OK) return rc;
    // 3. encode + frame from the tables
    const uint64_t offs_bytes = up((n + 1) * 8, 256);
    if ((rc = grow_dev(ctx, (void**)&ctx->d_tmeta, &ctx->d_tmeta_cap, offs_bytes + up(n, 256))) != FG_OK) return rc;
    uint64_t* d_out_offsets = reinterpret_cast<uint64_t*>(ctx->d_tmeta);
    uint8_t* d_enc_status = ctx->d_tmeta + offs_bytes;
    if (!ctx->d_tout && (rc = grow_dev(ctx, (void**)&ctx->d_tout, &ctx->d_tout_cap, in_bytes + in_bytes / 2 + 4096)) != FG_OK) return rc;
    uint64_t total = 0;
    rc = fg_encode_device(ctx, fmt, ecfg, d_src, src_bytes, ctx->d_offsets, n, &dt, ctx->d_tout, ctx->d_tout_cap, d_out_offsets,
                          d_enc_status, &total, FG_STREAM_OWN);
    if (rc == FG_ERR_ENT_OVERFLOW) {
        if ((rc = grow_dev(ctx, (void**)&ctx->d_tout, &ctx->d_tout_cap, total + 4096)) != FG_OK) return rc;
        rc = fg_encode_device(ctx, fmt, ecfg, d_src, src_bytes, ctx->d_offsets, n, &dt, ctx->d_tout, ctx->d_tout_cap, d_out_offsets,
                              d_enc_status, &total, FG_STREAM_OWN);
    }
    if (rc != FG_OK) return rc;
    // 4. the messages, the fixed arrays behind them -- or, with a member stage, the members in the messages' place (ctx->h_zout)
    const bool members = ctx->wire != FG_WIRE_RAW || ctx->compress.codec != FG_COMP_NONE;
    const uint64_t plain = members ? 0 : up(total, 256);
    if ((rc = grow_pinned(ctx, (void**)&ctx->h_tout, &ctx->h_tout_cap, transcoded_arrays(nullptr, plain, n, frames, res))) != FG_OK) return rc;
    uint8_t* h = ctx->h_tout;
    transcoded_arrays(h, plain, n, frames, res);
    if (members) {
        if ((rc = member_stage(ctx, d_out_offsets, d_enc_status, n, total)) != FG_OK) return rc;
    } else if (total) {
        FG_HIP(ctx, hipMemcpyAsync(h, ctx->d_tout, total, hipMemcpyDeviceToHost, s));
    }
    FG_HIP(ctx, hipMemcpyAsync((void*)res->out_offsets, d_out_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    FG_HIP(ctx, hipMemcpyAsync((void*)res->meta, dt.meta, n * 4, hipMemcpyDeviceToHost, s));
    FG_HIP(ctx, hipMemcpyAsync((void*)res->enc_status, d_enc_status, n, hipMemcpyDeviceToHost, s));
    res->out = members ? nullptr : h;
    res->out_bytes = total;
    return FG_OK;
}

int fg_transcode_batch(fg_ctx* ctx, fg_format fmt, fg_framing framing, const fg_encode_cfg* ecfg, const uint8_t* bytes,
                       uint64_t nbytes, const uint64_t* offsets, uint64_t n, int final, fg_transcoded* out) {
    if (!ctx || !ecfg || !out || (nbytes && !bytes)) return FG_ERR_ARG;
    if ((int)framing < 0 || (int)framing > (int)FG_FRAME_CAPNP) return FG_ERR_ARG;
    if (fmt == FG_CAPNP && framing != FG_FRAME_NONE && framing != FG_FRAME_CAPNP) return FG_ERR_ARG;  // (a capnp stream has its own framing,
    if (fmt != FG_CAPNP && framing == FG_FRAME_CAPNP) return FG_ERR_ARG;                               //  and nothing else has it)
    const bool syslen = framing == FG_FRAME_SYSLEN, capnp = framing == FG_FRAME_CAPNP;
    if (syslen) ctx->last_syslen_stop = FG_SYSLEN_CLEAN;
    if (capnp) ctx->last_capnp_stop = FG_CAPNP_CLEAN;
    if (framing == FG_FRAME_NONE) {
        if (check_packed_batch(fmt, nbytes, offsets, n) != FG_OK) return FG_ERR_ARG;
    } else if (offsets) {
        return FG_ERR_ARG;  // a raw stream chunk is framed here; it does not come with offsets
    }
    *out = fg_transcoded{};
    ctx->last_comp = fg_compressed{};
    if (framing != FG_FRAME_NONE && nbytes == 0) return FG_OK;
    DeviceGuard g(ctx->device);
    hipStream_t s = ctx->stream;
    int rc;
    // (from 16 MiB: the slices start at 4 MiB, so a 25 MB batch already has its first download in flight while the rest uploads --
    //  100 000 lines 1.65 vs 1.81 ms in one piece, 250 000 lines 3.35 vs 4.2; at 13 MB the two forms are level)
    // (with compression set: one piece -- members are not cut across slices)
    if (framing == FG_FRAME_NONE && nbytes >= (16ull << 20) && n >= 4096 && !(ctx->lo.flags & FG_LO_TRANSCODE_ONE_PIECE) &&
        ctx->compress.codec == FG_COMP_NONE && ctx->wire == FG_WIRE_RAW) {
        rc = transcode_sliced(ctx, fmt, ecfg, bytes, nbytes, offsets, n, out);
        if (rc != FG_ERR_UNSUPPORTED) return rc;
        *out = fg_transcoded{};
    }
    // (with a member stage every exit from here on waits for what it queued: member_stage reads counts and sizes between its steps, so
    //  an error may leave with work queued behind them.  Without one this path's calls are what they were.)
    DrainGuard drained(ctx);
    drained.armed = ctx->compress.codec != FG_COMP_NONE || ctx->wire != FG_WIRE_RAW;
    // 1. the chunk (and, for framed input, its offsets) to HBM
    if (!syslen) {
        if ((rc = grow_dev(ctx, (void**)&ctx->d_bytes, &ctx->d_bytes_cap, up(nbytes, 16) + 16)) != FG_OK) return rc;
        if (nbytes) FG_HIP(ctx, hipMemcpyAsync(ctx->d_bytes, bytes, nbytes, hipMemcpyHostToDevice, s));
        FG_HIP(ctx, hipMemsetAsync(ctx->d_bytes + nbytes, 0, up(nbytes, 16) + 16 - nbytes, s));
    }
    uint64_t consumed = nbytes;
    const uint8_t* d_bad = nullptr;
    // (FG_FRAME_SYSLEN: what is decoded and encoded is the PACKED batch -- payloads back to back, FG_FRAME_NONE offsets)
    const uint8_t* d_src = nullptr;
    uint64_t src_bytes = 0;
    fg_framing dec_framing = framing;
    if (syslen) {
        if ((rc = syslen_stage(ctx, bytes, nbytes, final, &n, &consumed, &src_bytes)) != FG_OK) return rc;
        d_bad = ctx->d_bad;
        d_src = ctx->d_sl_packed;
        dec_framing = FG_FRAME_NONE;
    } else if (framing == FG_FRAME_NONE) {
        if ((rc = grow_dev(ctx, (void**)&ctx->d_offsets, &ctx->d_offsets_cap, (n + 1) * 8)) != FG_OK) return rc;
        if (n) FG_HIP(ctx, hipMemcpyAsync(ctx->d_offsets, offsets, (n + 1) * 8, hipMemcpyHostToDevice, s));
    } else if (capnp) {  // (framed where the chunk lies; what is decoded are the messages in ctx->d_bytes, FG_FRAME_NONE offsets)
        if ((rc = capnp_stage(ctx, bytes, nbytes, final, &n, &consumed)) != FG_OK) return rc;
        dec_framing = FG_FRAME_NONE;
    } else {
        if ((rc = frame_stage(ctx, framing, nbytes, final, &n, &consumed)) != FG_OK) return rc;
        d_bad = ctx->d_bad;
    }
    out->n = n;
    out->consumed = consumed;
    if (n == 0) {
        FG_HIP(ctx, hipStreamSynchronize(s));
        return FG_OK;
    }
    if (!syslen) {
        d_src = ctx->d_bytes;
        src_bytes = consumed;
    }
    // 2. - 4. decode, encode, and only the encoded stream and the per-line verdicts cross PCIe back
    const bool frames = framing != FG_FRAME_NONE;
    fg_transcoded res = *out;  // (n and consumed)
    if ((rc = transcode_tail(ctx, fmt, dec_framing, ecfg, d_src, src_bytes, n, d_bad, consumed, frames, &res)) != FG_OK) return rc;
    if (syslen) memcpy((void*)res.frame_offsets, ctx->h_off, (n + 1) * 8);  // (the frame starts in the caller's chunk, prefix included)
    else if (frames) FG_HIP(ctx, hipMemcpyAsync((void*)res.frame_offsets, ctx->d_offsets, (n + 1) * 8, hipMemcpyDeviceToHost, s));
    FG_HIP(ctx, hipStreamSynchronize(s));
    drained.armed = false;
    *out = res;
    return FG_OK;
}

// fg_transcode_batch for the chunks of MANY connections: the front half of the matching fg_frame_decode_*multi_batch entry (upload,
// segmented framing, the mirror of the per-segment and per-slot lists -- with the per-segment cut for octet-counted input), then the
// transcode tail over every slot.  One piece, as those entries.
int fg_transcode_multi_batch(fg_ctx* ctx, fg_format fmt, fg_framing framing, const fg_encode_cfg* ecfg, const uint8_t* bytes, uint64_t nbytes,
                             const uint64_t* seg_starts, const uint8_t* seg_final, uint64_t n_segs, fg_transcoded_multi* out) {
    if (!ctx || !ecfg || !out || (nbytes && !bytes)) return FG_ERR_ARG;
    const bool lines = framing == FG_FRAME_LINE || framing == FG_FRAME_NUL, syslen = framing == FG_FRAME_SYSLEN, capnp = framing == FG_FRAME_CAPNP;
    if (!lines && !syslen && !capnp) return FG_ERR_ARG;        // (FG_FRAME_NONE: a packed batch has no segments -- fg_transcode_batch)
    if ((fmt == FG_CAPNP) != capnp) return FG_ERR_ARG;         // (a capnp stream has its own framing, and nothing else has it)
    if (!lines && seg_final) return FG_ERR_ARG;
    if ((lines ? lines_multi_args(fmt, framing, nbytes, seg_starts, n_segs)
               : syslen ? syslen_multi_args(fmt, nbytes, seg_starts, n_segs) : capnp_multi_args(nbytes, seg_starts, n_segs)) != FG_OK)
        return FG_ERR_ARG;
    *out = fg_transcoded_multi{};
    ctx->last_comp = fg_compressed{};
    fg_tables none{};  // (SegBatch::upload clears the decode entries' tables)
    SegBatch b{ctx, n_segs, &none, &out->n, &out->seg_first, &out->seg_consumed, lines ? nullptr : &out->seg_stop, &out->slot_offsets, &out->slot_kind};
    DeviceGuard g(ctx->device);
    DrainGuard drained(ctx);  // (every exit from here on waits for what it queued)
    SegFramed f;
    fg_transcoded res{};
    int rc = lines ? lines_multi_front(b, framing, bytes, nbytes, seg_starts, seg_final, &f)
                   : syslen ? syslen_multi_front(b, bytes, nbytes, seg_starts, &f) : capnp_multi_front(b, bytes, nbytes, seg_starts, &f);
    if (rc == FG_OK) rc = b.finish_transcode(f, fmt, ecfg, nbytes, &res);
    if (rc == FG_OK) rc = drained.done();
    if (rc != FG_OK) {
        *out = fg_transcoded_multi{};
        ctx->last_host_path = 0;
        return rc;
    }
    out->out = res.out;
    out->out_bytes = res.out_bytes;
    out->out_offsets = res.out_offsets;
    out->meta = res.meta;
    out->enc_status = res.enc_status;
    return FG_OK;
}

// fg_transcode_batch for a batch of UDP datagrams: the front half of fg_udp_decode_batch with the one-walk unpacker (which sizes the
// packed buffer between its two halves, so no stream is walked for its size alone), then the transcode tail over every datagram with
// the drop flags as the skipped rows.  One piece, as fg_udp_decode_batch.
int fg_udp_transcode_batch(fg_ctx* ctx, fg_format fmt, const fg_encode_cfg* ecfg, const uint8_t* bytes, uint64_t nbytes, const uint64_t* offsets,
                           uint64_t n, uint64_t max_inflated, fg_transcoded* out, const uint8_t** udp_status) {
    if (!ctx || !ecfg || !out || !udp_status || !offsets || (nbytes && !bytes)) return FG_ERR_ARG;
    if (!text_format(fmt)) return FG_ERR_ARG;  // (FG_CAPNP: the reference has no Decoder for it, as fg_udp_decode_batch)
    if (n && (offsets[0] != 0 || offsets[n] != nbytes)) return FG_ERR_ARG;
    for (uint64_t i = 0; i < n; ++i)
        if (offsets[i] > offsets[i + 1]) return FG_ERR_ARG;
    if (max_inflated == 0) max_inflated = FG_UDP_DEFAULT_MAX_INFLATED;
    if (max_inflated > FG_UDP_MAX_MAX_INFLATED) return FG_ERR_ARG;
    *out = fg_transcoded{};
    ctx->last_comp = fg_compressed{};
    *udp_status = nullptr;
    ctx->udp_last_spilled = 0;
    out->consumed = nbytes;
    if (n == 0) return FG_OK;
    DeviceGuard g(ctx->device);
    DrainGuard drained(ctx);  // (every exit from here on waits for what it queued)
    hipStream_t s = ctx->stream;
    int rc;
    // 1. the datagrams and their offsets to HBM
    if ((rc = grow_dev(ctx, (void**)&ctx->d_bytes, &ctx->d_bytes_cap, up(nbytes, 16) + 16)) != FG_OK) return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_udp_off, &ctx->d_udp_off_cap, (n + 2) * 8)) != FG_OK) return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_offsets, &ctx->d_offsets_cap, (n + 2) * 8)) != FG_OK) return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_bad, &ctx->d_bad_cap, n + 1)) != FG_OK) return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_udp_st, &ctx->d_udp_st_cap, n + 1)) != FG_OK) return rc;
    if (nbytes) FG_HIP(ctx, hipMemcpyAsync(ctx->d_bytes, bytes, nbytes, hipMemcpyHostToDevice, s));
    FG_HIP(ctx, hipMemsetAsync(ctx->d_bytes + nbytes, 0, up(nbytes, 16) + 16 - nbytes, s));
    FG_HIP(ctx, hipMemcpyAsync(ctx->d_udp_off, offsets, (n + 1) * 8, hipMemcpyHostToDevice, s));
    // 2. one walk per stream; the packed buffer grows to the batch between the walk and the pack (the walk is never repeated)
    uint64_t total = 0;
    if ((rc = fg_udp_once_front(ctx, ctx->d_bytes, nbytes, ctx->d_udp_off, n, max_inflated, ctx->d_offsets, ctx->d_bad, ctx->d_udp_st, &total, s)) != FG_OK)
        return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_sl_packed, &ctx->d_sl_packed_cap, up(total, 16) + 16)) != FG_OK) return rc;
    if ((rc = fg_udp_once_pack(ctx, ctx->d_bytes, ctx->d_udp_off, n, ctx->d_offsets, ctx->d_sl_packed, total, ctx->d_bad, ctx->d_udp_st, s)) != FG_OK) return rc;
    // (the decoders load 16 bytes at a time: the pad behind the last payload is zero, as behind an uploaded batch)
    FG_HIP(ctx, hipMemsetAsync(ctx->d_sl_packed + total, 0, up(total, 16) + 16 - total, s));
    // 3. decode, encode, frame; the stream, the verdicts and the reasons back
    fg_transcoded res{};
    res.n = n;
    res.consumed = nbytes;
    if ((rc = transcode_tail(ctx, fmt, FG_FRAME_NONE, ecfg, ctx->d_sl_packed, total, n, ctx->d_bad, nbytes, false, &res)) != FG_OK) return rc;
    if ((rc = grow_pinned(ctx, (void**)&ctx->h_udp, &ctx->h_udp_cap, up(n, 16))) != FG_OK) return rc;
    FG_HIP(ctx, hipMemcpyAsync(ctx->h_udp, ctx->d_udp_st, n, hipMemcpyDeviceToHost, s));
    if ((rc = drained.done()) != FG_OK) return rc;
    *out = res;
    *udp_status = ctx->h_udp;
    return FG_OK;
}

}  // extern "C"
