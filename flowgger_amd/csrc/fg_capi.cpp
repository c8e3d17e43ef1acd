// fg_capi.cpp -- host side of the C ABI declared in include/fg_hip.h.
//
// Owns: device selection (gfx950 only, no CPU fallback), the per-ctx HIP stream, staging
// buffers for the host-buffer entry point, HIP-event timing of the decode kernels.
// It mirrors what XDecoder::new(&Config) + Box<dyn Decoder+Send>::clone do in the reference
// (src/flowgger/mod.rs:413-422, src/flowgger/decoder/mod.rs:23-36): a ctx is built once from the
// configuration and cloned per connection thread.
#include "fg_ctx.hpp"
#include "fg_syslen_parse.hpp"
#include "fg_capnp_next.hpp"

namespace {

const char* const kErr5424[] = {
    "",
    "Unsupported BOM",
    "The priority should be inside brackets",
    "Invalid priority",
    "Missing version",
    "Unsupported version",
    "Missing timestamp",
    "Unable to parse the date from RFC3339 to Unix time in RFC5424 decoder",
    "Missing hostname",
    "Missing application name",
    "Missing process id",
    "Missing message id",
    "Missing message data",
    "Missing log message",
    "Malformated RFC5424 message",
    "Missing structured data",
    "Format error in the structured data",
    "Missing ] after structured data",
};
const char* const kErrLtsv[] = {
    "",
    "Invalid severity level",
    "Severity level should be <= 7",
    "Type error; boolean was expected",
    "Type error; f64 was expected",
    "Type error; i64 was expected",
    "Type error; u64 was expected",
    "Missing timestamp",
    "Missing hostname",
    "Unable to parse the English to Unix timestamp in LTSV decoder",
};
const char* const kErrGelf[] = {
    "",
    "Invalid GELF input, unable to parse as a JSON object",
    "Empty GELF input",
    "Invalid GELF timestamp",
    "GELF host name must be a string",
    "GELF short message must be a string",
    "GELF full message must be a string",
    "GELF version must be a string",
    "Unsupported GELF version",
    "Invalid severity level",
    "Invalid severity level (too high)",
    "Invalid value type in structured data",
    "Missing hostname",
};

// Upload the LTSV schema / suffixes once per ctx (LTSVDecoder::new, ltsv_decoder.rs:24-84).
int upload_ltsv_cfg(fg_ctx* ctx) {
    std::vector<uint8_t> blob;
    std::vector<uint32_t> off;
    for (const auto& nme : ctx->schema_names) {
        off.push_back((uint32_t)blob.size());
        blob.insert(blob.end(), nme.begin(), nme.end());
    }
    off.push_back((uint32_t)blob.size());
    fg::LtsvDevCfg c{};
    c.n_schema = (uint32_t)ctx->schema_names.size();
    for (int k = 0; k < 4; ++k) {
        c.suf_off[k] = (uint32_t)blob.size();
        c.suf_len[k] = (uint32_t)ctx->suffix[k].size();
        c.has_suf[k] = ctx->has_suffix[k] ? 1u : 0u;
        blob.insert(blob.end(), ctx->suffix[k].begin(), ctx->suffix[k].end());
    }
    const uint64_t blob_sz = up(blob.size() + 1, 16), off_sz = up(off.size() * 4, 16), ty_sz = up(ctx->schema_types.size() + 1, 16);
    FG_HIP(ctx, hipMalloc((void**)&ctx->d_cfg, blob_sz + off_sz + ty_sz));
    std::vector<uint8_t> host(blob_sz + off_sz + ty_sz, 0);
    if (!blob.empty()) memcpy(host.data(), blob.data(), blob.size());
    memcpy(host.data() + blob_sz, off.data(), off.size() * 4);
    if (!ctx->schema_types.empty()) memcpy(host.data() + blob_sz + off_sz, ctx->schema_types.data(), ctx->schema_types.size());
    FG_HIP(ctx, hipMemcpy(ctx->d_cfg, host.data(), host.size(), hipMemcpyHostToDevice));
    c.blob = ctx->d_cfg;
    c.name_off = (const uint32_t*)(ctx->d_cfg + blob_sz);
    c.types = ctx->d_cfg + blob_sz + off_sz;
    ctx->ltsv = c;
    return FG_OK;
}

// What every decode launch of a ctx needs on the device, allocated by the first: the per-wave entry stash (8 waves on every CU) and
// the ring of hand-over words.
int ensure_launch_state(fg_ctx* ctx) {
    if (!ctx->d_stash) {
        const int cus = fg::device_cus();  // (the DeviceGuard of the call has selected ctx->device)
        if (cus < 1) {
            ctx->last_hip = (int)hipErrorInvalidValue;
            return FG_ERR_HIP;
        }
        const uint32_t blocks = 8u * (uint32_t)cus;
        FG_HIP(ctx, hipMalloc((void**)&ctx->d_stash, fg_stash_bytes(blocks)));
        ctx->stash_blocks = blocks;
    }
    if (!ctx->d_pending) {
        FG_HIP(ctx, hipMalloc((void**)&ctx->d_pending, fg_ctx::kPendingRing * sizeof(uint32_t)));
        FG_HIP(ctx, hipMemset(ctx->d_pending, 0, fg_ctx::kPendingRing * sizeof(uint32_t)));
    }
    return FG_OK;
}
// the ctx's launch counter (0 = the pending ring's initial content: never a valid epoch) and the hand-over word of an epoch
uint32_t next_epoch(fg_ctx* ctx) {
    ctx->epoch += 1u;
    if (ctx->epoch == 0u) ctx->epoch = 1u;
    return ctx->epoch;
}
uint32_t* pending_word(const fg_ctx* ctx, uint32_t epoch) { return ctx->d_pending + (epoch % fg_ctx::kPendingRing); }

// the HIP-event bracket around the kernels of a call (fg_set_timing / fg_last_kernel_ms); end() only where every launch went out
int timing_begin(fg_ctx* ctx, hipStream_t s) {
    if (ctx->timing) FG_HIP(ctx, hipEventRecord(ctx->ev0, s));
    return FG_OK;
}
int timing_end(fg_ctx* ctx, hipStream_t s) {
    if (ctx->timing) {
        FG_HIP(ctx, hipEventRecord(ctx->ev1, s));
        ctx->ev_valid = true;
    }
    return FG_OK;
}

}  // namespace

extern "C" {

int fg_abi_version(void) { return FG_ABI_VERSION; }
int fg_last_host_path(const fg_ctx* ctx) { return ctx ? ctx->last_host_path : 0; }
int fg_last_syslen_stop(const fg_ctx* ctx) { return ctx ? ctx->last_syslen_stop : 0; }
int fg_last_capnp_stop(const fg_ctx* ctx) { return ctx ? ctx->last_capnp_stop : 0; }

int fg_tables_layout(uint64_t n, uint64_t ent_cap, uint64_t sizes[FG_TABLE_ARRAYS]) {
    if (!sizes) return FG_ERR_ARG;
    fg::layout(n, ent_cap, sizes);
    return FG_OK;
}

int fg_create(int device, const fg_cfg* cfg, fg_ctx** out) {
    if (!out) return FG_ERR_ARG;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return FG_ERR_NO_DEVICE;
    if (device < 0 || device >= count) return FG_ERR_NO_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return FG_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return FG_ERR_NO_DEVICE;  // kernels are gfx950-only
    if (cfg && cfg->n_schema) {
        if (!cfg->schema_names || !cfg->schema_types) return FG_ERR_ARG;
        for (uint32_t i = 0; i < cfg->n_schema; ++i)
            if (!cfg->schema_names[i] || cfg->schema_types[i] > FG_T_U64) return FG_ERR_ARG;
    }
    fg_ctx* ctx = new (std::nothrow) fg_ctx();
    if (!ctx) return FG_ERR_NOMEM;
    ctx->device = device;
    if (cfg) {
        for (uint32_t i = 0; i < cfg->n_schema; ++i) {
            ctx->schema_names.emplace_back(cfg->schema_names[i]);
            ctx->schema_types.push_back(cfg->schema_types[i]);
        }
        const char* s[4] = {cfg->suffix_bool, cfg->suffix_f64, cfg->suffix_i64, cfg->suffix_u64};
        for (int k = 0; k < 4; ++k)
            if (s[k]) {
                ctx->suffix[k] = s[k];
                ctx->has_suffix[k] = true;
            }
    }
    DeviceGuard g(device);
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return FG_ERR_HIP;
    }
    if (upload_ltsv_cfg(ctx) != FG_OK) {
        fg_destroy(ctx);
        return FG_ERR_HIP;
    }
    *out = ctx;
    return FG_OK;
}

static int upload_tz(fg_ctx* ctx);
static int utc_year_now() {
    const time_t t = time(nullptr);
    struct tm g;
    gmtime_r(&t, &g);
    return g.tm_year + 1900;
}
// OffsetDateTime::now_utc().year() is evaluated per parse by the reference (rfc3164_decoder.rs:179); here once per decode
// call when the ctx was configured with FG_YEAR_NOW: a long-lived decoder crosses New Year without a restart.
static int refresh_year(fg_ctx* ctx) {
    if (!ctx->r3164_auto_year) return FG_OK;
    const int y = utc_year_now();
    if (y == ctx->r3164_year) return FG_OK;
    // launches already queued on the caller's streams may still read the old block: it is retired, not freed.  The year is
    // taken over only when the new block is in place -- a failed upload leaves year, block and view as they were, so the next
    // call tries again instead of decoding zone-tagged lines without a zone table.
    const int32_t old_year = ctx->r3164_year;
    uint8_t* const old_tz = ctx->d_tz;
    const fg::r3164::Cfg old_cfg = ctx->r3164;
    ctx->r3164_year = y;
    ctx->d_tz = nullptr;
    const int rc = upload_tz(ctx);
    if (rc != FG_OK) {
        if (ctx->d_tz) (void)hipFree(ctx->d_tz);
        ctx->d_tz = old_tz;
        ctx->r3164 = old_cfg;
        ctx->r3164_year = old_year;
        return rc;
    }
    if (old_tz) ctx->retired_tz.push_back(old_tz);
    return FG_OK;
}

int fg_clone(const fg_ctx* src, fg_ctx** out) {
    if (!src || !out) return FG_ERR_ARG;
    fg_ctx* ctx = new (std::nothrow) fg_ctx();
    if (!ctx) return FG_ERR_NOMEM;
    ctx->device = src->device;
    ctx->lo = src->lo;
    ctx->compress = src->compress;
    ctx->deflate_mode = src->deflate_mode;
    ctx->wire = src->wire;
    ctx->schema_names = src->schema_names;
    ctx->schema_types = src->schema_types;
    for (int k = 0; k < 4; ++k) {
        ctx->suffix[k] = src->suffix[k];
        ctx->has_suffix[k] = src->has_suffix[k];
    }
    DeviceGuard g(ctx->device);
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return FG_ERR_HIP;
    }
    if (upload_ltsv_cfg(ctx) != FG_OK) {
        fg_destroy(ctx);
        return FG_ERR_HIP;
    }
    if (src->r3164_set) {
        ctx->r3164_set = true;
        ctx->r3164_auto_year = src->r3164_auto_year;
        ctx->r3164_year = src->r3164_year;
        ctx->tz_names = src->tz_names;
        ctx->tz_first = src->tz_first;
        ctx->tz_start = src->tz_start;
        ctx->tz_off = src->tz_off;
        if (upload_tz(ctx) != FG_OK) {
            fg_destroy(ctx);
            return FG_ERR_HIP;
        }
    }
    *out = ctx;
    return FG_OK;
}

void fg_destroy(fg_ctx* ctx) {
    if (!ctx) return;
    DeviceGuard g(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->d_bytes) (void)hipFree(ctx->d_bytes);
    if (ctx->d_offsets) (void)hipFree(ctx->d_offsets);
    if (ctx->d_tab) (void)hipFree(ctx->d_tab);
    if (ctx->d_cfg) (void)hipFree(ctx->d_cfg);
    if (ctx->d_stash) (void)hipFree(ctx->d_stash);
    if (ctx->d_stash2) (void)hipFree(ctx->d_stash2);
    if (ctx->d_pending) (void)hipFree(ctx->d_pending);
    if (ctx->d_ticket) (void)hipFree(ctx->d_ticket);
    if (ctx->d_merge) (void)hipFree(ctx->d_merge);
    if (ctx->d_sink) (void)hipFree(ctx->d_sink);
    if (ctx->d_used) (void)hipFree(ctx->d_used);
    if (ctx->d_frame) (void)hipFree(ctx->d_frame);
    if (ctx->d_fused) (void)hipFree(ctx->d_fused);
    if (ctx->d_r3164) (void)hipFree(ctx->d_r3164);
    if (ctx->d_bad) (void)hipFree(ctx->d_bad);
    if (ctx->d_sl_packed) (void)hipFree(ctx->d_sl_packed);
    if (ctx->d_sl_starts) (void)hipFree(ctx->d_sl_starts);
    if (ctx->d_udp) (void)hipFree(ctx->d_udp);
    if (ctx->d_udp_stage) (void)hipFree(ctx->d_udp_stage);
    if (ctx->d_udp_off) (void)hipFree(ctx->d_udp_off);
    if (ctx->d_udp_st) (void)hipFree(ctx->d_udp_st);
    if (ctx->h_udp) (void)hipHostFree(ctx->h_udp);
    if (ctx->d_ms) (void)hipFree(ctx->d_ms);
    if (ctx->h_ms) (void)hipHostFree(ctx->h_ms);
    if (ctx->d_enc) (void)hipFree(ctx->d_enc);
    if (ctx->h_enc_ring) (void)hipHostFree(ctx->h_enc_ring);
    for (hipEvent_t e : ctx->ev_enc)
        if (e) (void)hipEventDestroy(e);
    if (ctx->d_tz) (void)hipFree(ctx->d_tz);
    for (uint8_t* p : ctx->retired_tz) (void)hipFree(p);
    if (ctx->h_off) (void)hipHostFree(ctx->h_off);
    if (ctx->h_cnt) (void)hipHostFree(ctx->h_cnt);
    if (ctx->h_tab) (void)hipHostFree(ctx->h_tab);
    if (ctx->d_tout) (void)hipFree(ctx->d_tout);
    if (ctx->d_tmeta) (void)hipFree(ctx->d_tmeta);
    if (ctx->h_tout) (void)hipHostFree(ctx->h_tout);
    if (ctx->d_df) (void)hipFree(ctx->d_df);
    if (ctx->d_df_blk) (void)hipFree(ctx->d_df_blk);
    if (ctx->d_df_slots) (void)hipFree(ctx->d_df_slots);
    if (ctx->d_df_cut) (void)hipFree(ctx->d_df_cut);
    if (ctx->d_zout) (void)hipFree(ctx->d_zout);
    if (ctx->h_zout) (void)hipHostFree(ctx->h_zout);
    for (uint8_t* p : {ctx->d_kf, ctx->d_kf_wrap, ctx->d_kf_crc, ctx->d_kf_set, ctx->d_kf_off, ctx->d_kf_w})
        if (p) (void)hipFree(p);
    if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
    if (ctx->stream3) (void)hipStreamSynchronize(ctx->stream3);
    for (hipEvent_t e : ctx->ev_slice) (void)hipEventDestroy(e);
    if (ctx->stream3) (void)hipStreamDestroy(ctx->stream3);
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->ev_ready) (void)hipEventDestroy(ctx->ev_ready);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int fg_last_hip_error(const fg_ctx* ctx) { return ctx ? ctx->last_hip : 0; }

int fg_set_launch_opts(fg_ctx* ctx, const fg_launch_opts* opts) {
    if (!ctx) return FG_ERR_ARG;
    if (opts && (opts->lines_per_group > 64 || (opts->gelf_window_kib && (opts->gelf_window_kib < 2 || opts->gelf_window_kib > 6)))) return FG_ERR_ARG;
    ctx->lo = opts ? *opts : fg_launch_opts{};
    ctx->lo.flags &= ~(uint32_t)FG_LO_RESERVED;
    return FG_OK;
}

int fg_set_timing(fg_ctx* ctx, int enabled) {
    if (!ctx) return FG_ERR_ARG;
    DeviceGuard g(ctx->device);
    if (enabled && !ctx->ev0) {
        FG_HIP(ctx, hipEventCreate(&ctx->ev0));
        FG_HIP(ctx, hipEventCreate(&ctx->ev1));
    }
    ctx->timing = enabled != 0;
    ctx->ev_valid = false;
    return FG_OK;
}

int fg_ticket_ring_check(fg_ctx* ctx) {
    if (!ctx) return FG_ERR_ARG;
    DeviceGuard g(ctx->device);
    if (!ctx->d_ticket) return 0;  // no decode launch yet
    FG_HIP(ctx, hipDeviceSynchronize());  // (launches may have gone to any stream the caller passed)
    std::vector<uint32_t> dev(ctx->h_ticket.size());
    FG_HIP(ctx, hipMemcpy(dev.data(), ctx->d_ticket, dev.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    int bad = 0;
    for (size_t k = 0; k < dev.size(); ++k) bad += dev[k] != ctx->h_ticket[k] ? 1 : 0;
    return bad;
}

int fg_last_kernel_ms(fg_ctx* ctx, float* ms) {
    if (!ctx || !ms) return FG_ERR_ARG;
    *ms = 0.f;
    if (!ctx->timing || !ctx->ev_valid) return FG_OK;
    DeviceGuard g(ctx->device);
    FG_HIP(ctx, hipEventSynchronize(ctx->ev1));
    FG_HIP(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return FG_OK;
}

int fg_calibrate_device(fg_ctx* ctx, int mode, const uint8_t* d_src, uint8_t* d_dst, uint64_t nbytes, void* stream) {
    if (!ctx || !d_src || mode < FG_CALIB_COPY || mode > FG_CALIB_COPY_FLAT || (mode != FG_CALIB_READ && !d_dst)) return FG_ERR_ARG;
    if ((((uintptr_t)d_src) | ((uintptr_t)d_dst)) & 15u) return FG_ERR_ARG;
    DeviceGuard g(ctx->device);
    if (!ctx->d_sink) FG_HIP(ctx, hipMalloc((void**)&ctx->d_sink, 256));
    hipStream_t s = stream_of(ctx, stream);
    FG_LAUNCH(ctx, fg_launch_calib(mode, d_src, d_dst, nbytes, ctx->d_sink, s));
    return FG_OK;
}

int fg_merge_tables_device(fg_ctx* ctx, const fg_tables* parts, uint32_t g, const uint64_t* const* d_index, const fg_tables* out,
                           uint8_t* d_src_part, void* stream) {
    if (!ctx || !parts || !d_index || !out || g == 0 || g > 8) return FG_ERR_ARG;
    uint64_t rows = 0, cap = 0, max_rows = 0, max_cap = 0;
    // every column the merge kernels read or write must be there (a table without its entry counter was a device fault)
    auto complete = [](const fg_tables& t, bool entries) {
        return (t.n == 0 || fg::has_rows(t)) && (!entries || fg::has_entries(t)) && t.ent_used != nullptr;
    };
    if (!complete(*out, out->ent_cap != 0)) return FG_ERR_ARG;
    for (uint32_t k = 0; k < g; ++k) {
        if (parts[k].n && !d_index[k]) return FG_ERR_ARG;
        if (!complete(parts[k], parts[k].ent_cap != 0)) return FG_ERR_ARG;
        rows += parts[k].n;
        cap += parts[k].ent_cap;
        if (parts[k].n > max_rows) max_rows = parts[k].n;
        if (parts[k].ent_cap > max_cap) max_cap = parts[k].ent_cap;
    }
    if (out->n != rows || out->ent_cap < cap || cap > 0xFFFFFFFFull) return FG_ERR_ARG;
    DeviceGuard gd(ctx->device);
    hipStream_t s = stream_of(ctx, stream);
    (void)max_cap;
    int grc;
    if ((grc = grow_dev(ctx, (void**)&ctx->d_merge, &ctx->d_merge_cap, fg_merge_scratch_bytes(rows))) != FG_OK) return grc;
    FG_LAUNCH(ctx, fg_launch_merge_device(parts, g, d_index, out, d_src_part, max_rows, ctx->d_merge, s));
    return FG_OK;
}

int fg_decode_batch_device(fg_ctx* ctx, fg_format fmt, const uint8_t* d_bytes, uint64_t nbytes,
                           const uint64_t* d_offsets, uint64_t n, const fg_tables* tables, void* stream) {
    return fg_decode_frames_device(ctx, fmt, FG_FRAME_NONE, d_bytes, nbytes, d_offsets, n, nullptr, tables, stream);
}

int fg_frame_device(fg_ctx* ctx, fg_framing framing, const uint8_t* d_bytes, uint64_t nbytes, uint64_t* d_offsets,
                    uint8_t* d_bad_utf8, uint64_t cap_frames, uint64_t* n_frames, void* stream) {
    if (!ctx || !d_offsets || !d_bad_utf8 || !n_frames || (nbytes && !d_bytes)) return FG_ERR_ARG;
    if (framing != FG_FRAME_LINE && framing != FG_FRAME_NUL) return FG_ERR_UNSUPPORTED;
    if (((uintptr_t)d_bytes & 15u) != 0) return FG_ERR_ARG;
    DeviceGuard g(ctx->device);
    hipStream_t s = stream_of(ctx, stream);
    *n_frames = 0;
    if (nbytes == 0) return FG_OK;
    // frames = delimiters (+1 when the stream does not end with one)
    uint64_t total = 0, last_end = 0;
    const int rc = frame_scan(ctx, framing, d_bytes, nbytes, d_offsets, d_bad_utf8, cap_frames, s, &total, &last_end);
    if (rc == FG_ERR_ENT_OVERFLOW) *n_frames = total + 1;
    if (rc != FG_OK) return rc;
    *n_frames = last_end == nbytes ? total : total + 1;
    return FG_OK;
}

// An EMPTY buffer of n_segs connections: no slots, every segment starts at slot 0, consumed nothing and stopped `clean` (d_offsets,
// d_seg_stop: null where the framing has none).
static int clear_segments(fg_ctx* ctx, uint64_t n_segs, uint64_t* d_offsets, uint64_t* d_seg_first, uint64_t* d_seg_consumed, uint8_t* d_seg_stop,
                          int clean, hipStream_t s) {
    if (d_offsets) FG_HIP(ctx, hipMemsetAsync(d_offsets, 0, 8, s));
    if (n_segs) {
        FG_HIP(ctx, hipMemsetAsync(d_seg_first, 0, (n_segs + 1) * 8, s));
        FG_HIP(ctx, hipMemsetAsync(d_seg_consumed, 0, n_segs * 8, s));
        if (d_seg_stop) FG_HIP(ctx, hipMemsetAsync(d_seg_stop, clean, n_segs, s));
    }
    if (d_offsets || n_segs) FG_HIP(ctx, hipStreamSynchronize(s));
    return FG_OK;
}

// The result words of a chained framer's launch (fg::syslen / fg::capnpf H_*; `done` = the framing's H_DONE) into hdr: a launch
// that declined or did not finish -> FG_ERR_UNSUPPORTED; *n = its frames, more than cap -> FG_ERR_ENT_OVERFLOW.
namespace sl = fg::syslen;
namespace cp = fg::capnpf;
static_assert((int)sl::H_DECLINE == (int)cp::H_DECLINE && (int)sl::H_NFRAMES == (int)cp::H_NFRAMES, "both framings keep these two words in one place");
constexpr int kHdrWords = 8;  // the words the host reads: every H_* it asks for lies below
static_assert(sl::H_DONE < kHdrWords && cp::H_DONE < kHdrWords && sl::H_TOTAL < kHdrWords, "a result word the host reads is not copied");
static int read_frame_hdr(fg_ctx* ctx, const uint32_t* d_hdr, int done, uint64_t cap, uint64_t* n, uint32_t* hdr, hipStream_t s) {
    memset(hdr, 0, kHdrWords * sizeof(uint32_t));
    FG_HIP(ctx, hipMemcpyAsync(hdr, d_hdr, kHdrWords * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    FG_HIP(ctx, hipStreamSynchronize(s));
    if (hdr[sl::H_DECLINE] != 0 || hdr[done] != 1) return FG_ERR_UNSUPPORTED;
    *n = hdr[sl::H_NFRAMES];
    return *n > cap ? FG_ERR_ENT_OVERFLOW : FG_OK;
}

// replaces the per-connection `buf_reader.lines()` / `split(0)` + str::from_utf8 (tcp_input.rs:39-47, line_splitter.rs:17-25,
// nul_splitter.rs:18-40) for the chunks of n_segs connections at once
int fg_frame_multi_device(fg_ctx* ctx, fg_framing framing, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_seg_starts,
                          const uint8_t* d_seg_final, uint64_t n_segs, uint64_t* d_offsets, uint8_t* d_kind, uint64_t cap_slots,
                          uint64_t* d_seg_first, uint64_t* d_seg_consumed, uint64_t* n_slots, void* stream) {
    if (!ctx || !d_offsets || !n_slots || (cap_slots && !d_kind) || (nbytes && !d_bytes)) return FG_ERR_ARG;
    if (n_segs && (!d_seg_starts || !d_seg_first || !d_seg_consumed)) return FG_ERR_ARG;
    if (framing != FG_FRAME_LINE && framing != FG_FRAME_NUL) return FG_ERR_ARG;
    if (((uintptr_t)d_bytes & 15u) != 0) return FG_ERR_ARG;
    *n_slots = 0;
    if (!fg_launch_frame_multi || !fg_frame_multi_scratch_bytes) return FG_ERR_UNSUPPORTED;  // (only in a build without the kernels: fg_ctx.hpp)
    DeviceGuard g(ctx->device);
    hipStream_t s = stream_of(ctx, stream);
    if (nbytes == 0 || n_segs == 0) return clear_segments(ctx, n_segs, nullptr, d_seg_first, d_seg_consumed, nullptr, 0, s);
    int rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_frame, &ctx->d_frame_cap, fg_frame_multi_scratch_bytes(nbytes, n_segs))) != FG_OK) return rc;
    uint64_t res[2] = {0, 0};
    for (int classic = (ctx->lo.flags & FG_LO_FRAME_CLASSIC) ? 1 : 0;; classic = 1) {
        uint64_t* d_res = nullptr;
        FG_LAUNCH(ctx, fg_launch_frame_multi(d_bytes, nbytes, framing == FG_FRAME_LINE ? 0x0Au : 0x00u, d_seg_starts, d_seg_final, n_segs, ctx->d_frame,
                                              d_offsets, d_kind, cap_slots, d_seg_first, d_seg_consumed, &d_res, s, classic));
        FG_HIP(ctx, hipMemcpyAsync(res, d_res, 16, hipMemcpyDeviceToHost, s));
        FG_HIP(ctx, hipStreamSynchronize(s));
        if (res[0] != FG_FRAME_ABORTED || classic == 1) break;  // (the one-pass scan gave up waiting on a tile: the classic form)
    }
    *n_slots = res[1];
    return res[1] > cap_slots ? FG_ERR_ENT_OVERFLOW : FG_OK;
}

// replaces read_msglen + read_exact + String::from_utf8 of SyslenSplitter::run (splitter/syslen_splitter.rs:17-57) for a chunk
int fg_frame_syslen_device(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, int final, uint8_t* d_packed, uint64_t* d_offsets,
                           uint64_t* d_frame_starts, uint8_t* d_bad_utf8, uint64_t cap_frames, uint64_t* n_frames, uint64_t* consumed,
                           int* stop_reason, void* stream) {
    (void)final;  // (a frame needs its whole payload either way; what a TAIL means at the end of the stream is the caller's business)
    if (!ctx || !d_packed || !d_offsets || !d_frame_starts || !d_bad_utf8 || !n_frames || !consumed || !stop_reason || (nbytes && !d_bytes))
        return FG_ERR_ARG;
    if (((uintptr_t)d_bytes & 15u) != 0 || ((uintptr_t)d_packed & 15u) != 0) return FG_ERR_ARG;
    *n_frames = 0;
    *consumed = 0;
    *stop_reason = FG_SYSLEN_CLEAN;
    if (!fg_launch_syslen || !fg_syslen_max_bytes || !fg_syslen_scratch_bytes) return FG_ERR_UNSUPPORTED;  // (only in a build without the kernels: fg_ctx.hpp)
    if (nbytes > fg_syslen_max_bytes()) return FG_ERR_UNSUPPORTED;  // (the scratch keeps positions as 32-bit words)
    DeviceGuard g(ctx->device);
    hipStream_t s = stream_of(ctx, stream);
    int rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_frame, &ctx->d_frame_cap, fg_syslen_scratch_bytes(nbytes))) != FG_OK) return rc;
    uint32_t* d_hdr = nullptr;
    FG_LAUNCH(ctx, fg_launch_syslen(d_bytes, nbytes, ctx->d_frame, d_packed, d_offsets, d_frame_starts, d_bad_utf8, cap_frames, &d_hdr, s));
    uint32_t hdr[kHdrWords];  // (declined: more speculative chains than the kernels track)
    if ((rc = read_frame_hdr(ctx, d_hdr, sl::H_DONE, cap_frames, n_frames, hdr, s)) != FG_OK) return rc;
    *consumed = hdr[sl::H_CONSUMED];
    *stop_reason = (int)hdr[sl::H_STOP];
    ctx->last_syslen_payload = hdr[sl::H_TOTAL];
    return FG_OK;
}

// ... for the chunks of n_segs connections at once (a SyslenSplitter per connection: input/tcp/tcp_input.rs:39-47)
int fg_frame_syslen_multi_device(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_seg_starts, uint64_t n_segs,
                                 uint8_t* d_packed, uint64_t* d_offsets, uint64_t* d_frame_starts, uint8_t* d_bad_utf8, uint64_t cap_frames,
                                 uint64_t* d_seg_first, uint64_t* d_seg_consumed, uint8_t* d_seg_stop, uint64_t* n_frames,
                                 uint64_t* payload_bytes, void* stream) {
    if (!ctx || !d_packed || !d_offsets || !n_frames || !payload_bytes || (nbytes && !d_bytes)) return FG_ERR_ARG;
    if (cap_frames && (!d_frame_starts || !d_bad_utf8)) return FG_ERR_ARG;
    if (n_segs ? (!d_seg_starts || !d_seg_first || !d_seg_consumed || !d_seg_stop) : nbytes != 0) return FG_ERR_ARG;
    if (((uintptr_t)d_bytes & 15u) != 0 || ((uintptr_t)d_packed & 15u) != 0) return FG_ERR_ARG;
    *n_frames = 0;
    *payload_bytes = 0;
    if (!fg_launch_syslen_multi || !fg_syslen_multi_scratch_bytes || !fg_syslen_max_bytes) return FG_ERR_UNSUPPORTED;  // (only in a build without the kernels: fg_ctx.hpp)
    if (nbytes > fg_syslen_max_bytes()) return FG_ERR_UNSUPPORTED;  // (the scratch keeps positions as 32-bit words)
    DeviceGuard g(ctx->device);
    hipStream_t s = stream_of(ctx, stream);
    if (nbytes == 0) return clear_segments(ctx, n_segs, d_offsets, d_seg_first, d_seg_consumed, d_seg_stop, FG_SYSLEN_CLEAN, s);
    if (n_segs > (1ull << 24)) return FG_ERR_UNSUPPORTED;  // (node numbers are 32-bit words)
    int rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_frame, &ctx->d_frame_cap, fg_syslen_multi_scratch_bytes(nbytes, n_segs))) != FG_OK) return rc;
    uint32_t* d_hdr = nullptr;
    FG_LAUNCH(ctx, fg_launch_syslen_multi(d_bytes, nbytes, d_seg_starts, n_segs, ctx->d_frame, d_packed, d_offsets, d_frame_starts, d_bad_utf8,
                                           cap_frames, d_seg_first, d_seg_consumed, d_seg_stop, &d_hdr, s));
    uint32_t hdr[kHdrWords];  // (declined: more speculative chains than the kernels track)
    if ((rc = read_frame_hdr(ctx, d_hdr, sl::H_DONE, cap_frames, n_frames, hdr, s)) != FG_OK) return rc;
    *payload_bytes = ctx->last_syslen_payload = hdr[sl::H_TOTAL];
    return FG_OK;
}

// replaces the walk of capnp::serialize::read_message over the segment tables in CapnpSplitter::run (splitter/capnp_splitter.rs:24-46)
int fg_frame_capnp_device(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, int final, uint64_t* d_offsets, uint64_t cap_frames,
                          uint64_t* n_frames, uint64_t* consumed, int* stop_reason, void* stream) {
    (void)final;  // (a message needs its whole body either way; what a TAIL means at the end of the stream is the caller's business)
    if (!ctx || !d_offsets || !n_frames || !consumed || !stop_reason || (nbytes && !d_bytes)) return FG_ERR_ARG;
    if (((uintptr_t)d_bytes & 15u) != 0) return FG_ERR_ARG;
    *n_frames = 0;
    *consumed = 0;
    *stop_reason = FG_CAPNP_CLEAN;
    if (nbytes > FG_CAPNP_FRAME_MAX_BYTES) return FG_ERR_ARG;  // (the scratch keeps word indices in 29 bits)
    if (!fg_launch_capnp_frame || !fg_capnp_frame_max_bytes || !fg_capnp_frame_scratch_bytes) return FG_ERR_UNSUPPORTED;  // (only in a build without the kernels: fg_ctx.hpp)
    if (nbytes > fg_capnp_frame_max_bytes()) return FG_ERR_ARG;
    DeviceGuard g(ctx->device);
    hipStream_t s = stream_of(ctx, stream);
    int rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_frame, &ctx->d_frame_cap, fg_capnp_frame_scratch_bytes(nbytes))) != FG_OK) return rc;
    uint32_t* d_hdr = nullptr;
    FG_LAUNCH(ctx, fg_launch_capnp_frame(d_bytes, nbytes, ctx->d_frame, d_offsets, cap_frames, &d_hdr, s));
    uint32_t hdr[kHdrWords];  // (declined: more nodes than the store holds)
    if ((rc = read_frame_hdr(ctx, d_hdr, cp::H_DONE, cap_frames, n_frames, hdr, s)) != FG_OK) return rc;
    *consumed = (uint64_t)hdr[cp::H_CONSUMED] * 8u;
    *stop_reason = (int)hdr[cp::H_STOP];
    return FG_OK;
}

// ... for the chunks of n_segs connections at once (a CapnpSplitter per connection: input/tcp/tcp_input.rs:39-47)
int fg_frame_capnp_multi_device(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_seg_starts, uint64_t n_segs,
                                uint64_t* d_offsets, uint8_t* d_kind, uint64_t cap_slots, uint64_t* d_seg_first, uint64_t* d_seg_consumed,
                                uint8_t* d_seg_stop, uint64_t* n_slots, void* stream) {
    if (!ctx || !d_offsets || !n_slots || (nbytes && !d_bytes) || (cap_slots && !d_kind)) return FG_ERR_ARG;
    if (n_segs ? (!d_seg_starts || !d_seg_first || !d_seg_consumed || !d_seg_stop) : nbytes != 0) return FG_ERR_ARG;
    if (((uintptr_t)d_bytes & 15u) != 0) return FG_ERR_ARG;
    *n_slots = 0;
    if (nbytes > FG_CAPNP_FRAME_MAX_BYTES || n_segs > (1ull << 24)) return FG_ERR_ARG;  // (word indices in 29 bits, node numbers in 32)
    if (!fg_launch_capnp_frame_multi || !fg_capnp_frame_multi_scratch_bytes) return FG_ERR_UNSUPPORTED;  // (only in a build without the kernels: fg_ctx.hpp)
    DeviceGuard g(ctx->device);
    hipStream_t s = stream_of(ctx, stream);
    if (nbytes == 0) return clear_segments(ctx, n_segs, d_offsets, d_seg_first, d_seg_consumed, d_seg_stop, FG_CAPNP_CLEAN, s);
    int rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_frame, &ctx->d_frame_cap, fg_capnp_frame_multi_scratch_bytes(nbytes, n_segs))) != FG_OK) return rc;
    uint32_t* d_hdr = nullptr;
    FG_LAUNCH(ctx, fg_launch_capnp_frame_multi(d_bytes, nbytes, d_seg_starts, n_segs, ctx->d_frame, d_offsets, d_kind, cap_slots, d_seg_first,
                                                d_seg_consumed, d_seg_stop, &d_hdr, s));
    uint32_t hdr[kHdrWords];  // (declined: more nodes than the store holds)
    return read_frame_hdr(ctx, d_hdr, cp::H_DONE, cap_slots, n_slots, hdr, s);
}

const char* fg_udp_error_string(uint8_t st) {
    switch (st) {
        case FG_UDP_RAW:
        case FG_UDP_ZLIB:
        case FG_UDP_GZIP: return "";
        case FG_UDP_BAD_ZLIB: return "Corrupted compressed (zlib) record";  // udp_input.rs:113
        case FG_UDP_BAD_GZIP: return "Corrupted compressed (gzip) record";  // udp_input.rs:124
        case FG_UDP_BAD_UTF8: return "Invalid UTF-8 input";                 // udp_input.rs:136
        case FG_UDP_TOO_LARGE: return "Compressed record inflates beyond max_inflated (not inflated on the GPU)";
        default: return nullptr;
    }
}

// ---- the sized resident calls (fg_udp_unpack_device, fg_udp_unpack_once_device, fg_deflate_device, fg_kafka_messageset_device,
// fg_kafka_wrap_device): a front half leaves the offsets and *total, a write half fills the caller's buffer.
extern "C++" {
namespace {
// What such an entry does between its argument checks and its write half, on s: n == 0 clears offsets[0] and waits; else front(),
// which leaves d_offsets_out[0 .. n] and synchronises for *total.  FG_SIZED_WRITE: the caller's buffer holds *total bytes -- the entry
// goes on to its write half (and waits for it or not, as it documents); anything else is the entry's answer: FG_OK for the sizing call
// (no buffer) and for n == 0, FG_ERR_ENT_OVERFLOW for a buffer that is too small, front()'s error.
constexpr int FG_SIZED_WRITE = 1;
template <class Front>
int sized_front(fg_ctx* ctx, hipStream_t s, uint64_t n, uint64_t* d_offsets_out, bool has_buffer, uint64_t cap, const uint64_t* total, Front&& front) {
    if (n == 0) {
        FG_HIP(ctx, hipMemsetAsync(d_offsets_out, 0, 8, s));
        FG_HIP(ctx, hipStreamSynchronize(s));
        return FG_OK;
    }
    const int rc = front();
    if (rc != FG_OK) return rc;
    if (!has_buffer) return FG_OK;  // the sizing call
    return *total > cap ? FG_ERR_ENT_OVERFLOW : FG_SIZED_WRITE;
}

// What a front half does around its sizing launch: the ctx's error word cleared (h_err; nullptr: the launch has none), the launch, the
// error word and the launch's other results (totals, counts) downloaded, one synchronisation of s.  FG_ERR_ARG: the kernel refused its
// input (the error word is set).
struct Download {
    void* host;
    const void* dev;
    size_t bytes;
};
template <class Launch>
int front_results(fg_ctx* ctx, hipStream_t s, uint32_t* h_err, const uint32_t* d_err, std::initializer_list<Download> words, Launch&& launch) {
    if (h_err) *h_err = 0;
    FG_LAUNCH(ctx, launch());
    if (h_err) FG_HIP(ctx, hipMemcpyAsync(h_err, d_err, 4, hipMemcpyDeviceToHost, s));
    for (const Download& w : words) FG_HIP(ctx, hipMemcpyAsync(w.host, w.dev, w.bytes, hipMemcpyDeviceToHost, s));
    FG_HIP(ctx, hipStreamSynchronize(s));
    return h_err && *h_err ? FG_ERR_ARG : FG_OK;
}

// ctx->d_udp as fg_udp_unpack_device lays it out for n datagrams: sizes | their per-64 sums
struct UdpSizes {
    uint32_t* d_sizes;
    uint64_t *d_sums, bytes;
    UdpSizes(uint8_t* b, uint64_t n) {
        Carver c{b};
        d_sizes = c.take<uint32_t>(n);
        d_sums = c.take<uint64_t>((n + 63) / 64, 8);
        bytes = c.off;
    }
};
// ... and as the one-walk form does: sizes | their per-64 sums | stage capacities | their sums | stage offsets [n + 1] | spilled flags |
// the spilled count (ctx->d_udp_stage holds the stages)
struct UdpOnce {
    uint32_t *d_sizes, *d_stage_sizes, *d_n_spilled;
    uint64_t *d_sums, *d_stage_sums, *d_stage_off, bytes;
    uint8_t* d_spilled;
    UdpOnce(uint8_t* b, uint64_t n) {
        Carver c{b};
        const uint64_t nb = (n + 63) / 64;
        d_sizes = c.take<uint32_t>(n);
        d_sums = c.take<uint64_t>(nb, 8);
        d_stage_sizes = c.take<uint32_t>(n);
        d_stage_sums = c.take<uint64_t>(nb, 8);
        d_stage_off = c.take<uint64_t>(n + 2, 8);
        d_spilled = c.take<uint8_t>(n);
        d_n_spilled = c.take<uint32_t>(1);
        bytes = c.off;
    }
};
}  // namespace
}  // extern "C++"

// replaces handle_record_maybe_compressed (input/udp_input.rs:100-143) up to decoder.decode, for a batch of datagrams
int fg_udp_unpack_device(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_offsets, uint64_t n, uint64_t max_inflated,
                         uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_offsets, uint8_t* d_drop, uint8_t* d_udp_status, uint64_t* total,
                         void* stream) {
    if (!ctx || !d_offsets || !d_out_offsets || !d_drop || !d_udp_status || !total || (nbytes && !d_bytes)) return FG_ERR_ARG;
    if (((uintptr_t)d_out & 15u) != 0) return FG_ERR_ARG;
    if (max_inflated == 0) max_inflated = FG_UDP_DEFAULT_MAX_INFLATED;
    if (max_inflated > FG_UDP_MAX_MAX_INFLATED) return FG_ERR_ARG;
    *total = 0;
    if (!fg_launch_udp_count || !fg_launch_udp_write || !fg_launch_udp_finish) return FG_ERR_UNSUPPORTED;  // (only in a build without the kernels: fg_ctx.hpp)
    DeviceGuard g(ctx->device);
    hipStream_t s = stream_of(ctx, stream);
    int rc = sized_front(ctx, s, n, d_out_offsets, d_out != nullptr, out_cap, total, [&]() -> int {
        const int grc = grow_dev(ctx, (void**)&ctx->d_udp, &ctx->d_udp_cap, UdpSizes(nullptr, n).bytes);
        if (grc != FG_OK) return grc;
        const UdpSizes u(ctx->d_udp, n);
        int lrc = fg_launch_udp_count(d_bytes, d_offsets, n, (uint32_t)max_inflated, u.d_sizes, u.d_sums, d_udp_status, d_drop, s);
        if (lrc == 0) lrc = fg_launch_encode_scan(u.d_sizes, u.d_sums, n, d_out_offsets, 0ull, s);
        FG_LAUNCH(ctx, lrc);
        FG_HIP(ctx, hipMemcpyAsync(total, d_out_offsets + n, 8, hipMemcpyDeviceToHost, s));
        FG_HIP(ctx, hipStreamSynchronize(s));
        return FG_OK;
    });
    if (rc != FG_SIZED_WRITE) return rc;
    rc = fg_launch_udp_write(d_bytes, d_offsets, n, d_out_offsets, d_out, out_cap, d_udp_status, d_drop, s);
    if (rc == 0) rc = fg_launch_udp_finish(d_bytes, d_offsets, n, d_out_offsets, d_out, out_cap, d_udp_status, d_drop, s);
    FG_LAUNCH(ctx, rc);
    FG_HIP(ctx, hipStreamSynchronize(s));
    return FG_OK;
}

// The front half of the one-walk form: every datagram walked once into its stage, d_out_offsets / d_drop / d_udp_status as
// fg_udp_unpack_device leaves them except for what the back half settles (the checksums of spilled rows, UTF-8), *total = the packed
// bytes.  Synchronises s once.  n > 0, max_inflated checked by the caller.
int fg_udp_once_front(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_offsets, uint64_t n, uint64_t max_inflated,
                      uint64_t* d_out_offsets, uint8_t* d_drop, uint8_t* d_udp_status, uint64_t* total, hipStream_t s) {
    ctx->udp_last_spilled = 0;
    if (!fg_launch_udp_stage || !fg_launch_udp_write_spilled || !fg_launch_udp_pack || !fg_udp_stage_bytes) return FG_ERR_UNSUPPORTED;  // (only in a build without the kernels: fg_ctx.hpp)
    int rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_udp, &ctx->d_udp_cap, UdpOnce(nullptr, n).bytes)) != FG_OK) return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_udp_stage, &ctx->d_udp_stage_cap, fg_udp_stage_bytes(nbytes, n))) != FG_OK) return rc;
    const UdpOnce u(ctx->d_udp, n);
    return front_results(ctx, s, nullptr, nullptr, {{total, d_out_offsets + n, 8}, {&ctx->udp_last_spilled, u.d_n_spilled, 4}}, [&] {
        return fg_launch_udp_stage(d_bytes, d_offsets, n, (uint32_t)max_inflated, u.d_stage_sizes, u.d_stage_sums, u.d_stage_off, ctx->d_udp_stage,
                                   ctx->d_udp_stage_cap, u.d_sizes, u.d_sums, d_out_offsets, d_udp_status, d_drop, u.d_spilled, u.d_n_spilled, s);
    });
}
// The back half, into d_out[0 .. out_cap) with out_cap >= the front half's total: the write walk for the spilled rows (when there are
// any), every other row from its stage or its datagram, UTF-8.  Queued on s, not waited for.
int fg_udp_once_pack(fg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n, const uint64_t* d_out_offsets, uint8_t* d_out,
                     uint64_t out_cap, uint8_t* d_drop, uint8_t* d_udp_status, hipStream_t s) {
    const UdpOnce u(ctx->d_udp, n);
    if (ctx->udp_last_spilled)
        FG_LAUNCH(ctx, fg_launch_udp_write_spilled(d_bytes, d_offsets, n, d_out_offsets, d_out, out_cap, d_udp_status, d_drop, u.d_spilled, s));
    FG_LAUNCH(ctx, fg_launch_udp_pack(d_bytes, d_offsets, n, d_out_offsets, d_out, out_cap, d_udp_status, d_drop, ctx->d_udp_stage, u.d_stage_off,
                                      ctx->d_udp_stage_cap, u.d_spilled, s));
    return FG_OK;
}

// fg_udp_unpack_device without the sizing call: one walk per stream (fg_udp.hip)
int fg_udp_unpack_once_device(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_offsets, uint64_t n, uint64_t max_inflated,
                              uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_offsets, uint8_t* d_drop, uint8_t* d_udp_status, uint64_t* total,
                              void* stream) {
    if (!ctx || !d_out || !d_offsets || !d_out_offsets || !d_drop || !d_udp_status || !total || (nbytes && !d_bytes)) return FG_ERR_ARG;
    if (((uintptr_t)d_out & 15u) != 0) return FG_ERR_ARG;
    if (max_inflated == 0) max_inflated = FG_UDP_DEFAULT_MAX_INFLATED;
    if (max_inflated > FG_UDP_MAX_MAX_INFLATED) return FG_ERR_ARG;
    *total = 0;
    ctx->udp_last_spilled = 0;
    DeviceGuard g(ctx->device);
    hipStream_t s = stream_of(ctx, stream);
    const int rc = sized_front(ctx, s, n, d_out_offsets, true, out_cap, total, [&] {
        return fg_udp_once_front(ctx, d_bytes, nbytes, d_offsets, n, max_inflated, d_out_offsets, d_drop, d_udp_status, total, s);
    });
    if (rc != FG_SIZED_WRITE) return rc;
    return fg_udp_once_pack(ctx, d_bytes, d_offsets, n, d_out_offsets, d_out, out_cap, d_drop, d_udp_status, s);  // (queued, NOT waited for)
}
uint64_t fg_udp_last_spilled(const fg_ctx* ctx) { return ctx ? ctx->udp_last_spilled : 0; }

// ---- the output compressor (fg_deflate.hip).  ctx->d_df_slots holds the slots the blocks are compressed into.
namespace {
// ctx->d_df, for n members: block counts | sizes | CRCs | the sums of the two scans (one after the other) | blk_first[n + 1] | the error
// word, the ticket word
struct DfMembers {
    uint32_t *d_nblk, *d_msize, *d_crc, *d_err, *d_ticket;
    uint64_t *d_sums, *d_blk_first, bytes;
    DfMembers(uint8_t* b, uint64_t n) {
        Carver c{b};
        d_nblk = c.take<uint32_t>(n);
        d_msize = c.take<uint32_t>(n);
        d_crc = c.take<uint32_t>(n);
        d_sums = c.take<uint64_t>((n + 63) / 64);
        d_blk_first = c.take<uint64_t>(n + 2, 8);
        d_err = c.take<uint32_t>(2);
        d_ticket = b ? d_err + 1 : nullptr;
        bytes = c.off;
    }
};
// ctx->d_df_blk, per block: size | CRC | offset in its member
struct DfBlocks {
    uint32_t *d_size, *d_crc, *d_rel;
    uint64_t bytes;
    DfBlocks(uint8_t* b, uint64_t nb) {
        Carver c{b};
        d_size = c.take<uint32_t>(nb);
        d_crc = c.take<uint32_t>(nb);
        d_rel = c.take<uint32_t>(nb);
        bytes = c.off;
    }
};
}  // namespace

int fg_deflate_front(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_cuts, uint64_t n_members, uint64_t* d_z_offsets,
                     uint64_t* total, hipStream_t s) {
    *total = 0;
    ctx->df_blocks = 0;
    if (!fg_launch_deflate_count || !fg_launch_deflate_blocks || !fg_launch_deflate_sizes || !fg_launch_deflate_pack || !fg_deflate_slot_bytes)
        return FG_ERR_UNSUPPORTED;  // (only in a build without the kernels: fg_ctx.hpp)
    const bool dyn = ctx->deflate_mode == FG_DEFLATE_DYNAMIC;
    if (dyn && !fg_launch_deflate_blocks_dyn) return FG_ERR_UNSUPPORTED;
    int rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_df, &ctx->d_df_cap, DfMembers(nullptr, n_members).bytes)) != FG_OK) return rc;
    const DfMembers m(ctx->d_df, n_members);
    uint64_t nb = 0;
    rc = front_results(ctx, s, &ctx->df_err, m.d_err, {{&nb, m.d_blk_first + n_members, 8}},
                       [&] { return fg_launch_deflate_count(d_cuts, n_members, nbytes, m.d_nblk, m.d_sums, m.d_blk_first, m.d_err, s); });
    if (rc != FG_OK) return rc;
    if (nb == 0) {  // (nothing but empty members: the cleared offsets are waited for, as the scan's are below)
        FG_HIP(ctx, hipMemsetAsync(d_z_offsets, 0, (n_members + 1) * 8, s));
        FG_HIP(ctx, hipStreamSynchronize(s));
        return FG_OK;
    }
    if ((rc = grow_dev(ctx, (void**)&ctx->d_df_blk, &ctx->d_df_blk_cap, DfBlocks(nullptr, nb).bytes)) != FG_OK) return rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_df_slots, &ctx->d_df_slots_cap, fg_deflate_slot_bytes(nbytes, nb))) != FG_OK) return rc;
    const DfBlocks b(ctx->d_df_blk, nb);
    FG_LAUNCH(ctx, (dyn ? fg_launch_deflate_blocks_dyn : fg_launch_deflate_blocks)(d_bytes, d_cuts, m.d_blk_first, n_members, nb, ctx->d_df_slots,
                                                                                   ctx->d_df_slots_cap, b.d_size, b.d_crc, m.d_ticket, fg::device_cus(), s));
    FG_LAUNCH(ctx, fg_launch_deflate_sizes(d_cuts, m.d_blk_first, n_members, b.d_size, b.d_crc, b.d_rel, m.d_crc, m.d_msize, m.d_sums, d_z_offsets, s));
    FG_HIP(ctx, hipMemcpyAsync(total, d_z_offsets + n_members, 8, hipMemcpyDeviceToHost, s));
    FG_HIP(ctx, hipStreamSynchronize(s));
    ctx->df_blocks = nb;
    return FG_OK;
}
int fg_deflate_pack(fg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_cuts, uint64_t n_members, const uint64_t* d_z_offsets, uint8_t* d_z,
                    uint64_t z_cap, hipStream_t s) {
    if (ctx->df_blocks == 0) return FG_OK;
    const DfMembers m(ctx->d_df, n_members);
    const DfBlocks b(ctx->d_df_blk, ctx->df_blocks);
    FG_LAUNCH(ctx, fg_launch_deflate_pack(d_bytes, d_cuts, m.d_blk_first, n_members, ctx->df_blocks, ctx->d_df_slots, b.d_size, b.d_rel, m.d_crc, d_z_offsets,
                                          d_z, z_cap, s));
    return FG_OK;
}

// output.kafka_compression = "gzip" for a resident stream (output/kafka_output.rs:163-182 compresses what it sends; here on the GPU)
int fg_deflate_device(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_cuts, uint64_t n_members, uint8_t* d_z, uint64_t z_cap,
                      uint64_t* d_z_offsets, uint64_t* total, void* stream) {
    if (!ctx || !d_cuts || !d_z_offsets || !total || (nbytes && !d_bytes)) return FG_ERR_ARG;
    if (n_members >= 0x7FFFFFFFull * 64u) return FG_ERR_ARG;
    *total = 0;
    if (!fg_launch_deflate_count) return FG_ERR_UNSUPPORTED;
    DeviceGuard g(ctx->device);
    hipStream_t s = stream_of(ctx, stream);
    int rc = sized_front(ctx, s, n_members, d_z_offsets, d_z != nullptr, z_cap, total,
                         [&] { return fg_deflate_front(ctx, d_bytes, nbytes, d_cuts, n_members, d_z_offsets, total, s); });
    if (rc != FG_SIZED_WRITE) return rc;
    if ((rc = fg_deflate_pack(ctx, d_bytes, d_cuts, n_members, d_z_offsets, d_z, z_cap, s)) != FG_OK) return rc;
    FG_HIP(ctx, hipStreamSynchronize(s));
    return FG_OK;
}

int fg_set_output_compression(fg_ctx* ctx, const fg_compress_cfg* cfg) {
    if (!ctx) return FG_ERR_ARG;
    if (!cfg) {
        ctx->compress = fg_compress_cfg{FG_COMP_NONE, 1u, 0u};
        return FG_OK;
    }
    // (FG_COMP_NONE keeps the member policy: nothing reads it but the message sets of FG_WIRE_KAFKA_V0, which are cut by it)
    if (cfg->codec != FG_COMP_GZIP && cfg->codec != FG_COMP_NONE) return FG_ERR_ARG;
    ctx->compress = *cfg;
    return FG_OK;
}
int fg_set_deflate_mode(fg_ctx* ctx, int mode) {
    if (!ctx || (mode != FG_DEFLATE_FIXED && mode != FG_DEFLATE_DYNAMIC)) return FG_ERR_ARG;
    ctx->deflate_mode = mode;
    return FG_OK;
}
int fg_last_compressed(const fg_ctx* ctx, fg_compressed* out) {
    if (!ctx || !out) return FG_ERR_ARG;
    *out = ctx->last_comp;
    return FG_OK;
}

// ---- Kafka v0 message sets (fg_kafka.hip).  ctx->d_kf_crc holds a CRC register per piece.
namespace {
// ctx->d_kf, for n messages: sizes [n + 1] | the scan's sums | the error word
struct KfSet {
    uint32_t *d_sizes, *d_err;
    uint64_t *d_sums, bytes;
    KfSet(uint8_t* b, uint64_t n) {
        Carver c{b};
        d_sizes = c.take<uint32_t>(n + 1);
        d_sums = c.take<uint64_t>((n + 63) / 64);
        d_err = c.take<uint32_t>(1);
        bytes = c.off;
    }
};
// ctx->d_kf_wrap, for n members: wrapper sizes | pieces | the sums of the two scans | piece_first[n + 1] | the error word
struct KfWrap {
    uint32_t *d_wsize, *d_npiece, *d_err;
    uint64_t *d_sums, *d_piece_first, bytes;
    KfWrap(uint8_t* b, uint64_t n) {
        Carver c{b};
        d_wsize = c.take<uint32_t>(n);
        d_npiece = c.take<uint32_t>(n);
        d_sums = c.take<uint64_t>((n + 63) / 64 * 2);
        d_piece_first = c.take<uint64_t>(n + 2, 8);
        d_err = c.take<uint32_t>(1);
        bytes = c.off;
    }
};
}  // namespace

int fg_kafka_set_front(fg_ctx* ctx, const uint64_t* d_offsets, const uint8_t* d_skip, uint64_t n, uint64_t nbytes, uint64_t* d_set_offsets, uint64_t* total,
                       hipStream_t s) {
    *total = 0;
    if (!fg_launch_kafka_sizes || !fg_launch_kafka_write) return FG_ERR_UNSUPPORTED;  // (only in a build without the kernels: fg_ctx.hpp)
    int rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_kf, &ctx->d_kf_cap, KfSet(nullptr, n).bytes)) != FG_OK) return rc;
    const KfSet m(ctx->d_kf, n);
    rc = front_results(ctx, s, &ctx->kf_err, m.d_err, {{total, d_set_offsets + n, 8}},
                       [&] { return fg_launch_kafka_sizes(d_offsets, d_skip, n, nbytes, m.d_sizes, m.d_sums, d_set_offsets, m.d_err, s); });
    if (rc == FG_ERR_ARG) *total = 0;  // (refused offsets: whatever the scan left is no size)
    return rc;
}
int fg_kafka_set_write(fg_ctx* ctx, const uint8_t* d_bytes, const uint64_t* d_offsets, const uint8_t* d_skip, uint64_t n, const uint64_t* d_set_offsets,
                       uint8_t* d_set, uint64_t set_cap, hipStream_t s) {
    FG_LAUNCH(ctx, fg_launch_kafka_write(d_bytes, d_offsets, d_skip, n, d_set_offsets, d_set, set_cap, fg::device_cus(), s));
    return FG_OK;
}
int fg_kafka_messageset_device(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_offsets, const uint8_t* d_skip, uint64_t n,
                               uint8_t* d_set, uint64_t set_cap, uint64_t* d_set_offsets, uint64_t* total, void* stream) {
    if (!ctx || !d_offsets || !d_set_offsets || !total || (nbytes && !d_bytes)) return FG_ERR_ARG;
    if (n >= 0x7FFFFFFFull * 64u) return FG_ERR_ARG;
    *total = 0;
    if (!fg_launch_kafka_sizes) return FG_ERR_UNSUPPORTED;
    DeviceGuard g(ctx->device);
    hipStream_t s = stream_of(ctx, stream);
    int rc = sized_front(ctx, s, n, d_set_offsets, d_set != nullptr, set_cap, total,
                         [&] { return fg_kafka_set_front(ctx, d_offsets, d_skip, n, nbytes, d_set_offsets, total, s); });
    if (rc != FG_SIZED_WRITE) return rc;
    if (*total == 0) return FG_OK;  // (every row skipped: nothing to write or to wait for)
    if ((rc = fg_kafka_set_write(ctx, d_bytes, d_offsets, d_skip, n, d_set_offsets, d_set, set_cap, s)) != FG_OK) return rc;
    FG_HIP(ctx, hipStreamSynchronize(s));
    return FG_OK;
}

int fg_kafka_wrap_front(fg_ctx* ctx, const uint64_t* d_z_offsets, uint64_t n_members, uint64_t* d_w_offsets, uint64_t* total, hipStream_t s) {
    *total = 0;
    ctx->kf_pieces = 0;
    if (!fg_launch_kafka_wrap_sizes || !fg_launch_kafka_wrap) return FG_ERR_UNSUPPORTED;  // (only in a build without the kernels: fg_ctx.hpp)
    int rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_kf_wrap, &ctx->d_kf_wrap_cap, KfWrap(nullptr, n_members).bytes)) != FG_OK) return rc;
    const KfWrap m(ctx->d_kf_wrap, n_members);
    uint64_t np = 0;
    rc = front_results(ctx, s, &ctx->kf_err, m.d_err, {{&np, m.d_piece_first + n_members, 8}, {total, d_w_offsets + n_members, 8}}, [&] {
        return fg_launch_kafka_wrap_sizes(d_z_offsets, n_members, m.d_wsize, m.d_npiece, m.d_sums, d_w_offsets, m.d_piece_first, m.d_err, s);
    });
    if (rc == FG_ERR_ARG) *total = 0;  // (refused offsets, as in fg_kafka_set_front)
    if (rc == FG_OK) ctx->kf_pieces = np;
    return rc;
}
int fg_kafka_wrap_write(fg_ctx* ctx, const uint8_t* d_z, const uint64_t* d_z_offsets, uint64_t n_members, const uint64_t* d_w_offsets, uint8_t* d_w,
                        uint64_t w_cap, hipStream_t s) {
    if (ctx->kf_pieces == 0) return FG_OK;  // (nothing but empty members)
    int rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_kf_crc, &ctx->d_kf_crc_cap, ctx->kf_pieces * 4)) != FG_OK) return rc;
    const KfWrap m(ctx->d_kf_wrap, n_members);
    FG_LAUNCH(ctx, fg_launch_kafka_wrap(d_z, d_z_offsets, m.d_piece_first, n_members, ctx->kf_pieces, d_w_offsets, d_w, w_cap, (uint32_t*)ctx->d_kf_crc,
                                        fg::device_cus(), s));
    return FG_OK;
}
int fg_kafka_wrap_device(fg_ctx* ctx, const uint8_t* d_z, const uint64_t* d_z_offsets, uint64_t n_members, uint8_t* d_w, uint64_t w_cap,
                         uint64_t* d_w_offsets, uint64_t* total, void* stream) {
    if (!ctx || !d_z_offsets || !d_w_offsets || !total) return FG_ERR_ARG;
    if (n_members >= 0x7FFFFFFFull * 64u) return FG_ERR_ARG;
    *total = 0;
    if (!fg_launch_kafka_wrap_sizes) return FG_ERR_UNSUPPORTED;
    DeviceGuard g(ctx->device);
    hipStream_t s = stream_of(ctx, stream);
    int rc = sized_front(ctx, s, n_members, d_w_offsets, d_w != nullptr, w_cap, total,
                         [&] { return fg_kafka_wrap_front(ctx, d_z_offsets, n_members, d_w_offsets, total, s); });
    if (rc != FG_SIZED_WRITE) return rc;
    if (*total && !d_z) return FG_ERR_ARG;
    if ((rc = fg_kafka_wrap_write(ctx, d_z, d_z_offsets, n_members, d_w_offsets, d_w, w_cap, s)) != FG_OK) return rc;
    FG_HIP(ctx, hipStreamSynchronize(s));
    return FG_OK;
}

int fg_set_output_wire(fg_ctx* ctx, int wire) {
    if (!ctx || (wire != FG_WIRE_RAW && wire != FG_WIRE_KAFKA_V0)) return FG_ERR_ARG;
    ctx->wire = wire;
    return FG_OK;
}

int fg_decode_frames_device(fg_ctx* ctx, fg_format fmt, fg_framing framing, const uint8_t* d_bytes, uint64_t nbytes,
                            const uint64_t* d_offsets, uint64_t n, const uint8_t* d_bad_utf8, const fg_tables* tables,
                            void* stream) {
    return fg_decode_frames_impl(ctx, fmt, framing, d_bytes, nbytes, d_offsets, n, d_bad_utf8, tables, stream, true, nbytes);
}

// reset_counter = false: a further slice of a batch whose entry counter is already live (the
// pipelined host paths decode one batch as several slices).  span_bytes = the bytes
// the n lines cover (the launch geometry is planned from the average line length; nbytes is only
// the readable range of d_bytes and, for a slice, covers the whole batch).
int fg_decode_frames_impl(fg_ctx* ctx, fg_format fmt, fg_framing framing, const uint8_t* d_bytes, uint64_t nbytes,
                              const uint64_t* d_offsets, uint64_t n, const uint8_t* d_bad_utf8, const fg_tables* tables,
                              void* stream, bool reset_counter, uint64_t span_bytes, uint32_t lane) {
    if ((int)framing < 0 || (int)framing > 2) return FG_ERR_ARG;
    if (fmt == FG_CAPNP && framing != FG_FRAME_NONE) return FG_ERR_ARG;  // (a chain of length prefixes: framed on the host)
    if (!ctx || !tables || (n && (!d_offsets || !tables->meta))) return FG_ERR_ARG;
    if (nbytes && !d_bytes) return FG_ERR_ARG;
    if (((uintptr_t)d_bytes & 15u) != 0) return FG_ERR_ARG;
    if (tables->n < n) return FG_ERR_ARG;
    if (tables->ent_cap > 0xFFFFFFFFull) return FG_ERR_ARG;
    DeviceGuard g(ctx->device);
    hipStream_t s = stream_of(ctx, stream);
    fg::DevTables dt = to_dev(*tables);
    if (dt.ent_used && reset_counter) FG_HIP(ctx, hipMemsetAsync(dt.ent_used, 0, 8, s));
    if (n == 0) return FG_OK;
    int rc;
    if ((rc = ensure_launch_state(ctx)) != FG_OK) return rc;
    uint64_t* stash = ctx->d_stash;
    if (lane) {  // (fg_ctx.hpp: the sliced fg_transcode_batch's odd slices)
        if (!ctx->d_stash2) FG_HIP(ctx, hipMalloc((void**)&ctx->d_stash2, fg_stash_bytes(ctx->stash_blocks)));
        stash = ctx->d_stash2;
    }
    dt.shares = ctx->table_shares ? ctx->table_shares : 1u;
    fg_launch_opts lo_call = ctx->lo;
    if (ctx->link_bound_waves && lo_call.waves_per_cu == 0) lo_call.waves_per_cu = ctx->link_bound_waves;
    if (ctx->defer_general && fmt == FG_GELF) {
        // the slices of one batch: one hand-over word for all of them, the exact form once behind the last (fg_finish_deferred_general)
        if (!ctx->batch_epoch) ctx->batch_epoch = next_epoch(ctx);
        dt.epoch = ctx->batch_epoch;
        lo_call.flags |= (uint32_t)FG_LO_RESERVED;
    } else {
        dt.epoch = next_epoch(ctx);
    }
    dt.pending = pending_word(ctx, dt.epoch);
    // the launch's ticket counter (dynamic chunk dispatch, fg_pipeline.hpp): one word of a ring per LAUNCH -- the slices of a batch may be
    // in flight on two streams at once and must not draw from one counter -- never reset: the host knows what every launch adds
    constexpr uint32_t kTicketRing = 1024;
    if (!ctx->d_ticket) {
        FG_HIP(ctx, hipMalloc((void**)&ctx->d_ticket, kTicketRing * sizeof(uint32_t)));
        FG_HIP(ctx, hipMemset(ctx->d_ticket, 0, kTicketRing * sizeof(uint32_t)));
        ctx->h_ticket.assign(kTicketRing, 0u);
    }
    const uint32_t tslot = ctx->ticket_seq++ % kTicketRing;
    fg::TicketSlot tk_slot{ctx->d_ticket + tslot, &ctx->h_ticket[tslot]};
    fg::TicketSlot* const tk = (ctx->lo.flags & FG_LO_STATIC_CHUNKS) ? nullptr : &tk_slot;
    if ((rc = timing_begin(ctx, s)) != FG_OK) return rc;
    const uint64_t avg_len = (span_bytes + n - 1) / n;
    switch (fmt) {
        case FG_RFC5424:
            rc = fg_launch_rfc5424(d_bytes, d_offsets, n, &dt, avg_len, s, stash, ctx->stash_blocks, (uint32_t)framing,
                                   d_bad_utf8, &lo_call, tk);
            break;
        case FG_LTSV:
            rc = fg_launch_ltsv(d_bytes, d_offsets, n, &dt, &ctx->ltsv, avg_len, s, stash, ctx->stash_blocks,
                                (uint32_t)framing, d_bad_utf8, &lo_call, tk);
            break;
        case FG_GELF:
            rc = fg_launch_gelf(d_bytes, d_offsets, n, &dt, avg_len, s, stash, ctx->stash_blocks,
                                (uint32_t)framing, d_bad_utf8, &lo_call, tk);
            break;
        case FG_RFC3164:
            if (!ctx->r3164_set) return FG_ERR_ARG;  // fg_set_rfc3164 first
            if ((rc = refresh_year(ctx)) != FG_OK) return rc;
{
                // (large batches: lines regrouped by shape -- fg_rfc3164.hip; the scratch is 16 bytes per line: the slow shapes' lists)
                const int regroup = (ctx->lo.flags & FG_LO_RFC3164_NO_REGROUP) ? 2 : (ctx->lo.flags & FG_LO_RFC3164_REGROUP) ? 1 : 0;
                uint8_t* scratch = nullptr;
                if (regroup != 2 && n < 0xFFFFFFFFull && (regroup == 1 || n >= fg_rfc3164_regroup_from()) && lane == 0u) {
                    if ((rc = grow_dev(ctx, (void**)&ctx->d_r3164, &ctx->d_r3164_cap, fg_rfc3164_scratch_bytes(n))) != FG_OK) return rc;
                    scratch = ctx->d_r3164;
                }
                rc = fg_launch_rfc3164(d_bytes, d_offsets, n, &dt, &ctx->r3164, pick_tile_cap(ctx, span_bytes, n, 56 * 1024), s, (uint32_t)framing,
                                       d_bad_utf8, scratch, regroup);
            }
            break;
        case FG_CAPNP:
            if (!fg_launch_capnp) return FG_ERR_UNSUPPORTED;  // (only in a build without the kernel: fg_ctx.hpp)
            rc = fg_launch_capnp(d_bytes, d_offsets, n, &dt, avg_len, s, d_bad_utf8, &lo_call, tk);
            break;
        default:
            return FG_ERR_UNSUPPORTED;
    }
    if (rc != 0) {
        // The launcher has already moved the host's copy of the launch's ticket word on (take_tickets) and the kernel that would have drawn
        // those tickets did not run: word and copy would differ for good, and every later launch on this slot of the ring would compute
        // chunk indices from a wrong base -- rows silently left undecoded.  Both go back to zero, behind whatever is queued.
        (void)hipMemsetAsync(ctx->d_ticket + tslot, 0, sizeof(uint32_t), s);
        ctx->h_ticket[tslot] = 0u;
        ctx->last_hip = rc;
        return FG_ERR_HIP;
    }
    return timing_end(ctx, s);
}


// FRAME + DECODE IN ONE KERNEL (fg_fused.hpp): the raw stream chunk d_bytes[0 .. nbytes) is framed by the decode kernel itself --
// rows into `tables` (tables->n = the rows it holds), frame starts into d_offsets (tables->n + 2 entries), and two result words in the
// ctx's scratch: (*d_total)[0] = the frames of the chunk (beyond tables->n: those rows were not written), (*d_total)[1] != 0 = a wave
// gave up waiting on the look-back (nothing is valid: run the separate framing + decode kernels).  Asynchronous on `stream`; nothing
// visits the host.  avg_line = the average frame length to plan for (0: the ctx's experience).  FG_ERR_UNSUPPORTED = this format /
// line length keeps the separate framing pass (RFC3164; long lines, whose kernels stage heads only): nothing was launched.
int fg_frame_decode_impl(fg_ctx* ctx, fg_format fmt, fg_framing framing, const uint8_t* d_bytes, uint64_t nbytes, int final, uint64_t* d_offsets,
                         uint64_t cap, const fg_tables* tables, uint64_t avg_line, void* stream, unsigned long long** d_total) {
    if (!ctx || !tables || !d_offsets || !d_total || (nbytes && !d_bytes)) return FG_ERR_ARG;
    if (framing != FG_FRAME_LINE && framing != FG_FRAME_NUL) return FG_ERR_ARG;
    if (fmt == FG_CAPNP) return FG_ERR_ARG;
    if (((uintptr_t)d_bytes & 15u) != 0 || tables->n < cap || (cap && !tables->meta) || tables->ent_cap > 0xFFFFFFFFull) return FG_ERR_ARG;
    if (fmt != FG_RFC5424 && fmt != FG_LTSV && fmt != FG_GELF) return FG_ERR_UNSUPPORTED;
    if (nbytes == 0 || cap == 0) return FG_ERR_UNSUPPORTED;
    if (avg_line == 0) avg_line = ctx->frames_per_byte > 0.0 ? (uint64_t)(1.0 / ctx->frames_per_byte + 0.5) : 200u;
    fg_launch_opts lo_call = ctx->lo;
    // Across the link the queue of outstanding reads IS the latency of every dependent one (a tile staged on, a tail scan, the exact
    // GELF form): 2048 waves x a 15 KiB window are 30 MB = half a millisecond at 57 GB/s, and a wave that waits that long holds the
    // look-back of every tile behind it.  Two waves per CU keep the link as full (a few hundred KB in flight do) with a sixteenth of
    // the queue: cfg2 0.864 -> 0.900 of the link, structured data 0.870 -> 0.878 (profiles/r06y_fused_host.log); GELF needs the
    // waves for its arithmetic (one per CU: 0.63) and keeps the link-bound grid of the other zero-copy launches.
    if (ctx->link_bound_waves && lo_call.waves_per_cu == 0) lo_call.waves_per_cu = fmt == FG_GELF ? ctx->link_bound_waves : 2u;
    const fg::FusedGeom g = fg::fused_geometry(fmt, avg_line, lo_call, ctx->link_bound_waves != 0);
    if (!g.ok) return FG_ERR_UNSUPPORTED;
    DeviceGuard guard(ctx->device);
    hipStream_t s = stream_of(ctx, stream);
    int rc;
    if ((rc = grow_dev(ctx, (void**)&ctx->d_fused, &ctx->d_fused_cap, fg::fused_scratch_bytes(nbytes, g.S))) != FG_OK) return rc;
    fg::DevTables dt = to_dev(*tables);
    if (dt.ent_used) FG_HIP(ctx, hipMemsetAsync(dt.ent_used, 0, 8, s));
    if ((rc = ensure_launch_state(ctx)) != FG_OK) return rc;
    dt.epoch = next_epoch(ctx);
    dt.pending = pending_word(ctx, dt.epoch);
    dt.n = cap;
    if ((rc = timing_begin(ctx, s)) != FG_OK) return rc;
    int lrc;
    switch (fmt) {
        case FG_RFC5424:
            lrc = fg_launch_rfc5424_fused(d_bytes, nbytes, &dt, &g, s, ctx->d_stash, ctx->stash_blocks, (uint32_t)framing, final, d_offsets, cap, ctx->d_fused,
                                          &lo_call, d_total);
            break;
        case FG_LTSV:
            lrc = fg_launch_ltsv_fused(d_bytes, nbytes, &dt, &ctx->ltsv, &g, s, ctx->d_stash, ctx->stash_blocks, (uint32_t)framing, final, d_offsets, cap,
                                       ctx->d_fused, &lo_call, d_total);
            break;
        default:
            lrc = fg_launch_gelf_fused(d_bytes, nbytes, &dt, &g, s, (uint32_t)framing, final, d_offsets, cap, ctx->d_fused, &lo_call, d_total);
            // the lines the fast form handed back: the exact form over the offsets the launch wrote (rows = its frame count, read on the device)
            if (lrc == 0) lrc = fg_launch_gelf_general_dev(d_bytes, d_offsets, cap, &dt, s, (uint32_t)framing, nullptr, *d_total);
            break;
    }
    FG_LAUNCH(ctx, lrc);
    return timing_end(ctx, s);
}

int fg_frame_decode_device(fg_ctx* ctx, fg_format fmt, fg_framing framing, const uint8_t* d_bytes, uint64_t nbytes, int final, uint64_t* d_offsets,
                           uint64_t cap_frames, const fg_tables* tables, uint64_t avg_line_hint, uint64_t* d_result, void* stream) {
    if (!d_result) return FG_ERR_ARG;
    unsigned long long* d_total = nullptr;
    const int rc = fg_frame_decode_impl(ctx, fmt, framing, d_bytes, nbytes, final, d_offsets, cap_frames, tables, avg_line_hint, stream, &d_total);
    if (rc != FG_OK) return rc;
    DeviceGuard guard(ctx->device);
    hipStream_t s = stream_of(ctx, stream);
    FG_HIP(ctx, hipMemcpyAsync(d_result, d_total, 16, hipMemcpyDeviceToDevice, s));
    return FG_OK;
}

#if defined(FG_FUSED_STATS)
// measurement variant only (FG_BUILD_VARIANT=stats): the counters / phase clocks the last fused launch of this ctx left (fg_fused.hpp)
extern "C" int fg_debug_fused_stats(fg_ctx* ctx, uint64_t out[16]) {
    if (!ctx || !ctx->d_fused) return FG_ERR_ARG;
    DeviceGuard guard(ctx->device);
    FG_HIP(ctx, hipDeviceSynchronize());
    FG_HIP(ctx, hipMemcpy(out, ctx->d_fused + fg::kFusedCounters * fg::kFusedCounterStride * 4u, 128, hipMemcpyDeviceToHost));
    return FG_OK;
}
#endif

// The exact form of GELF for ALL rows of a batch whose slices were decoded with ctx->defer_general set (a no-op when none was).
int fg_finish_deferred_general(fg_ctx* ctx, fg_framing framing, const uint8_t* d_bytes, const uint64_t* d_offsets, uint64_t n,
                               const uint8_t* d_bad_utf8, const fg_tables* tables, void* stream) {
    const uint32_t epoch = ctx->batch_epoch;
    ctx->batch_epoch = 0;
    ctx->defer_general = false;
    if (!epoch || n == 0) return FG_OK;
    DeviceGuard g(ctx->device);
    hipStream_t s = stream_of(ctx, stream);
    fg::DevTables dt = to_dev(*tables);
    dt.n = n;
    dt.epoch = epoch;
    dt.pending = pending_word(ctx, epoch);
    FG_LAUNCH(ctx, fg_launch_gelf_general(d_bytes, d_offsets, n, &dt, s, (uint32_t)framing, d_bad_utf8));
    return FG_OK;
}

namespace {
// fg_encode_device (total != nullptr: synchronises for the configuration's entry count and for the total) and
// fg_encode_device_async (total == nullptr: nothing on the host waits; ent_hint replaces the entry count read back)
int encode_device_impl(fg_ctx* ctx, fg_format src_fmt, const fg_encode_cfg* ecfg, const uint8_t* d_bytes, uint64_t nbytes,
                       const uint64_t* d_offsets, uint64_t n, const fg_tables* tables, uint8_t* d_out, uint64_t out_cap,
                       uint64_t* d_out_offsets, uint8_t* d_enc_status, uint64_t* total, uint64_t ent_hint, void* stream) {
    const bool async = total == nullptr;
    if (!ctx || !ecfg || !tables || !d_out_offsets || (n && (!d_offsets || !tables->meta))) return FG_ERR_ARG;
    if (async && !d_out) return FG_ERR_ARG;
    if ((int)src_fmt < 0 || (int)src_fmt > (int)FG_CAPNP) return FG_ERR_ARG;
    if (tables->n < n) return FG_ERR_ARG;
    if (((uintptr_t)d_bytes & 15u) != 0) return FG_ERR_ARG;  // (the emitters' global reader loads aligned 16-byte chunks: as the decoders require)
    DeviceGuard g(ctx->device);
    hipStream_t s = stream_of(ctx, stream);
    if (total) *total = 0;
    int rc;
    EncStage enc;
    if ((rc = stage_encoder(ctx, src_fmt, ecfg, n, n / 64 + 2, &enc)) != FG_OK) return rc;
    uint64_t ent_used = ~0ull;
    if (async && enc.image_bytes <= fg_ctx::kEncSlot) {
        // the configuration through a pinned ring: the copy is queued, nothing waits (a slot is reused four calls later; its
        // event has long fired by then)
        if (!ctx->h_enc_ring) {
            FG_HIP(ctx, hipHostMalloc((void**)&ctx->h_enc_ring, (size_t)fg_ctx::kEncRing * fg_ctx::kEncSlot, hipHostMallocDefault));
            for (uint32_t k = 0; k < fg_ctx::kEncRing; ++k) FG_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_enc[k], hipEventDisableTiming));
        }
        const uint32_t slot = ctx->enc_ring_next++ % fg_ctx::kEncRing;
        FG_HIP(ctx, hipEventSynchronize(ctx->ev_enc[slot]));
        uint8_t* hp = ctx->h_enc_ring + (size_t)slot * fg_ctx::kEncSlot;
        enc.write_image(hp);
        FG_HIP(ctx, hipMemcpyAsync(ctx->d_enc, hp, enc.image_bytes, hipMemcpyHostToDevice, s));
        FG_HIP(ctx, hipEventRecord(ctx->ev_enc[slot], s));
        ent_used = ent_hint;
    } else {
        std::vector<uint8_t> host(enc.image_bytes);
        enc.write_image(host.data());
        // (synchronous copy of a few hundred bytes: `host` goes out of scope at return); the same sync brings back the
        // number of entries the decode produced, which sizes the GELF ranking scratch
        FG_HIP(ctx, hipMemcpyAsync(ctx->d_enc, host.data(), host.size(), hipMemcpyHostToDevice, s));
        if (!async && ecfg->encoder == FG_ENC_GELF && tables->ent_used)
            FG_HIP(ctx, hipMemcpyAsync(&ent_used, tables->ent_used, 8, hipMemcpyDeviceToHost, s));
        FG_HIP(ctx, hipStreamSynchronize(s));
        if (async) ent_used = ent_hint;
    }
    fg::EncCfg& cfg = enc.cfg;
    pick_sort_slots(&cfg, ent_used, n);
    const uint32_t cfg_lds = enc.cfg_lds;
    uint32_t* const d_sizes = enc.d_sizes;
    uint64_t* const d_block_sums = enc.d_block_sums;
    fg::DevTables dt = to_dev(*tables);
    if (n == 0) {
        FG_HIP(ctx, hipMemsetAsync(d_out_offsets, 0, 8, s));
        return FG_OK;
    }
    // LDS tile of a 64-line group: average group + 6.25 % + 512 B, 4..40 KiB (longer groups read from global memory);
    // the tile is what limits the waves per CU (the emitters are latency-bound: occupancy is throughput)
    const uint32_t tile_cap = pick_tile_cap(ctx, nbytes, n, 40 * 1024, 1);
    if ((rc = timing_begin(ctx, s)) != FG_OK) return rc;
    FG_LAUNCH(ctx, fg_launch_encode_sizes(d_bytes, d_offsets, n, &dt, &cfg, tile_cap, cfg_lds, d_sizes, d_block_sums, d_enc_status, d_out_offsets, s));
    if (!async) {
        FG_HIP(ctx, hipMemcpyAsync(total, d_out_offsets + n, 8, hipMemcpyDeviceToHost, s));
        FG_HIP(ctx, hipStreamSynchronize(s));
        if (!d_out) return FG_OK;  // sizing call
        if (*total > out_cap) return FG_ERR_ENT_OVERFLOW;
    } else {
        cfg.out_cap = out_cap ? out_cap : 1;  // the write kernel reads out_offsets[n] itself and leaves d_out alone when it exceeds this
    }
    FG_LAUNCH(ctx, fg_launch_encode_write(d_bytes, d_offsets, n, &dt, &cfg, tile_cap, cfg_lds, d_out_offsets, d_out, d_sizes, s));
    return timing_end(ctx, s);  // count + scan + write (fg_last_kernel_ms)
}
}  // namespace

int fg_encode_device(fg_ctx* ctx, fg_format src_fmt, const fg_encode_cfg* ecfg, const uint8_t* d_bytes, uint64_t nbytes,
                     const uint64_t* d_offsets, uint64_t n, const fg_tables* tables, uint8_t* d_out, uint64_t out_cap,
                     uint64_t* d_out_offsets, uint8_t* d_enc_status, uint64_t* total, void* stream) {
    if (!total) return FG_ERR_ARG;
    return encode_device_impl(ctx, src_fmt, ecfg, d_bytes, nbytes, d_offsets, n, tables, d_out, out_cap, d_out_offsets, d_enc_status, total, 0, stream);
}

int fg_encode_device_async(fg_ctx* ctx, fg_format src_fmt, const fg_encode_cfg* ecfg, const uint8_t* d_bytes, uint64_t nbytes,
                           const uint64_t* d_offsets, uint64_t n, const fg_tables* tables, uint8_t* d_out, uint64_t out_cap,
                           uint64_t* d_out_offsets, uint8_t* d_enc_status, uint64_t ent_hint, void* stream) {
    return encode_device_impl(ctx, src_fmt, ecfg, d_bytes, nbytes, d_offsets, n, tables, d_out, out_cap, d_out_offsets, d_enc_status, nullptr,
                              ent_hint, stream);
}

int fg_encode_gelf_device(fg_ctx* ctx, fg_format src_fmt, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_offsets,
                          uint64_t n, const fg_tables* tables, const fg_gelf_extra* extra, uint8_t* d_out, uint64_t out_cap,
                          uint64_t* d_out_offsets, uint64_t* total, void* stream) {
    fg_encode_cfg ec{};
    ec.encoder = FG_ENC_GELF;
    ec.merger = FG_MERGE_NONE;
    if (extra) {
        ec.n_extra = extra->n;
        ec.extra_keys = extra->keys;
        ec.extra_values = extra->values;
    }
    return fg_encode_device(ctx, src_fmt, &ec, d_bytes, nbytes, d_offsets, n, tables, d_out, out_cap, d_out_offsets, nullptr, total, stream);
}

const char* fg_encode_error_string(uint8_t st) {
    switch (st) {
        case fg::ES_OK:
        case fg::ES_DECODE_FAILED: return "";
        case fg::ES_5424_DATE: return "Failed to parse date";                                         // rfc5424_encoder.rs:46
        case fg::ES_5424_FORMAT: return "Failed to parse date as Rfc3339 format";                     // rfc5424_encoder.rs:52
        case fg::ES_3164_TS: return "Failed to parse unix timestamp in RFC3164 encoder";              // rfc3164_encoder.rs:53
        case fg::ES_PASSTHROUGH_EMPTY: return "Cannot output empty raw message";                      // passthrough_encoder.rs:47
    }
    return nullptr;
}

const char* const kErr3164[] = {
    "",
    "Malformed RFC3164 event: Invalid priority",               // rfc3164_decoder.rs:128-130
    "Invalid priority",                                        // :136
    "Malformed RFC3164 event: Invalid timestamp or hostname",  // :121
    "Invalid time format",                                     // :158
    "Unable to parse RFC3164 date with year",                  // :176
    "Unable to parse the date in RFC3164 decoder",             // :211
    "<the reference panics here: index out of bounds (rfc3164_decoder.rs:67)>",
};

static int upload_tz(fg_ctx* ctx) {
    DeviceGuard g(ctx->device);
    if (ctx->d_tz) {
        (void)hipFree(ctx->d_tz);
        ctx->d_tz = nullptr;
    }
    ctx->r3164 = fg::r3164::Cfg{};
    ctx->r3164.current_year = ctx->r3164_year;
    if (ctx->tz_names.empty()) return FG_OK;
    fg::r3164::TzIndex idx;  // hash index, reject masks, year hints (fg_tz_index.hpp)
    if (!idx.build(ctx->tz_names, ctx->tz_first, ctx->tz_start, ctx->tz_off, ctx->r3164_year)) return FG_ERR_ARG;
    FG_HIP(ctx, hipMalloc((void**)&ctx->d_tz, idx.blob.size()));
    FG_HIP(ctx, hipMemcpy(ctx->d_tz, idx.blob.data(), idx.blob.size(), hipMemcpyHostToDevice));
    ctx->r3164.tz = idx.view(ctx->d_tz);
    return FG_OK;
}

int fg_set_rfc3164(fg_ctx* ctx, const fg_rfc3164_cfg* cfg) {
    if (!ctx || !cfg) return FG_ERR_ARG;
    ctx->r3164_auto_year = cfg->current_year == FG_YEAR_NOW;
    ctx->r3164_year = ctx->r3164_auto_year ? utc_year_now() : cfg->current_year;
    ctx->tz_names.clear();
    ctx->tz_first.clear();
    ctx->tz_start.clear();
    ctx->tz_off.clear();
    if (cfg->tz && cfg->tz->n_zones) {
        const fg_tz_table* t = cfg->tz;
        if (!t->names || !t->zone_first || !t->utc_start || !t->utc_offset) return FG_ERR_ARG;
        for (uint32_t z = 0; z < t->n_zones; ++z) {
            if (!t->names[z] || t->zone_first[z + 1] <= t->zone_first[z]) return FG_ERR_ARG;
            if (z && strcmp(t->names[z - 1], t->names[z]) >= 0) return FG_ERR_ARG;  // sorted bytewise, unique
            ctx->tz_names.emplace_back(t->names[z]);
        }
        ctx->tz_first.assign(t->zone_first, t->zone_first + t->n_zones + 1);
        const uint32_t ne = t->zone_first[t->n_zones];
        ctx->tz_start.assign(t->utc_start, t->utc_start + ne);
        ctx->tz_off.assign(t->utc_offset, t->utc_offset + ne);
    }
    ctx->r3164_set = true;
    return upload_tz(ctx);
}

// capnp_splitter.rs:135,140; [3] has no counterpart: the reference unwrap()s get_root() (:47) and the connection thread panics
const char* const kErrCapnp[] = {"", "Missing timestamp", "Missing host name", "Capnp decoding error: the root pointer cannot be read"};

const char* fg_error_string(fg_format fmt, uint8_t status) {
    if (status == FG_ST_BAD_UTF8) return "Invalid UTF-8 input";  // line_splitter.rs:23, nul_splitter.rs:36
    switch (fmt) {
        case FG_RFC5424:
            return status < sizeof(kErr5424) / sizeof(*kErr5424) ? kErr5424[status] : nullptr;
        case FG_LTSV:
            return status < sizeof(kErrLtsv) / sizeof(*kErrLtsv) ? kErrLtsv[status] : nullptr;
        case FG_GELF:
            return status < sizeof(kErrGelf) / sizeof(*kErrGelf) ? kErrGelf[status] : nullptr;
        case FG_RFC3164:
            return status < sizeof(kErr3164) / sizeof(*kErr3164) ? kErr3164[status] : nullptr;
        case FG_CAPNP:
            return status < sizeof(kErrCapnp) / sizeof(*kErrCapnp) ? kErrCapnp[status] : nullptr;
    }
    return nullptr;
}

int fg_shard_plan(const uint64_t* offsets, uint64_t n, uint32_t g, uint64_t* line_starts) {
    if (!line_starts || g == 0 || (n && !offsets)) return FG_ERR_ARG;
    line_starts[0] = 0;
    line_starts[g] = n;
    if (n == 0) {
        for (uint32_t k = 1; k < g; ++k) line_starts[k] = 0;
        return FG_OK;
    }
    const uint64_t b0 = offsets[0], total = offsets[n] - b0;
    uint64_t lo = 0;
    for (uint32_t k = 1; k < g; ++k) {
        // first line whose start is >= k/g of the bytes (binary search; offsets is non-decreasing)
        uint64_t target = b0 + (uint64_t)((__uint128_t)total * k / g);
        uint64_t a = lo, b = n;
        while (a < b) {
            uint64_t m = a + (b - a) / 2;
            if (offsets[m] < target) a = m + 1;
            else b = m;
        }
        line_starts[k] = a;
        lo = a;
    }
    return FG_OK;
}

}  // extern "C"
