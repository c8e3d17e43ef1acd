/*
 * fg_hip.h -- C ABI of libfg_hip: the MI355X (gfx950) bulk log-line decoder that replaces
 * flowgger's per-line Decoder::decode() hot path.
 *
 * Reference interface replaced (paths relative to the flowgger source tree):
 *   trait Decoder { fn decode(&self, line:&str) -> Result<Record,&'static str> }
 *                                                   src/flowgger/decoder/mod.rs:44-46
 *   RFC5424Decoder::decode                          src/flowgger/decoder/rfc5424_decoder.rs:17-50
 *   LTSVDecoder::new / decode                       src/flowgger/decoder/ltsv_decoder.rs:23-221
 *   GelfDecoder::decode                             src/flowgger/decoder/gelf_decoder.rs:34-125
 *   RFC3164Decoder::decode                          src/flowgger/decoder/rfc3164_decoder.rs:31-213
 *   Record / StructuredData / SDValue               src/flowgger/record.rs:3-82
 *   the per-line call site the batching framer replaces
 *                                                   src/flowgger/splitter/line_splitter.rs:44-54
 *
 * Model: the framer packs N framed lines (valid UTF-8, framing bytes already stripped exactly
 * as BufRead::lines()/split(0)/syslen do) into one byte buffer + an offset array and makes ONE
 * call; hand-written HIP kernels tokenise every line and emit field-offset TABLES (struct of
 * arrays below).  A `Record` identical to the reference decoder's is materialised from a table
 * row + the line bytes (fg_tables_serialize / the Rust shim in INTEGRATION.md).  Errors are
 * part of the result: status[i] != 0 indexes the reference's exact &'static str.
 *
 * Plain C, plain pointers and sizes; no torch / C++ types.  All functions return 0 on success
 * or a negative FG_ERR_* (never throw, never abort).
 */
#ifndef FG_HIP_H
#define FG_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FG_ABI_VERSION 4 /* 4 (round 6): fg_frame_decode_device (framing inside the decode kernels), FG_LO_NO_FUSED_FRAMING, fg_launch_opts.fused_look / fused_ext (the struct grew), fg_last_host_path; 3 (round 5): fg_launch_opts.ent_chunk (the struct grew), FG_LO_STATIC_CHUNKS / _FRAME_SELFTEST_STALL, fg_ticket_ring_check; 2 (round 4): FG_YEAR_NOW = INT32_MIN, FG_F_LTSV_NOVALUE and the failed-LTSV-row count, ent_used = RESERVED slots, fg_calibrate_device */

/* FG_CAPNP (input.format = "capnp", splitter/capnp_splitter.rs:65-167): a "line" of the batch is ONE WHOLE Cap'n Proto message
 * INCLUDING its segment table; offsets[i] must be multiples of 8 (a message is an array of 8-byte words; the host-buffer entry
 * points answer FG_ERR_ARG otherwise, fg_decode_batch_device -- whose offsets live on the device -- gives such a row status 3);
 * spans are relative to offsets[i] as for every other format.  FG_FRAME_NONE and FG_FRAME_CAPNP are valid with it: a capnp stream is a chain
 * of length prefixes, framed where it lies by fg_frame_capnp_device (or by the host-buffer entry points with FG_FRAME_CAPNP) or on
 * the host (flowgger_amd/host/fg_decoder.hpp CapnpFramer).  FG_CAPNP is an additive value
 * under the same FG_ABI_VERSION: a library without it rejects it with FG_ERR_ARG / FG_ERR_UNSUPPORTED.  All six encoders and the
 * mergers take FG_CAPNP tables (fg_encode_device, fg_encode_device_async, fg_transcode_batch with FG_FRAME_NONE): the relay's
 * handle_message + encoder.encode (capnp_splitter.rs:47-60) is one fg_transcode_batch.  The passthrough encoder emits the
 * message's full_msg text, not the message. */
typedef enum fg_format { FG_RFC5424 = 0, FG_LTSV = 1, FG_GELF = 2, FG_RFC3164 = 3, FG_CAPNP = 4 } fg_format;

/* return codes */
enum {
    FG_OK = 0,
    FG_ERR_ARG = -1,       /* NULL / inconsistent arguments */
    FG_ERR_HIP = -2,       /* a HIP runtime call failed (fg_last_hip_error has the code) */
    FG_ERR_NO_DEVICE = -3, /* no gfx950 device / kernels not loadable: there is NO CPU fallback */
    FG_ERR_ENT_OVERFLOW = -4, /* entry table too small; tables are valid except status==FG_ST_OVERFLOW rows */
    FG_ERR_UNSUPPORTED = -5,
    FG_ERR_NOMEM = -6      /* host allocation failed */
};

/* SDValue discriminants (record.rs:3-11) + the SD-element marker used in the entry table */
enum {
    FG_T_STRING = 0, FG_T_BOOL = 1, FG_T_F64 = 2, FG_T_I64 = 3, FG_T_U64 = 4, FG_T_NULL = 5,
    FG_T_SDID = 6 /* entry opens a new StructuredData element; name = its sd_id */
};

/* A byte span inside ONE line: off is relative to the line's first byte (offsets[i]).
 * len == FG_NONE means Option::None. */
#define FG_NONE 0xFFFFFFFFu
typedef struct fg_span { uint32_t off; uint32_t len; } fg_span;

/* meta word: status | facility<<8 | severity<<16 | flags<<24
 *   status   0 = Ok, else the format's error index (fg_error_string)
 *   facility / severity  0xFF = None
 *   flags    FG_F_* */
#define FG_META_STATUS(m)   ((uint8_t)((m) & 0xFF))
#define FG_META_FACILITY(m) ((uint8_t)(((m) >> 8) & 0xFF))
#define FG_META_SEVERITY(m) ((uint8_t)(((m) >> 16) & 0xFF))
#define FG_META_FLAGS(m)    ((uint8_t)(((m) >> 24) & 0xFF))
enum {
    FG_F_TS_NOW = 1,        /* GELF without "timestamp": Record.ts = wall clock at materialisation (gelf_decoder.rs:109) */
    FG_F_HOST_ESC = 2,      /* GELF: hostname span holds JSON escapes (decode when materialising) */
    FG_F_MSG_ESC = 4,       /* GELF: short_message span holds JSON escapes */
    FG_F_FULLMSG_ESC = 8,   /* GELF: full_message span holds JSON escapes */
    FG_F_BOM = 16,          /* RFC5424: line started with U+FEFF (spans already skip it) */
    FG_F_GELF_RETRY = 32,   /* GELF: accepted via the '\n' -> "\\n" retry (gelf_decoder.rs:44-46); when decoding
                               escapes a backslash followed by a raw LF means backslash + 'n' */
    FG_F_MSG_JOIN = 64,     /* RFC3164 standard form: Record.msg = the msg span's whitespace-separated tokens joined
                               with single spaces (`_log_tokens[1..].join(" ")`, rfc3164_decoder.rs:70) */
    FG_F_LTSV_NOVALUE = 128 /* LTSV: the line has tab-separated parts without ':'; the reference println!s
                               "Missing value for name '{}'" for each while it decodes (ltsv_decoder.rs:99) -- set on Ok AND on
                               failed rows (a failed row's hostname.off = how many parts had been reported when the decode
                               stopped; the same number, saturated at 254, is in its facility byte for callers that only
                               see the meta column).  fg_tables_stdout reproduces the text. */
};
#define FG_ST_OVERFLOW 0xFE /* status: the line's entries did not get slots: the table (ent_cap) is used up, counting the slots
                               parked in other waves' reservations (see ent_used).  Re-run with more; all other rows are valid */
#define FG_ST_BAD_UTF8 0xFD /* status: the frame is not valid UTF-8; the reference never decodes it, it prints
                               "Invalid UTF-8 input" and drops it (line_splitter.rs:22-25, nul_splitter.rs:34-40) */

/* How the frames handed to the decoders are delimited inside the byte buffer. */
typedef enum fg_framing {
    FG_FRAME_NONE = 0, /* offsets delimit bare lines (framing bytes already stripped by the caller) */
    FG_FRAME_LINE = 1, /* BufRead::lines(): "\n" terminated, the "\n" and one preceding "\r" are not part of the line */
    FG_FRAME_NUL = 2,  /* BufRead::split(0): "\0" terminated */
    FG_FRAME_SYSLEN = 3, /* RFC 6587 octet counting (splitter/syslen_splitter.rs:17-57): "<len> " followed by exactly len bytes, untrimmed
                           (a trailing "\n" belongs to the message); framed by fg_frame_syslen_device and by the host-buffer entry points
                           fg_frame_decode_batch / fg_transcode_batch.  An additive value under the same FG_ABI_VERSION: a library without
                           it rejects it with FG_ERR_ARG / FG_ERR_UNSUPPORTED */
    FG_FRAME_CAPNP = 4  /* a Cap'n Proto stream (splitter/capnp_splitter.rs:24-46, capnp::serialize::read_message): a segment table, then
                           the words it counts; frame i is one whole message, its table included.  Valid with FG_CAPNP only (FG_ERR_ARG
                           otherwise), framed by fg_frame_capnp_device and by fg_frame_decode_batch / fg_transcode_batch.  An additive
                           value under the same FG_ABI_VERSION */
} fg_framing;

/* How the chain of segment tables of an FG_FRAME_CAPNP chunk ended (fg_frame_capnp_device, fg_last_capnp_stop).  The whole messages
 * in front of `consumed` are valid output in every case: the reference handles them first and ends the connection afterwards. */
typedef enum fg_capnp_stop {
    FG_CAPNP_CLEAN = 0,             /* consumed == nbytes: the chunk ended on a message boundary */
    FG_CAPNP_TAIL = 1,              /* the table or the body of the message at `consumed` runs past nbytes (fewer than 8 bytes left
                                       included): carry bytes[consumed ..) over */
    FG_CAPNP_TOO_MANY_SEGMENTS = 2, /* the table at `consumed` counts 512 segments or more: "Too many segments", the connection is over */
    FG_CAPNP_TOO_LARGE = 3          /* its sizes add up to more than 8 Mi words: "Message has N words, which is too large" */
} fg_capnp_stop;

/* How the "<len> " chain of an FG_FRAME_SYSLEN chunk ended (fg_frame_syslen_device, fg_last_syslen_stop): what the caller does next
 * to reproduce SyslenSplitter::run (syslen_splitter.rs:42-57). */
typedef enum fg_syslen_stop {
    FG_SYSLEN_CLEAN = 0,      /* consumed == nbytes: the chunk ended on a frame boundary.  At the end of the stream read_until returns
                                 Ok(0): "Can't read message's length" */
    FG_SYSLEN_TAIL = 1,       /* the prefix or the payload at `consumed` runs past nbytes.  Not final: carry bytes[consumed ..) over.
                                 Final: EOF inside the length (the reference drops the last byte it read, parses the rest, and
                                 read_exact fails) or inside the payload ("failed to fill whole buffer") -- the host code
                                 (flowgger_amd/host/fg_decoder.hpp) tells the two apart on the few bytes of the tail */
    FG_SYSLEN_BAD_LEN = 2,    /* the bytes at `consumed` are no length (a lone ' ', a non-digit, '+' alone, a value beyond 64 bits):
                                 "Can't read message's length", the connection is over */
    FG_SYSLEN_LONG_PREFIX = 3 /* the prefix at `consumed` is longer than FG_SYSLEN_MAX_PREFIX bytes (leading zeros: legal, never seen):
                                 the caller hops that one frame on the host and resubmits the rest */
} fg_syslen_stop;
#define FG_SYSLEN_MAX_PREFIX 24u /* bytes of a "<len> " prefix, the ' ' included, the device parser reads */

/* Bytes of the "<len> " prefix of an FG_FRAME_SYSLEN frame as fg_frame_decode_batch / fg_transcode_batch return it (`frame` = its
 * first byte, frame_len = off[i + 1] - off[i]): the payload -- what the table's spans are relative to -- starts that many bytes in. */
static inline uint32_t FG_SYSLEN_PREFIX_LEN(const uint8_t* frame, uint64_t frame_len) {
    uint32_t k = 0;
    while (k < frame_len && frame[k] != (uint8_t)' ') ++k;
    return k < frame_len ? k + 1u : (uint32_t)frame_len;
}

/* entry flags */
enum {
    FG_EF_VAL_ESC = 1,   /* value span needs unescaping: RFC5424 \" \\ \] (rfc5424_decoder.rs:105-125) or JSON escapes (GELF) */
    FG_EF_NAME_ESC = 2,  /* GELF: key span holds JSON escapes */
    FG_EF_SUFFIX = 4,    /* LTSV: append the configured type suffix to the name (ltsv_decoder.rs:131-136) */
    FG_EF_NAME_VERBATIM = 8 /* FG_CAPNP: the Record key is the name span as it is -- the `extra` pairs (capnp_splitter.rs:104-108);
                               every other FG_CAPNP name gets a leading '_' unless the span starts with one (:80-87), the rule of
                               the GELF rows */
};

/* One entry = one (name, SDValue) pair or one SD-element header, 18 bytes as SoA:
 *   ent_name[k]  span of the name WITHOUT the leading '_' the decoders add (sd_id for FG_T_SDID)
 *   ent_val[k]   String: span packed as off | (uint64)len<<32 ; Bool: 0/1 ; F64: IEEE bits ;
 *                I64: two's complement ; U64: value ; Null/SDID: 0
 *   ent_type[k]  FG_T_*      ent_flags[k]  FG_EF_*
 * LTSV / GELF rows have ONE element without an id and no FG_T_SDID entry: their entries are its pairs.  An FG_CAPNP row whose
 * Record.sd is Some opens with ONE FG_T_SDID entry -- its name span has len == FG_NONE when sd_id is None (malformed messages
 * only; a null pointer is Some("") = a span of length 0) -- followed by the kept pairs, then the kept extras; ent_count == 0 is
 * sd == None.  (The element needs its entry even without an id: Some([{None, []}]) and None are different Records.)  An optional
 * text of an FG_CAPNP row that is None (its getter failed) is a span with len == FG_NONE.
 * Line i owns entries [ent_first[i], ent_first[i]+ent_count[i]) in decoder order.  Slices of
 * different lines may appear in any order inside the entry table (wave-level allocation). */
typedef struct fg_tables {
    uint64_t n;          /* rows (lines) */
    uint64_t ent_cap;    /* capacity of the ent_* arrays, in entries */
    uint32_t* meta;      /* [n] */
    double*   ts;        /* [n] Record.ts, bit-exact (utils/mod.rs:23-28) */
    fg_span*  hostname;  /* [n] */
    fg_span*  appname;   /* [n] */
    fg_span*  procid;    /* [n] */
    fg_span*  msgid;     /* [n] */
    fg_span*  msg;       /* [n] */
    fg_span*  full_msg;  /* [n] */
    uint32_t* ent_first; /* [n] */
    uint32_t* ent_count; /* [n] */
    fg_span*  ent_name;  /* [ent_cap] */
    uint64_t* ent_val;   /* [ent_cap] */
    uint8_t*  ent_type;  /* [ent_cap] */
    uint8_t*  ent_flags; /* [ent_cap] */
    uint64_t* ent_used;  /* [1] entry slots RESERVED by the call (may exceed ent_cap on overflow).  Waves reserve slots in
                            chunks (one atomic per chunk instead of one per line group), so this is >= the sum of ent_count and
                            the range [0, ent_used) contains slots no row refers to (uninitialised holes): always walk the
                            entries through ent_first / ent_count.  Sizing ent_cap: a table with fewer than 256 slots per
                            resident wave x 16 (ent_cap < ~8 M on an MI355X) gets exact reservations -- no slack needed
                            beyond the entries themselves; above that, up to ent_cap / 16 slots plus one line's entries per
                            chunk (at most 4096 slots) can be stranded: size from the input bytes (the host-buffer entry points use
                            nbytes / 16 for RFC5424, nbytes / 8 otherwise) and retry with ent_used + ent_used / 8 on
                            FG_ERR_ENT_OVERFLOW, as they do. */
} fg_tables;

/* Fixed table bytes written per line (meta 4 + ts 8 + 6 spans 48 + ent_first/count 8). */
#define FG_ROW_BYTES 68u
#define FG_ENT_BYTES 18u

/* LTSVDecoder::new configuration (input.ltsv_schema / input.ltsv_suffixes, ltsv_decoder.rs:24-84).
 * Names are matched byte-exactly; types are FG_T_STRING..FG_T_U64. */
typedef struct fg_cfg {
    uint32_t n_schema;
    const char* const* schema_names;
    const uint8_t* schema_types;
    const char* suffix_bool; /* NULL = None */
    const char* suffix_f64;
    const char* suffix_i64;
    const char* suffix_u64;
} fg_cfg;

/* RFC3164Decoder configuration.  The reference takes two things from its environment that are configuration here:
 *   current_year  OffsetDateTime::now_utc().year() prepended to dates without a year (rfc3164_decoder.rs:179): a fixed
 *                 year (tests, replays), or FG_YEAR_NOW = what the reference does -- the library re-reads the UTC year
 *                 at every FG_RFC3164 decode call, so a long-lived decoder (and its clones) crosses New Year correctly
 *   tz            the IANA zone table behind time_tz::timezones::get_by_name (rfc3164_decoder.rs:195; the time-tz
 *                 crate embeds the tz database at build time): n_zones names SORTED BYTEWISE (exact match), zone i
 *                 owns entries [zone_first[i], zone_first[i+1]) of (utc_start, utc_offset): utc_offset[k] seconds east
 *                 of UTC are in effect from utc_start[k] on, the zone's first entry starts at INT64_MIN.  NULL = no
 *                 zone name is recognised.  flowgger_amd/tzdb.py builds it from the system's TZif files. */
typedef struct fg_tz_table {
    uint32_t n_zones;
    const char* const* names;
    const uint32_t* zone_first;
    const int64_t* utc_start;
    const int32_t* utc_offset;
} fg_tz_table;
/* current_year: follow the wall clock (UTC year re-read at every FG_RFC3164 decode call).  Outside every representable year
 * (INT32_MIN), so that year 0 -- which `time` accepts -- can be configured explicitly. */
#define FG_YEAR_NOW (-2147483647 - 1)
typedef struct fg_rfc3164_cfg {
    int32_t current_year;
    const fg_tz_table* tz;
} fg_rfc3164_cfg;

typedef struct fg_ctx fg_ctx;
#define FG_STREAM_OWN ((void*)(intptr_t)-1)

int fg_abi_version(void);

/* Launch-geometry overrides of a ctx: the parity sweeps over the kernel variants (tests/) and tuning (tools/) set them through
 * this call.  The library reads NO environment variables (a stray FG_* in a daemon's environment must not change how it runs);
 * a zero field = the library's own choice; results are identical for every setting.  Clones made afterwards inherit them.
 * opts == NULL restores the defaults. */
typedef struct fg_launch_opts {
    uint32_t lines_per_group; /* lines a wave takes per group, 1..64 */
    uint32_t tile_cap;        /* LDS tile bytes (rounded up to 1 KiB) */
    uint32_t waves_per_cu;    /* upper bound of resident waves per CU */
    uint32_t gelf_lds_budget; /* GELF: LDS bytes per wave the lines per group are fitted to */
    uint32_t gelf_window_kib; /* GELF: register prefetch window in KiB (2..6) */
    uint32_t flags;           /* FG_LO_* */
    uint32_t chunk_lines;     /* lines a wave takes at a time (the first chunk by block index, further ones drawn by ticket), 1..65536 */
    uint32_t ent_chunk;       /* entry slots a wave reserves from the table's counter at a time: 1 = exactly what each request needs,
                                 >= 2 = that many (tuning: fewer atomics on the one counter word against slots stranded at the end of
                                 every wave's last reservation) */
    uint32_t fused_look;      /* fused frame + decode launches (fg_frame_decode_device): bytes staged behind a tile, where its last line ends
                                 (a multiple of 16; the library's own choice: one average line) */
    uint32_t fused_ext;       /* ... bytes staged ON at a time when that line runs past them (a multiple of 16, at most 1024) */
} fg_launch_opts;
enum {
    FG_LO_GELF_GENERIC = 1,        /* GELF: the run-time-geometry kernel even where the constant-geometry instantiation applies */
    FG_LO_TRANSCODE_ONE_PIECE = 2, /* fg_transcode_batch / fg_frame_decode_batch: never slice a large batch over the streams */
    FG_LO_NO_HEAD = 4,             /* RFC5424: stage whole lines even when they are long (the head-only kernel is the default from 768 B) */
    FG_LO_FORCE_HEAD = 8,          /* RFC5424: the head-only kernel for lines of any length (parity sweeps) */
    FG_LO_SD_WALK = 16,            /* RFC5424: the lane-per-line structured-data walker even for long lines (the pair-parallel walk is the
                                      default from an average of 320 bytes per line) */
    FG_LO_SD_PAIRS = 32,           /* RFC5424: the pair-parallel structured-data walk for lines of any length (parity sweeps) */
    FG_LO_NO_ZERO_COPY = 64,       /* fg_decode_batch: the sliced hipMemcpy pipeline even when the caller's buffers are pinned (A/B, tests) */
    FG_LO_FRAME_KERNEL_UPLOAD = 128, /* fg_frame_decode_batch, pinned chunk: the framing scan reads the chunk in place and stores it to HBM
                                      itself instead of hipMemcpy uploads (measured slower on MI355X / ROCm 7.2: off by default) */
    FG_LO_FRAME_CLASSIC = 256,     /* framing: the three-kernel form (masks to HBM, one-workgroup scan, emit) instead of the one-pass chained
                                      scan -- which falls back to it by itself should its look-back ever give up (A/B, tests) */
    FG_LO_STATIC_CHUNKS = 512,     /* decode kernels: deal the chunks of a batch out round-robin over the waves (rounds 3-4) instead of by
                                      ticket -- every wave draws its next chunk from a per-launch counter when it needs one (A/B, tests) */
    FG_LO_FRAME_SELFTEST_STALL = 1024, /* framing self-test: the one-pass scan's second tile never publishes its descriptor, so the tiles behind
                                      it must give up within the spin bound and the call must come back through the classic kernels with
                                      the same result (tests; never set in production: it costs the spin bound, ~0.2 s) */
    FG_LO_NO_TAPER = 2048,         /* ticket launches: every chunk of the batch the same size -- by default the last chunk per wave's worth of
                                      lines is dealt out in halves, quarters and eighths of a chunk, so that the grid finishes together
                                      (fg_plan_policy.hpp; A/B, tests) */
    FG_LO_TAPER_1 = 4096,          /* ... at most one such level (halves) instead of the format's own depth; */
    FG_LO_TAPER_2 = 8192,          /* ... at most two (halves, quarters); both bits: three (tuning) */
    FG_LO_NO_FUSED_FRAMING = 16384, /* fg_frame_decode_batch / fg_transcode_batch: the separate framing pass (rounds 1-5) even where the decode kernels
                                      can frame a pinned chunk themselves (A/B, tests) */
    FG_LO_RFC3164_REGROUP = 32768, /* FG_RFC3164: hand the lines of the slow shapes (zone names, the custom form) to a second kernel, 64 of a kind to the workgroup,
                                      for batches of any size -- the library does so from 1 M lines on (tests) */
    FG_LO_RFC3164_NO_REGROUP = 65536, /* ... never: lines in arrival order, a wave runs the union of its lines' shapes (rounds 1-5; A/B) */
    FG_LO_NO_SPARSE = 131072,      /* RFC5424: the whole-line window for short lines even where the library would leave the message bodies out of it */
    FG_LO_FORCE_SPARSE = 262144,   /* RFC5424: the sparse window -- only the chunks that hold a line's head or its last bytes are fetched -- for every
                                      batch that takes the whole-line kernel without the pair-parallel walk (parity sweeps, A/B) */
    FG_LO_RESERVED = 0x40000000    /* the library's own (fg_set_launch_opts clears it) */
};

/* Create a decoder context on HIP device `device` (replaces XDecoder::new(&Config),
 * flowgger/mod.rs:413-422).  cfg may be NULL (RFC5424 / GELF take no configuration).
 * Fails with FG_ERR_NO_DEVICE when no gfx950 GPU is usable -- there is no CPU fallback.
 * A ctx is cheap to clone per connection thread (decoder/mod.rs:23-36): fg_clone shares the
 * device-side configuration and gets its own stream + staging buffers. */
int fg_create(int device, const fg_cfg* cfg, fg_ctx** out);
int fg_clone(const fg_ctx* ctx, fg_ctx** out);
void fg_destroy(fg_ctx* ctx);
int fg_last_hip_error(const fg_ctx* ctx);
int fg_set_launch_opts(fg_ctx* ctx, const fg_launch_opts* opts);
/* Configure the RFC3164 decoder of this ctx (copied; clones made afterwards inherit it).  Required before the first
 * FG_RFC3164 decode (FG_ERR_ARG otherwise). */
int fg_set_rfc3164(fg_ctx* ctx, const fg_rfc3164_cfg* cfg);

/* Bytes of device scratch fg_decode_batch_device needs in `tables` are all caller-provided;
 * this helper returns the byte size of every array of an fg_tables for (n, ent_cap) so that a
 * caller can carve one allocation: sizes[k] for k = meta, ts, hostname, appname, procid, msgid,
 * msg, full_msg, ent_first, ent_count, ent_name, ent_val, ent_type, ent_flags, ent_used. */
#define FG_TABLE_ARRAYS 15
int fg_tables_layout(uint64_t n, uint64_t ent_cap, uint64_t sizes[FG_TABLE_ARRAYS]);

/* DEVICE-RESIDENT decode (the hot path): every pointer is a device pointer on ctx's device.
 *   d_bytes    packed lines; must be 16-byte aligned and readable up to nbytes rounded up to 16
 *   d_offsets  n+1 entries, offsets[0] >= 0, offsets[n] <= nbytes, non-decreasing
 *   tables     struct (host memory) of DEVICE array pointers, n rows, ent_cap entries
 *   stream     a hipStream_t passed through verbatim (NULL = HIP's default/null stream, which is
 *              what PyTorch's default current stream is), or FG_STREAM_OWN = the ctx's own
 *              non-blocking stream; the call is asynchronous on it.
 * replaces: `for line { decoder.decode(line) }` (line_splitter.rs:17,50). */
int fg_decode_batch_device(fg_ctx* ctx, fg_format fmt, const uint8_t* d_bytes, uint64_t nbytes,
                           const uint64_t* d_offsets, uint64_t n, const fg_tables* tables,
                           void* stream);

/* GPU FRAMING + UTF-8 VALIDATION of a raw byte stream (replaces `buf_reader.lines()` /
 * `buf_reader.split(0)` + `str::from_utf8`, splitter/line_splitter.rs:17-25, nul_splitter.rs:18-40):
 *   d_bytes     raw stream chunk (device), 16-byte aligned, readable up to nbytes rounded up to 16
 *   d_offsets   out, cap_frames + 2 entries: frame i = [offsets[i], offsets[i+1]) INCLUDING its
 *               terminator; a final unterminated piece is a frame if it is non-empty
 *   d_bad_utf8  out, cap_frames + 1 bytes: 1 = the frame is not valid UTF-8
 *   n_frames    out (host): number of frames; the call synchronises the stream to read it
 * Returns FG_ERR_ENT_OVERFLOW when cap_frames is too small (*n_frames then holds the need).
 * framing must be FG_FRAME_LINE or FG_FRAME_NUL (FG_ERR_UNSUPPORTED otherwise: FG_FRAME_SYSLEN has its own entry point,
 * fg_frame_syslen_device, because its frames carry a prefix and come out packed). */
int fg_frame_device(fg_ctx* ctx, fg_framing framing, const uint8_t* d_bytes, uint64_t nbytes,
                    uint64_t* d_offsets, uint8_t* d_bad_utf8, uint64_t cap_frames, uint64_t* n_frames,
                    void* stream);

/* GPU FRAMING OF THE CHUNKS OF MANY CONNECTIONS IN ONE LAUNCH (additive under the same FG_ABI_VERSION).  The reference gives every
 * connection its own splitter (input/tcp/tcp_input.rs:39-47) whose `buf_reader.lines()` / `buf_reader.split(0)` frames that
 * connection's stream alone (splitter/line_splitter.rs:17-54, nul_splitter.rs:18-60); this call replaces that for K connections at once.
 *   d_bytes        the chunks back to back (device), 16-byte aligned, readable up to nbytes rounded up to 16
 *   d_seg_starts   n_segs + 1 entries (device): segment k = bytes[seg_starts[k] .. seg_starts[k + 1]).  The segments tile the
 *                  buffer: seg_starts[0] == 0, seg_starts[n_segs] == nbytes, non-decreasing; empty segments are allowed and a start
 *                  needs NO alignment.  A list that does not tile is clamped (each value into [its predecessor, nbytes], the first
 *                  to 0, the last to nbytes): the results are then those of the clamped list, and memory safety never depends on it.
 *   d_seg_final    n_segs bytes (device) or NULL = all zero: nonzero = connection k ended with this chunk
 *   framing        FG_FRAME_LINE or FG_FRAME_NUL (FG_ERR_ARG otherwise: FG_FRAME_SYSLEN has fg_frame_syslen_multi_device, FG_FRAME_CAPNP
 *                  fg_frame_capnp_multi_device)
 * Every segment is framed as if it were the whole stream.  The output is a list of SLOTS that tile the buffer, in buffer order:
 *   d_offsets      out, cap_slots + 1 entries: slot i = [offsets[i], offsets[i + 1]), terminator included.  A nonempty segment has
 *                  one slot per delimiter in it and one more when its last byte is no delimiter (its tail); an empty one has none
 *   d_kind         out, cap_slots bytes, an fg_slot_kind per slot:
 *                  FG_SLOT_FRAME     a frame, valid UTF-8
 *                  FG_SLOT_BAD_UTF8  a frame whose bytes are not valid UTF-8 BY THEMSELVES (str::from_utf8 of exactly those bytes):
 *                                    a neighbouring segment's bytes never make a slot valid or invalid; a sequence cut off by the end
 *                                    of a final segment is invalid in its tail; a continuation byte that opens a segment is stray
 *                  FG_SLOT_CARRY     the unterminated tail of a segment that is NOT final: no frame, no UTF-8 verdict -- the caller
 *                                    carries those bytes over to the connection's next chunk.  (A final segment's tail is a frame.)
 *                  d_kind is what fg_decode_frames_device takes as d_bad_utf8, unchanged: nonzero = not decoded, FG_ST_BAD_UTF8 --
 *                  a CARRY slot costs one skipped row, at most one per segment
 *   d_seg_first    out, n_segs + 1 entries: the slots of segment k are [seg_first[k], seg_first[k + 1]); seg_first[n_segs] = *n_slots
 *   d_seg_consumed out, n_segs entries: the bytes of segment k that its frames cover (its length less its CARRY tail)
 *   n_slots        out (host); the call synchronises the stream to read it
 * With n_segs == 1 and seg_final[0] != 0 the slots, offsets and flags are those of fg_frame_device on the same bytes.
 * Returns FG_ERR_ENT_OVERFLOW when cap_slots is too small (*n_slots holds the need; nothing beyond the capacity is written and the
 * per-segment outputs are not).  Honours FG_LO_FRAME_CLASSIC. */
typedef enum fg_slot_kind {
    FG_SLOT_FRAME = 0,
    FG_SLOT_BAD_UTF8 = 1,
    FG_SLOT_CARRY = 2,
    FG_SLOT_UNREACHED = 3 /* fg_transcode_multi_batch, FG_FRAME_SYSLEN only: a frame behind its segment's first FG_SLOT_BAD_UTF8 frame, which the
                             reference's connection thread never reads (additive under the same FG_ABI_VERSION) */
} fg_slot_kind;
int fg_frame_multi_device(fg_ctx* ctx, fg_framing framing, const uint8_t* d_bytes, uint64_t nbytes,
                          const uint64_t* d_seg_starts, const uint8_t* d_seg_final, uint64_t n_segs,
                          uint64_t* d_offsets, uint8_t* d_kind, uint64_t cap_slots,
                          uint64_t* d_seg_first, uint64_t* d_seg_consumed, uint64_t* n_slots, void* stream);

/* Decode frames as produced by fg_frame_device: the kernels strip the terminators themselves, and
 * frames flagged in d_bad_utf8 (may be NULL) get status FG_ST_BAD_UTF8 instead of a decode.
 * fg_decode_batch_device(...) == fg_decode_frames_device(..., FG_FRAME_NONE, ..., NULL, ...).
 * FG_FRAME_SYSLEN is rejected (FG_ERR_ARG): decode what fg_frame_syslen_device packed with FG_FRAME_NONE. */
int fg_decode_frames_device(fg_ctx* ctx, fg_format fmt, fg_framing framing, const uint8_t* d_bytes,
                            uint64_t nbytes, const uint64_t* d_offsets, uint64_t n,
                            const uint8_t* d_bad_utf8, const fg_tables* tables, void* stream);

/* FRAME + DECODE IN ONE KERNEL (round 6; ABI 4): the decode kernel frames the raw stream chunk itself -- one read of the stream, no
 * framing pass, no frame count that visits the host between two kernels.  Replaces, for a chunk of the stream, the whole loop of
 * LineSplitter::run / NulSplitter::run (splitter/line_splitter.rs:17-54, nul_splitter.rs:18-60): `lines()` / `split(0)`, the UTF-8
 * check and decoder.decode(line) for every frame.
 *   d_bytes      raw stream chunk (device-addressable: HBM, or the device view of pinned host memory), 16-byte aligned, readable
 *                up to nbytes rounded up to 16
 *   final        nonzero: the stream ends with this chunk (an unterminated last piece is a frame); zero: it is not a frame, and
 *                d_offsets[frames] says where it starts (carry it over)
 *   d_offsets    out, cap_frames + 2 entries: frame i = [d_offsets[i], d_offsets[i + 1]) INCLUDING its terminator
 *   tables       device arrays for cap_frames rows (tables->n >= cap_frames); a frame that is not valid UTF-8 gets FG_ST_BAD_UTF8
 *   avg_line_hint  the average frame length to plan the launch for (0 = what this ctx last saw); only the speed depends on it
 *   d_result     out (device), two words: [0] the frames of the chunk -- when it exceeds cap_frames the rows beyond were not
 *                written: run again with more; [1] nonzero: the kernel's look-back gave up (never seen; bounded spin) -- nothing is
 *                valid, use fg_frame_device + fg_decode_frames_device
 * Asynchronous on `stream`.  FG_ERR_UNSUPPORTED (nothing launched): FG_RFC3164, or lines so long (average >= 768 bytes) that the
 * decoders stage heads only -- those keep the separate framing pass.  FG_FRAME_SYSLEN is rejected (FG_ERR_ARG): see
 * fg_frame_syslen_device. */

/* GPU FRAMING of an OCTET-COUNTED stream (input.framing = "syslen"; replaces read_msglen + read_exact + String::from_utf8 of
 * SyslenSplitter::run, splitter/syslen_splitter.rs:17-57, for a chunk of the stream that lies in device-addressable memory).
 * At a frame start the prefix is the bytes up to and including the first ' '; the text before it is usize::from_str (an optional
 * '+', at least one ASCII digit, leading zeros allowed, nothing else, the value fits 64 bits); the payload is the next len bytes,
 * untrimmed; the next frame starts right behind it; len == 0 is an empty message.  The frames are written FRAMED AND PACKED:
 *   d_bytes         raw stream chunk (device-addressable), 16-byte aligned, readable up to nbytes rounded up to 16
 *   final           nonzero: the stream ends with this chunk.  (The frames found are the same either way -- a frame needs its whole
 *                   payload; what differs is what the caller does with a TAIL.)
 *   d_packed        out: the payloads back to back, capacity nbytes rounded up to 16, plus 16
 *   d_offsets       out, cap_frames + 1 entries INTO d_packed, the FG_FRAME_NONE convention: everything downstream
 *                   (fg_decode_frames_device(..., FG_FRAME_NONE, ...), fg_encode_device*, the mergers) takes the two unchanged
 *   d_frame_starts  out, cap_frames + 1 entries INTO d_bytes, prefix included: the frames tile [0, consumed)
 *   d_bad_utf8      out, cap_frames bytes: 1 = the payload is not valid UTF-8 (rows decoded with it get FG_ST_BAD_UTF8).  The
 *                   reference unwrap()-panics at the FIRST such payload (syslen_splitter.rs:32): every such frame is flagged here,
 *                   stopping at the first one is the CALLER's job
 *   n_frames, consumed, stop_reason   out (host): frames, the bytes they cover, an fg_syslen_stop; the call synchronises the stream
 * Returns FG_ERR_ENT_OVERFLOW when cap_frames is too small (*n_frames holds the need; nbytes / 2 always suffices), and
 * FG_ERR_UNSUPPORTED when the device path DECLINES the chunk -- payload text that looks like prefixes sent more speculative chains
 * across a tile boundary than the kernels track: nothing is valid, frame the chunk on the host (the host-buffer entry points do).
 * The chain is resolved exactly: a result that is returned is the sequential walk's. */
int fg_frame_syslen_device(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, int final, uint8_t* d_packed, uint64_t* d_offsets,
                           uint64_t* d_frame_starts, uint8_t* d_bad_utf8, uint64_t cap_frames, uint64_t* n_frames, uint64_t* consumed,
                           int* stop_reason, void* stream);
/* GPU FRAMING OF THE OCTET-COUNTED CHUNKS OF MANY CONNECTIONS IN ONE LAUNCH (additive under the same FG_ABI_VERSION).  The reference
 * gives every connection a SyslenSplitter of its own (input/tcp/tcp_input.rs:39-47, tcpco_input.rs, tlsco_input.rs,
 * splitter/syslen_splitter.rs:10-57); this call replaces read_msglen + read_exact + String::from_utf8 for K connections at once.
 *   d_bytes, d_seg_starts, n_segs   as fg_frame_multi_device: the segments tile the buffer, a start needs no alignment, empty segments
 *                   are allowed, and the list is clamped on the device (memory safety never depends on it).  There is no seg_final: a
 *                   frame needs its whole payload whether or not the connection ended, and what a tail means at the end of a stream
 *                   is the caller's business, as for fg_frame_syslen_device
 * Every segment is walked as if it were the whole chunk.  A neighbouring segment's bytes never complete a prefix or a payload: a prefix
 * that meets its segment's end without a ' ' is a TAIL, so is a payload that would run past it (whatever the buffer holds there), and
 * a segment that begins with ' ' or a non-digit is a BAD_LEN whatever digits the segment before ended on.  A UTF-8 sequence cut off by
 * the end of a payload is invalid in that payload, whatever byte follows.  The frames come out in buffer order, FRAMED AND PACKED as
 * fg_frame_syslen_device writes them:
 *   d_packed        out: the payloads back to back, capacity nbytes rounded up to 16, plus 16; 16-byte aligned
 *   d_offsets       out, cap_frames + 1 entries INTO d_packed, the FG_FRAME_NONE convention
 *   d_frame_starts  out, cap_frames entries INTO d_bytes: where the prefix of frame i starts.  The frames no longer tile the buffer:
 *                   frame i ends at start + FG_SYSLEN_PREFIX_LEN + (offsets[i + 1] - offsets[i])
 *   d_bad_utf8      out, cap_frames bytes, as fg_frame_syslen_device
 *   d_seg_first     out, n_segs + 1 entries: the frames of segment k are [seg_first[k], seg_first[k + 1]); seg_first[n_segs] = *n_frames
 *   d_seg_consumed  out, n_segs entries: the bytes of segment k that its frames cover
 *   d_seg_stop      out, n_segs bytes: an fg_syslen_stop -- how the chain of segment k ended at seg_starts[k] + seg_consumed[k].  A stop
 *                   in one segment changes nothing in any other; an empty segment is CLEAN with no frames
 *   n_frames, payload_bytes   out (host): the frames and the bytes packed; the call synchronises the stream
 * With n_segs == 1 the frames, offsets, starts, flags, consumed and stop are those of fg_frame_syslen_device on the same bytes.
 * Returns FG_ERR_ENT_OVERFLOW when cap_frames is too small (*n_frames holds the need; NOTHING is written to the frame outputs and the
 * per-segment outputs), FG_ERR_UNSUPPORTED when the launch DECLINES (as fg_frame_syslen_device: nothing is valid, frame on the host;
 * segment starts inside one tile never cause it -- they do not go through the tiles' inboxes) or nbytes exceeds the single-stream
 * framer's bound or n_segs 2^24. */
int fg_frame_syslen_multi_device(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_seg_starts, uint64_t n_segs,
                                 uint8_t* d_packed, uint64_t* d_offsets, uint64_t* d_frame_starts, uint8_t* d_bad_utf8, uint64_t cap_frames,
                                 uint64_t* d_seg_first, uint64_t* d_seg_consumed, uint8_t* d_seg_stop, uint64_t* n_frames,
                                 uint64_t* payload_bytes, void* stream);
/* GPU FRAMING of a CAP'N PROTO stream (input.format = "capnp"; replaces the walk of capnp::serialize::read_message over the segment
 * tables in CapnpSplitter::run, splitter/capnp_splitter.rs:24-46, for a chunk of the stream that lies in device-addressable memory
 * and starts at a message).  At a message start p: fewer than 8 bytes left is a TAIL; segs = u32le(p) + 1, 512 or more stops with
 * TOO_MANY_SEGMENTS; a table of roundup8(4 + 4 * segs) bytes that runs past the chunk is a TAIL; the 64-bit sum of the segs sizes
 * beyond 8 Mi words stops with TOO_LARGE; a body of 8 * sum bytes that runs past the chunk is a TAIL; else the next message starts
 * right behind the body (a message may be 8 bytes long).
 *   d_bytes      raw stream chunk (device-addressable), 16-byte aligned, readable up to nbytes rounded up to 16
 *   final        accepted for symmetry with the other framers: the messages found are the same either way (a message needs its
 *                whole body); what a TAIL means at the end of the stream is the caller's business
 *   d_offsets    out, cap_frames + 1 entries INTO d_bytes: message i = [off[i], off[i + 1]), its segment table included -- with
 *                d_bytes exactly what fg_decode_frames_device(FG_CAPNP, FG_FRAME_NONE, ...) takes.  Nothing is packed and no
 *                UTF-8 pass runs: Text is checked by the decoder
 *   n_frames, consumed, stop_reason   out (host): messages, the bytes they cover (= off[n]; for every stop but CLEAN the position
 *                of the table at which the walk stopped), an fg_capnp_stop; the call synchronises the stream
 * Returns FG_ERR_ENT_OVERFLOW when cap_frames is too small (*n_frames holds the need; nbytes / 8 always suffices),
 * FG_ERR_UNSUPPORTED when the launch DECLINES the chunk -- more words that other words' speculative messages end on than the
 * node store holds (one per 6 words): nothing is valid, walk the chunk on the host (the host-buffer entry points do) --, and
 * FG_ERR_ARG for a chunk of more than FG_CAPNP_FRAME_MAX_BYTES bytes (the scratch keeps word indices in 29 bits).
 * The chain is resolved exactly: a result that is returned is the sequential walk's, bit for bit. */
#define FG_CAPNP_FRAME_MAX_BYTES 0xFFFF0000ull
int fg_frame_capnp_device(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, int final, uint64_t* d_offsets, uint64_t cap_frames,
                          uint64_t* n_frames, uint64_t* consumed, int* stop_reason, void* stream);
/* GPU FRAMING OF THE CAP'N PROTO CHUNKS OF MANY CONNECTIONS IN ONE LAUNCH (additive under the same FG_ABI_VERSION).  The reference gives
 * every connection a CapnpSplitter of its own (input/tcp/tcp_input.rs:39-47, splitter/capnp_splitter.rs:24-46); this call replaces the
 * walk over the segment tables for K connections at once.  Every segment is walked as if it were the whole chunk: a table or a body
 * that would cross its segment's end is a TAIL whatever bytes the buffer holds there, and a stop in one segment changes nothing in
 * any other.
 *   d_bytes         as fg_frame_capnp_device
 *   d_seg_starts    n_segs + 1 entries (device), as fg_frame_multi_device, with ONE more rule: every start seg_starts[k], k < n_segs, is
 *                   a multiple of 8 (the framer works on 8-byte words counted from the buffer's start).  nbytes need not be, so only
 *                   the last segment may end off a word.  The rule loses nothing: a message is whole words, so the last len % 8 bytes
 *                   of a connection's pending bytes never complete one -- keep them back.  The list is clamped on the device and each
 *                   start rounded DOWN to a word: memory safety never depends on it.  Empty segments are allowed
 *   d_offsets       out, cap_slots + 1 entries INTO d_bytes.  The slots TILE the buffer: slot i = [off[i], off[i + 1]), off[n_slots] = nbytes
 *   d_kind          out, cap_slots bytes: FG_SLOT_FRAME -- a whole message with its segment table -- or FG_SLOT_CARRY -- the bytes of a
 *                   segment behind seg_consumed: at most one per segment, none when the segment ended CLEAN, the tail of a TAIL,
 *                   TOO_MANY_SEGMENTS or TOO_LARGE stop alike.  FG_SLOT_BAD_UTF8 never occurs: Text is the decoder's business.  With
 *                   d_bytes and d_offsets it is exactly what fg_decode_frames_device(FG_CAPNP, FG_FRAME_NONE, ..., d_bad_utf8 = d_kind)
 *                   takes: the CARRY rows are skipped (status FG_ST_BAD_UTF8)
 *   d_seg_first     out, n_segs + 1 entries: the slots of segment k are [seg_first[k], seg_first[k + 1]); seg_first[n_segs] = *n_slots
 *   d_seg_consumed  out, n_segs entries: the bytes of segment k that its messages cover
 *   d_seg_stop      out, n_segs bytes: an fg_capnp_stop -- how the walk of segment k ended at seg_starts[k] + seg_consumed[k]; an empty
 *                   segment is CLEAN with no slots
 *   n_slots         out (host); the call synchronises the stream
 * With n_segs == 1 the FRAME offsets, seg_consumed[0] and seg_stop[0] are those of fg_frame_capnp_device on the same bytes.
 * Returns FG_ERR_ENT_OVERFLOW when cap_slots is too small (*n_slots holds the need; NOTHING is written to the slot outputs and the
 * per-segment outputs; nbytes / 8 + n_segs always suffices), FG_ERR_UNSUPPORTED when the launch DECLINES (as fg_frame_capnp_device,
 * with n_segs more nodes in the store: nothing is valid, walk the segments on the host), FG_ERR_ARG for more than
 * FG_CAPNP_FRAME_MAX_BYTES bytes or more than 2^24 segments. */
int fg_frame_capnp_multi_device(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_seg_starts, uint64_t n_segs,
                                uint64_t* d_offsets, uint8_t* d_kind, uint64_t cap_slots, uint64_t* d_seg_first, uint64_t* d_seg_consumed,
                                uint8_t* d_seg_stop, uint64_t* n_slots, void* stream);
int fg_frame_decode_device(fg_ctx* ctx, fg_format fmt, fg_framing framing, const uint8_t* d_bytes, uint64_t nbytes, int final,
                           uint64_t* d_offsets, uint64_t cap_frames, const fg_tables* tables, uint64_t avg_line_hint,
                           uint64_t* d_result, void* stream);

/* THE UDP INPUT'S BODY ON THE GPU (input.type = "udp"; replaces handle_record_maybe_compressed, src/flowgger/input/udp_input.rs:
 * 100-143, up to decoder.decode, for a batch of datagrams).  A datagram is a zlib stream when it has at least 8 bytes, byte 0 is 0x78
 * and byte 1 is 0x01, 0x9c or 0xda; a gzip member when it has at least 24 bytes and starts 1f 8b 08; a bare record otherwise.
 * Compressed payloads are inflated (RFC 1950 / 1951 / 1952 in full, with zlib's notion of what is malformed; the first gzip member
 * only; bytes behind the trailer ignored), every payload is checked as str::from_utf8 does, and the payloads come out PACKED, the
 * FG_FRAME_NONE convention everything downstream takes.
 *
 * DEPARTURE FROM THE REFERENCE: max_inflated.  The reference inflates without a limit (its Vec::with_capacity(65_527 * 5) is a
 * reservation); a GPU that others share needs one.  A compressed datagram that inflates to more than max_inflated bytes is
 * dropped with FG_UDP_TOO_LARGE and is the caller's to inflate on the host; nothing beyond max_inflated + 1 bytes of it is ever
 * produced.  0 = FG_UDP_DEFAULT_MAX_INFLATED (that same product).  Bare records are not subject to it.
 * The verdicts are zlib's with max_inflated + 1 bytes of room, in this order: a malformation met within that room is BAD_*, then more
 * than max_inflated bytes is TOO_LARGE, then a stream that did not end is BAD_*.  One consequence: a stream that ENDS at exactly
 * max_inflated + 1 bytes is inflated once, because zlib had the room to reach its trailer -- a wrong checksum makes it BAD_*, a right
 * one leaves it TOO_LARGE, and either way the dropped row occupies max_inflated + 1 bytes of d_out and of *total. */
typedef enum fg_udp_status {
    FG_UDP_RAW = 0,       /* kept: a bare record */
    FG_UDP_ZLIB = 1,      /* kept: inflated from a zlib stream */
    FG_UDP_GZIP = 2,      /* kept: inflated from a gzip member */
    FG_UDP_BAD_ZLIB = 3,  /* dropped: "Corrupted compressed (zlib) record" */
    FG_UDP_BAD_GZIP = 4,  /* dropped: "Corrupted compressed (gzip) record" */
    FG_UDP_BAD_UTF8 = 5,  /* dropped: "Invalid UTF-8 input" (bare or inflated) */
    FG_UDP_TOO_LARGE = 6  /* dropped: inflates beyond max_inflated (this library's own; see above) */
} fg_udp_status;
#define FG_UDP_DEFAULT_MAX_INFLATED 327635u   /* 65_527 * 5 */
#define FG_UDP_MAX_MAX_INFLATED 0x7FFFFFF0u
/* What the reference prints for a dropped datagram (udp_input.rs:84-86 prints the error of :113 / :124 / :136): "" for the three
 * kept values, a text of this library's own for FG_UDP_TOO_LARGE, NULL for an unknown value. */
const char* fg_udp_error_string(uint8_t st);
/*   d_bytes, d_offsets   the datagrams back to back (device-addressable): datagram i = d_bytes[d_offsets[i] .. d_offsets[i + 1])
 *   max_inflated         see above; at most FG_UDP_MAX_MAX_INFLATED
 *   d_out                out: the payloads, 16-byte aligned and writable up to out_cap ROUNDED UP TO 16 (what fg_decode_frames_device
 *                        reads).  NULL = the sizing call, as for fg_encode_device: only *total and d_out_offsets are produced
 *   d_out_offsets        out, n + 1 entries into d_out: payload i = [off[i], off[i + 1]).  A datagram dropped for its STREAM
 *                        (FG_UDP_BAD_ZLIB / _BAD_GZIP / _TOO_LARGE) has an empty payload, with two exceptions that show only once
 *                        the bytes exist: a stream that is whole, trailer included, and whose checksum (or gzip ISIZE) alone
 *                        disagrees keeps the bytes it produced, flagged BAD_*; and the TOO_LARGE row of exactly max_inflated + 1
 *                        bytes described above keeps those.  FG_UDP_BAD_UTF8 keeps its bytes
 *   d_drop               out, n bytes: nonzero = not to be decoded.  Goes straight into the d_bad_utf8 argument of
 *                        fg_decode_frames_device(..., FG_FRAME_NONE, ...): those rows come back with FG_ST_BAD_UTF8
 *   d_udp_status         out, n bytes: an fg_udp_status each, the real reason
 *   total                out (host): the bytes the payloads take.  The call synchronises the stream to read it.  With d_out given and
 *                        *total > out_cap nothing is written: FG_ERR_ENT_OVERFLOW, the need in *total
 * One lane walks one datagram, so a batch wants thousands of them; a single large stream is not what this is for. */
int fg_udp_unpack_device(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_offsets, uint64_t n,
                         uint64_t max_inflated, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_offsets,
                         uint8_t* d_drop, uint8_t* d_udp_status, uint64_t* total, void* stream);
/* THE SAME IN ONE WALK PER STREAM (additive under the same FG_ABI_VERSION).  fg_udp_unpack_device walks every compressed datagram
 * twice (count, then write) and a caller that has no size to give walks it a third time for the sizing call.  This form guesses:
 * every gated datagram of `len` bytes is inflated into a ctx-owned stage of min(max_inflated + 1, 4 * len + 64 rounded up to 16)
 * bytes by a walk that also counts, so its size, its verdict and its bytes exist after one pass; a stream that outgrows its stage
 * is only counted from there on ("spilled") and written by the write walk afterwards, into its slot.  Arguments and results are
 * those of fg_udp_unpack_device, byte for byte (d_out[0 .. *total), d_out_offsets, d_drop, d_udp_status, *total), except:
 *   d_out == NULL        FG_ERR_ARG: there is no sizing call -- give a buffer, and on FG_ERR_ENT_OVERFLOW one of *total bytes
 *   *total > out_cap     FG_ERR_ENT_OVERFLOW, the need in *total, nothing written to d_out (d_out_offsets, d_drop and d_udp_status
 *                        are as far as the front half takes them: checksums of spilled rows and UTF-8 are not settled)
 * The stream is synchronised ONCE, for *total; what is written behind that is queued on it and not waited for.
 * fg_udp_last_spilled: how many datagrams of the last one-walk unpack on this ctx (this entry or fg_udp_transcode_batch) spilled. */
int fg_udp_unpack_once_device(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_offsets, uint64_t n,
                              uint64_t max_inflated, uint8_t* d_out, uint64_t out_cap, uint64_t* d_out_offsets,
                              uint8_t* d_drop, uint8_t* d_udp_status, uint64_t* total, void* stream);
uint64_t fg_udp_last_spilled(const fg_ctx* ctx);

/* HOST-BUFFER decode: the batch is decoded into ctx-owned pinned host memory (`out` is filled with host pointers valid until
 * the next call on this ctx or fg_destroy).  Synchronous.  Entry-table capacity grows automatically.
 *   `bytes` AND `offsets` in PINNED memory (fg_alloc_pinned / hipHostRegister: where the batching framer accumulates lines),
 *   bytes 16-byte aligned: ZERO-COPY -- one launch, the kernels read the lines in place over the link and write the table columns
 *   straight into the pinned tables, both directions of the link busy at once.  The kernels load 16 bytes at a time: the pinned
 *   mapping must be READABLE UP TO nbytes ROUNDED UP TO 16 (fg_alloc_pinned memory is; a hipHostRegister'ed range must include
 *   those bytes), and bytes[0 .. that) and offsets[0 .. n] must each lie in ONE mapping -- buffers that do not qualify (the library
 *   checks the device view of the first and the last byte it will touch) silently take the sliced path below;
 *   anything else: the batch goes up as ~32 MiB slices on three streams (H2D, kernels, D2H of the tables), at the runtime's
 *   staged-copy speed for pageable memory. */
int fg_decode_batch(fg_ctx* ctx, fg_format fmt, const uint8_t* bytes, uint64_t nbytes,
                    const uint64_t* offsets, uint64_t n, fg_tables* out);

/* HOST-BUFFER RAW-STREAM decode: one call frames a chunk of the raw byte stream on the GPU
 * (FG_FRAME_LINE / FG_FRAME_NUL), validates UTF-8 per frame and decodes every frame -- what
 * LineSplitter::run / NulSplitter::run do per line (line_splitter.rs:17-54, nul_splitter.rs:18-60).
 *   final        nonzero: the stream ends with this chunk, so a trailing unterminated piece is a
 *                frame (BufRead semantics); zero: it is left for the next chunk
 *   out          tables in ctx-owned pinned host memory (as fg_decode_batch), *n_frames rows; a frame
 *                that is not valid UTF-8 has status FG_ST_BAD_UTF8
 *   out_offsets  ctx-owned host array, *n_frames + 1 entries: frame i = bytes[off[i] .. off[i+1])
 *                INCLUDING its terminator; spans in `out` are relative to off[i]
 *   consumed     bytes covered by the returned frames: carry bytes[consumed .. nbytes) over
 * FG_FRAME_SYSLEN (the whole loop of SyslenSplitter::run, syslen_splitter.rs:42-57, for a chunk): out_offsets are the frame starts
 * in `bytes`, "<len> " prefix included; the spans in `out` are relative to each frame's PAYLOAD start, off[i] +
 * FG_SYSLEN_PREFIX_LEN(bytes + off[i], off[i + 1] - off[i]); fg_last_syslen_stop says how the chain ended.  Every payload that is not
 * valid UTF-8 is flagged FG_ST_BAD_UTF8; the reference panics at the first one, and stopping there is the caller's job.  A chunk the
 * device framer declines is framed by a host hop over `bytes` instead, with the same results (fg_last_host_path tells).
 * FG_FRAME_CAPNP (FG_CAPNP only; the read_message loop of CapnpSplitter::run, capnp_splitter.rs:24-46, for a chunk): the chunk is
 * uploaded once, framed in HBM and decoded from the same buffer; out_offsets are the message starts in `bytes`, which the spans in
 * `out` are relative to; fg_last_capnp_stop says how the chain ended at `consumed`.  A chunk the device framer declines is walked
 * on the host over `bytes`, with the same results (fg_last_host_path tells).
 * Everything returned stays valid until the next call on this ctx. */
int fg_frame_decode_batch(fg_ctx* ctx, fg_format fmt, fg_framing framing, const uint8_t* bytes,
                          uint64_t nbytes, int final, fg_tables* out, const uint64_t** out_offsets,
                          uint64_t* n_frames, uint64_t* consumed);

/* HOST-BUFFER decode of the chunks of MANY connections: one call uploads the buffer, frames every segment as its own stream
 * (fg_frame_multi_device, whose contract this shares: segments, slots, kinds) and decodes every slot -- the stream-side sibling of
 * fg_udp_decode_batch.  fmt: FG_RFC5424, FG_LTSV, FG_GELF or FG_RFC3164 (FG_CAPNP: FG_ERR_ARG); framing: FG_FRAME_LINE or FG_FRAME_NUL
 * (FG_ERR_ARG otherwise).  Here the tiling of seg_starts IS checked (FG_ERR_ARG).  seg_final may be NULL (= all zero).
 *   out               tables in ctx-owned pinned host memory, *n_slots rows; FG_SLOT_BAD_UTF8 and FG_SLOT_CARRY rows have status
 *                     FG_ST_BAD_UTF8, (*out_kind)[i] tells them apart; spans are relative to (*out_offsets)[i]
 *   out_offsets       *n_slots + 1 entries;  out_kind: *n_slots bytes
 *   out_seg_first     n_segs + 1 entries;    out_seg_consumed: n_segs entries
 * Everything returned is ctx-owned and stays valid until the next call on this ctx.  fg_last_host_path says FG_PATH_FRAME_MULTI.
 * From which chunk size on a call per connection is as good has not been measured yet (tools/probe/multi_stream.py is the probe).
 * Out of scope here: slicing over streams, the zero-copy fused launch. */
int fg_frame_decode_multi_batch(fg_ctx* ctx, fg_format fmt, fg_framing framing, const uint8_t* bytes, uint64_t nbytes,
                                const uint64_t* seg_starts, const uint8_t* seg_final, uint64_t n_segs,
                                fg_tables* out, const uint64_t** out_offsets, const uint8_t** out_kind,
                                const uint64_t** out_seg_first, const uint64_t** out_seg_consumed, uint64_t* n_slots);

/* HOST-BUFFER decode of the OCTET-COUNTED chunks of many connections: one call uploads the buffer, frames and packs every segment as
 * its own stream (fg_frame_syslen_multi_device, whose contract this shares) and decodes the packed payloads (FG_FRAME_NONE, with the
 * UTF-8 flags).  fmt: FG_RFC5424, FG_LTSV, FG_GELF or FG_RFC3164 (FG_CAPNP: FG_ERR_ARG).  The tiling of seg_starts IS checked here
 * (FG_ERR_ARG).
 *   out               tables in ctx-owned pinned host memory, *n_frames rows; a payload that is not valid UTF-8 has status
 *                     FG_ST_BAD_UTF8; spans are relative to each frame's PAYLOAD start (as FG_FRAME_SYSLEN in fg_frame_decode_batch):
 *                     (*out_frame_starts)[i] + FG_SYSLEN_PREFIX_LEN
 *   out_frame_starts  *n_frames entries into `bytes`
 *   out_seg_first     n_segs + 1 entries;  out_seg_consumed: n_segs entries;  out_seg_stop: n_segs bytes (fg_syslen_stop)
 * When the device framer declines, or any segment stops with FG_SYSLEN_LONG_PREFIX, the whole buffer is hopped on the host, segment by
 * segment, with prefixes of any length: the same results (and no LONG_PREFIX).  fg_last_host_path says
 * FG_PATH_FRAME_SYSLEN_MULTI_DEVICE or FG_PATH_FRAME_SYSLEN_MULTI_HOST.  Everything returned is ctx-owned and stays valid until the
 * next call on this ctx.  Out of scope here: slicing over streams, the fused launch. */
int fg_frame_decode_syslen_multi_batch(fg_ctx* ctx, fg_format fmt, const uint8_t* bytes, uint64_t nbytes, const uint64_t* seg_starts,
                                       uint64_t n_segs, fg_tables* out, const uint64_t** out_frame_starts, const uint64_t** out_seg_first,
                                       const uint64_t** out_seg_consumed, const uint8_t** out_seg_stop, uint64_t* n_frames);

/* HOST-BUFFER decode of the CAP'N PROTO chunks of many connections: one call uploads the buffer, frames every segment as its own stream
 * (fg_frame_capnp_multi_device, whose contract this shares) and decodes the messages where they lie (FG_CAPNP, FG_FRAME_NONE, with
 * the slot kinds as the skip array).  The list IS checked here: FG_ERR_ARG when seg_starts does not tile the buffer or a start
 * seg_starts[k], k < n_segs, is not a multiple of 8.
 *   out               tables in ctx-owned pinned host memory, *n_slots rows; a FG_SLOT_CARRY row has status FG_ST_BAD_UTF8 and no entries;
 *                     spans are relative to each slot's start (*out_offsets)[i], the segment table included
 *   out_offsets       *n_slots + 1 entries into `bytes`;  out_kind: *n_slots bytes
 *   out_seg_first     n_segs + 1 entries;  out_seg_consumed: n_segs entries;  out_seg_stop: n_segs bytes (fg_capnp_stop)
 * When the device framer declines, every segment is walked on the host: the same results.  fg_last_host_path says
 * FG_PATH_FRAME_CAPNP_MULTI_DEVICE or FG_PATH_FRAME_CAPNP_MULTI_HOST.  Everything returned is ctx-owned and stays valid until the next
 * call on this ctx.  Out of scope here: slicing over streams. */
int fg_frame_decode_capnp_multi_batch(fg_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, const uint64_t* seg_starts, uint64_t n_segs,
                                      fg_tables* out, const uint64_t** out_offsets, const uint8_t** out_kind, const uint64_t** out_seg_first,
                                      const uint64_t** out_seg_consumed, const uint8_t** out_seg_stop, uint64_t* n_slots);

/* HOST-BUFFER UDP decode: upload the datagrams, fg_udp_unpack_device, decode -- the whole of handle_record_maybe_compressed for a
 * batch.  `bytes` / `offsets` pinned or pageable.  `out`: tables in ctx-owned pinned host memory, n rows; a dropped datagram has
 * status FG_ST_BAD_UTF8 and (*udp_status)[i] says why.  *out_lines / *out_line_offsets (n + 1 entries): the payloads as decoded, in
 * ctx-owned pinned memory -- the spans in `out` are relative to line i = (*out_lines)[off[i] .. off[i + 1]), NOT to the datagram, so
 * a caller needs them to materialise Records.  FG_CAPNP is rejected (FG_ERR_ARG): the reference has no Decoder for it.  Everything
 * returned stays valid until the next call on this ctx.  fg_last_host_path is not touched. */
int fg_udp_decode_batch(fg_ctx* ctx, fg_format fmt, const uint8_t* bytes, uint64_t nbytes, const uint64_t* offsets, uint64_t n,
                        uint64_t max_inflated, fg_tables* out, const uint8_t** out_lines, const uint64_t** out_line_offsets,
                        const uint8_t** udp_status);

/* Which form the last fg_decode_batch / fg_frame_decode_batch call on this ctx took (0 = none yet): the library picks by what the
 * caller's buffers allow, silently -- a harness that prices a leg against the link, or a test of one form, asks afterwards. */
enum {
    FG_PATH_DECODE_ZERO_COPY = 1,  /* fg_decode_batch: one launch, lines read over the link, tables written into pinned memory */
    FG_PATH_DECODE_SLICED = 2,     /* fg_decode_batch: hipMemcpy slices on three streams */
    FG_PATH_FRAME_FUSED = 3,       /* fg_frame_decode_batch: ONE launch -- the decode kernel frames the pinned chunk itself (round 6) */
    FG_PATH_FRAME_SLICED = 4,      /* fg_frame_decode_batch: upload slices + framing scan + decode per slice (rounds 3-5) */
    FG_PATH_FRAME_ONE_PIECE = 5,   /* fg_frame_decode_batch: upload, frame, count on the host, decode */
    FG_PATH_FRAME_SYSLEN_DEVICE = 6, /* fg_frame_decode_batch / fg_transcode_batch, FG_FRAME_SYSLEN: framed + packed by the device */
    FG_PATH_FRAME_SYSLEN_HOST = 7, /* ... the device framer declined the chunk: the prefixes were hopped on the host */
    FG_PATH_FRAME_CAPNP_DEVICE = 8, /* fg_frame_decode_batch / fg_transcode_batch, FG_FRAME_CAPNP: framed by the device where the chunk lies */
    FG_PATH_FRAME_CAPNP_HOST = 9,  /* ... the device framer declined the chunk: the segment tables were walked on the host */
    FG_PATH_FRAME_MULTI = 10,      /* fg_frame_decode_multi_batch: upload, segmented framing, decode */
    FG_PATH_FRAME_SYSLEN_MULTI_DEVICE = 11, /* fg_frame_decode_syslen_multi_batch: every segment framed + packed by the device */
    FG_PATH_FRAME_SYSLEN_MULTI_HOST = 12,   /* ... the device framer declined the buffer: the segments were hopped on the host */
    FG_PATH_FRAME_CAPNP_MULTI_DEVICE = 13,  /* fg_frame_decode_capnp_multi_batch: every segment framed by the device */
    FG_PATH_FRAME_CAPNP_MULTI_HOST = 14     /* ... the device framer declined the buffer: the segments were walked on the host */
};
int fg_last_host_path(const fg_ctx* ctx);
/* How the chain of segment tables of the last FG_FRAME_CAPNP call of fg_frame_decode_batch / fg_transcode_batch on this ctx ended (an
 * fg_capnp_stop; FG_CAPNP_CLEAN before the first such call). */
int fg_last_capnp_stop(const fg_ctx* ctx);
/* How the prefix chain of the last FG_FRAME_SYSLEN call of fg_frame_decode_batch / fg_transcode_batch on this ctx ended (an
 * fg_syslen_stop; FG_SYSLEN_CLEAN before the first such call). */
int fg_last_syslen_stop(const fg_ctx* ctx);

/* GELF ENCODER FROM THE TABLES: replaces GelfEncoder::encode (src/flowgger/encoder/
 * gelf_encoder.rs:59-115, serde_json 0.8 serialisation of the BTreeMap it builds) for a whole
 * decoded batch, without materialising Records: the JSON text of line i is written to
 * d_out[out_offsets[i] .. out_offsets[i+1]); a line whose decode failed (status != 0) produces
 * nothing.  `extra` = the output.gelf_extra table (may be NULL); the LTSV suffixes come from ctx.
 *   d_out_offsets  out, n + 1 entries (device)
 *   total          out (host): bytes needed; the call synchronises the stream to read it
 *   d_out == NULL  sizing call (only d_out_offsets / *total are produced);
 *   *total > out_cap -> FG_ERR_ENT_OVERFLOW, nothing written.
 * src_fmt says which decoder produced `tables`.  Same as fg_encode_device with FG_ENC_GELF / FG_MERGE_NONE. */
typedef struct fg_gelf_extra {
    uint32_t n;
    const char* const* keys;
    const char* const* values;
} fg_gelf_extra;
int fg_encode_gelf_device(fg_ctx* ctx, fg_format src_fmt, const uint8_t* d_bytes, uint64_t nbytes,
                          const uint64_t* d_offsets, uint64_t n, const fg_tables* tables,
                          const fg_gelf_extra* extra, uint8_t* d_out, uint64_t out_cap,
                          uint64_t* d_out_offsets, uint64_t* total, void* stream);

/* ANY ENCODER + MERGER FROM THE TABLES: replaces, for a whole decoded batch,
 *   Encoder::encode   encoder/{gelf,ltsv,rfc5424,rfc3164,passthrough}_encoder.rs   (trait: encoder/mod.rs:54-56)
 *   Merger::frame     merger/{line,nul,syslen}_merger.rs                             (trait: merger/mod.rs:30-32)
 * i.e. the `encoder.encode(decoded)?` of handle_line (splitter/line_splitter.rs:44-54) and the framing the outputs
 * apply to every message.  The encoded + framed bytes of line i are written to d_out[out_offsets[i] ..
 * out_offsets[i+1]); a line whose decode failed or whose encode returns Err produces nothing (the reference prints
 * the error and drops the line).  Records from all three decoders are accepted (GELF-sourced spans are JSON-unescaped
 * on the fly).  FG_ENC_CAPNP (encoder/capnp_encoder.rs) writes one Cap'n Proto message per line, byte for byte what
 * capnp::serialize::write_message writes for the Record the reference builds (schema record.capnp: segment table,
 * root struct, texts in allocation order; records beyond the first segment's 1024 words span several segments).
 * FG_ENC_CAPNP is an additive value under the same FG_ABI_VERSION: a library without it rejects it with FG_ERR_ARG.
 *   cfg->extra_*    output.gelf_extra (GELF) / output.ltsv_extra (LTSV) / output.capnp_extra (capnp) in the
 *                   configuration table's iteration order (a BTreeMap: sorted by key)
 *   cfg->prepend    RFC3164 / passthrough: the already formatted output.syslog_prepend_timestamp header (the
 *                   reference formats the wall clock per message, encoder/mod.rs:81-93); NULL = not configured;
 *                   ignored by the other encoders
 *   cfg->now_ts     Record.ts of GELF records decoded without "timestamp" (rows flagged FG_F_TS_NOW; the reference
 *                   reads the wall clock at decode time, gelf_decoder.rs:109)
 *   d_out_offsets   out, n + 1 entries (device)
 *   d_enc_status    out, n bytes (device), may be NULL: 0 = encoded, 1 = the row's decode had failed,
 *                   else an encoder error (fg_encode_error_string)
 *   total           out (host): bytes needed; the call synchronises the stream to read it
 *   d_out == NULL   sizing call (only d_out_offsets / d_enc_status / *total are produced);
 *   *total > out_cap -> FG_ERR_ENT_OVERFLOW, nothing written. */
typedef enum fg_encoder { FG_ENC_GELF = 0, FG_ENC_LTSV = 1, FG_ENC_RFC5424 = 2, FG_ENC_RFC3164 = 3, FG_ENC_PASSTHROUGH = 4, FG_ENC_CAPNP = 5 } fg_encoder;
typedef enum fg_merger { FG_MERGE_NONE = 0, FG_MERGE_LINE = 1, FG_MERGE_NUL = 2, FG_MERGE_SYSLEN = 3 } fg_merger;
typedef struct fg_encode_cfg {
    fg_encoder encoder;
    fg_merger merger;
    uint32_t n_extra;
    const char* const* extra_keys;
    const char* const* extra_values;
    const char* prepend;
    double now_ts;
} fg_encode_cfg;
int fg_encode_device(fg_ctx* ctx, fg_format src_fmt, const fg_encode_cfg* cfg, const uint8_t* d_bytes, uint64_t nbytes,
                     const uint64_t* d_offsets, uint64_t n, const fg_tables* tables, uint8_t* d_out, uint64_t out_cap,
                     uint64_t* d_out_offsets, uint8_t* d_enc_status, uint64_t* total, void* stream);

/* The same WITHOUT a host synchronisation (a device-resident pipeline must not wait on the host for a byte count):
 * count, scan and write are queued on `stream` and the call returns.  Nothing comes back to the host:
 *   d_out_offsets[n]  (device) = the bytes the batch needs; when it exceeds out_cap the write kernel leaves d_out untouched --
 *                     the caller checks that word whenever it next synchronises (d_out_offsets / d_enc_status are always produced)
 *   ent_hint          an upper bound of the entries in `tables` (sizes the GELF encoder's key-ranking scratch instead of the
 *                     ent_used read-back): 0 = none (RFC5424 without structured data), ~0 = unknown
 * The first calls on a ctx may still synchronise while its scratch grows to the batch size (hipFree / hipMalloc).
 * replaces: the same `encoder.encode` + `merger.frame` as fg_encode_device (splitter/line_splitter.rs:44-54). */
int fg_encode_device_async(fg_ctx* ctx, fg_format src_fmt, const fg_encode_cfg* cfg, const uint8_t* d_bytes, uint64_t nbytes,
                           const uint64_t* d_offsets, uint64_t n, const fg_tables* tables, uint8_t* d_out, uint64_t out_cap,
                           uint64_t* d_out_offsets, uint8_t* d_enc_status, uint64_t ent_hint, void* stream);
/* The reference's exact &'static str of an encode status (0 / 1 -> "", unknown -> NULL). */
const char* fg_encode_error_string(uint8_t enc_status);

/* THE WHOLE handle_line OF A BATCH -- HOST BUFFERS IN, ENCODED STREAM OUT (BASELINE configs[0]: input -> decoder ->
 * encoder -> output).  Replaces, for every line of a batch, the body of handle_line (splitter/line_splitter.rs:44-54:
 * `decoder.decode(line)` -> `encoder.encode(decoded)` -> `tx.send(..)`) plus the Merger::frame the output applies
 * (merger/mod.rs:30-32), and -- when `framing` is FG_FRAME_LINE / FG_FRAME_NUL -- the splitter's own framing + UTF-8
 * check (line_splitter.rs:17-25, nul_splitter.rs:18-40).  Everything between the two PCIe copies stays in HBM: the
 * decode tables are never copied back; what returns is the encoded + framed byte stream in input order and one
 * verdict per line, i.e. what the output thread writes and what the splitter prints to stderr.
 *   framing == FG_FRAME_NONE: `bytes` / `offsets[n + 1]` are framed lines (as for fg_decode_batch); `final` is ignored.
 *   framing == FG_FRAME_LINE / _NUL: `bytes` is a raw stream chunk, `offsets` must be NULL and `n` is ignored; an
 *     unterminated tail is a frame only when `final` != 0, otherwise out->consumed < nbytes and the caller carries
 *     the rest over to the next call (as for fg_frame_decode_batch).
 *   framing == FG_FRAME_SYSLEN: the same for an octet-counted chunk; frame_offsets are the frame starts, prefix included
 *     (FG_SYSLEN_PREFIX_LEN), and fg_last_syslen_stop says how the chain ended.
 *   framing == FG_FRAME_CAPNP (FG_CAPNP only): the same for a Cap'n Proto stream chunk; frame_offsets are the message starts and
 *     fg_last_capnp_stop says how the chain ended.
 * Results (pinned host memory owned by ctx, valid until the next host-buffer call on it):
 *   out / out_bytes / out_offsets[n + 1]   message i = out[out_offsets[i] .. out_offsets[i + 1]) -- empty when the
 *                                          line was dropped
 *   meta[n]         the table's meta column: meta & 0xFF = decoder status (fg_error_string; FG_ST_BAD_UTF8)
 *   enc_status[n]   0 = encoded, 1 = the decode had failed, else an encoder error (fg_encode_error_string)
 *   frame_offsets   the frames found in the chunk (n + 1 entries; NULL for FG_FRAME_NONE), for the stderr message
 *   n, consumed     lines handled, input bytes they cover */
typedef struct fg_transcoded {
    const uint8_t* out;
    uint64_t out_bytes;
    const uint64_t* out_offsets;
    const uint32_t* meta;
    const uint8_t* enc_status;
    const uint64_t* frame_offsets;
    uint64_t n;
    uint64_t consumed;
} fg_transcoded;
int fg_transcode_batch(fg_ctx* ctx, fg_format fmt, fg_framing framing, const fg_encode_cfg* cfg, const uint8_t* bytes,
                       uint64_t nbytes, const uint64_t* offsets, uint64_t n, int final, fg_transcoded* out);

/* THE SAME FOR THE CHUNKS OF MANY CONNECTIONS IN ONE CALL (additive under the same FG_ABI_VERSION): what fg_frame_decode_multi_batch,
 * fg_frame_decode_syslen_multi_batch and fg_frame_decode_capnp_multi_batch frame and decode -- K connections feeding one output,
 * input/tcp/tcp_input.rs:39-47 -- is encoded and framed for the output too; the tables stay in HBM, and what returns is the stream the
 * reference's K connection threads would have sent for these bytes, in buffer order, with one verdict per slot.
 *   framing   FG_FRAME_LINE / FG_FRAME_NUL (fmt: a text format), FG_FRAME_SYSLEN (a text format), FG_FRAME_CAPNP (FG_CAPNP, and only
 *             it); FG_FRAME_NONE is FG_ERR_ARG (a packed batch has no segments: fg_transcode_batch)
 *   seg_final LINE / NUL only (may be NULL = all zero); must be NULL otherwise (FG_ERR_ARG)
 * Argument rules, the tiling check of seg_starts and the size limits are those of the matching fg_frame_decode_*multi_batch, and so is
 * the contract of segments, slots, kinds, seg_first, seg_consumed and seg_stop -- with one addition for FG_FRAME_SYSLEN: in every segment
 * the first frame whose payload is not valid UTF-8 keeps FG_SLOT_BAD_UTF8 (the unwrap() of syslen_splitter.rs:33 that ends the
 * connection's thread) and every later frame of that segment, valid or not, is FG_SLOT_UNREACHED; both are skipped rows (status
 * FG_ST_BAD_UTF8, nothing encoded).  Other segments are not affected.
 * Results (pinned host memory owned by ctx, valid until the next host-buffer call on it):
 *   out / out_bytes / out_offsets[n + 1]   message i = out[out_offsets[i] .. out_offsets[i + 1]), empty when slot i produced nothing
 *   meta[n], enc_status[n]                 as fg_transcoded
 *   slot_offsets   LINE / NUL / CAPNP: n + 1 slot bounds in `bytes`; SYSLEN: n frame starts, "<len> " prefix included
 *   slot_kind[n]   fg_slot_kind
 *   seg_first[n_segs + 1], seg_consumed[n_segs], seg_stop[n_segs] (fg_syslen_stop / fg_capnp_stop; NULL for LINE / NUL)
 * fg_last_host_path says which framing form ran (FG_PATH_FRAME_MULTI .. FG_PATH_FRAME_CAPNP_MULTI_HOST); fg_last_syslen_stop and
 * fg_last_capnp_stop are not touched.  Out of scope here: slicing over streams, the fused launch. */
typedef struct fg_transcoded_multi {
    const uint8_t* out;
    uint64_t out_bytes;
    const uint64_t* out_offsets;
    const uint32_t* meta;
    const uint8_t* enc_status;
    const uint64_t* slot_offsets;
    const uint8_t* slot_kind;
    const uint64_t* seg_first;
    const uint64_t* seg_consumed;
    const uint8_t* seg_stop;
    uint64_t n;
} fg_transcoded_multi;
int fg_transcode_multi_batch(fg_ctx* ctx, fg_format fmt, fg_framing framing, const fg_encode_cfg* cfg, const uint8_t* bytes,
                             uint64_t nbytes, const uint64_t* seg_starts, const uint8_t* seg_final, uint64_t n_segs,
                             fg_transcoded_multi* out);

/* THE SAME FOR A BATCH OF UDP DATAGRAMS (additive under the same FG_ABI_VERSION): the body of the UDP input's receive loop
 * (input/udp_input.rs:66-143: the gate, inflate, from_utf8, `decoder.decode`, `encoder.encode`, `tx.send`) plus the Merger::frame of
 * the output.  Upload, the one-walk unpack (fg_udp_unpack_once_device) into ctx-owned HBM, then decode + encode + frame as
 * fg_transcode_batch does for FG_FRAME_NONE: neither the inflated payloads nor the tables cross the link.
 *   bytes, offsets, n, max_inflated   as fg_udp_decode_batch, with its argument checks; fmt a text format (FG_CAPNP: FG_ERR_ARG)
 *   out          as fg_transcode_batch: frame_offsets = NULL, consumed = nbytes, n = n.  A dropped datagram is a skipped row:
 *                meta & 0xFF == FG_ST_BAD_UTF8, enc_status == 1, an empty message
 *   udp_status   out: n fg_udp_status bytes (pinned, ctx-owned) -- why a datagram was dropped (fg_udp_error_string)
 * What the reference writes to stderr for datagram i is the bare error, without the line: fg_udp_error_string(udp_status[i]) for a
 * drop, else fg_error_string(meta[i] & 0xFF) for a failed decode, else fg_encode_error_string(enc_status[i]) for a failed encode.
 * Everything returned stays valid until the next host-buffer call on this ctx.  fg_last_host_path is not touched; fg_udp_last_spilled
 * tells how many streams took the second walk. */
int fg_udp_transcode_batch(fg_ctx* ctx, fg_format fmt, const fg_encode_cfg* cfg, const uint8_t* bytes, uint64_t nbytes,
                           const uint64_t* offsets, uint64_t n, uint64_t max_inflated, fg_transcoded* out, const uint8_t** udp_status);

/* THE ENCODED STREAM DEFLATED ON THE GPU (additive under the same FG_ABI_VERSION): output.kafka_compression = "gzip" with
 * output.kafka_coalesce (output/kafka_output.rs:163-182: every group of N messages is compressed), so that compressed bytes cross the
 * link on the way out as they already may on the way in (fg_udp_unpack_device).
 * The compressor takes a resident byte buffer and cuts[n_members + 1], ascending byte bounds: member m = bytes[cuts[m] .. cuts[m + 1]).
 * Every non-empty member comes out as ONE complete gzip member (RFC 1952: the fixed header 1f 8b 08 00 00 00 00 00 00 ff, a raw deflate
 * stream, CRC-32, ISIZE) that inflates on its own; an empty member produces no byte.  Members lie back to back, z_offsets[n_members + 1]
 * their bounds.  Inside, a member is cut into independent blocks of fg_deflate_block_bytes() input bytes, each the cheaper of a
 * fixed-Huffman block (greedy LZ77, matches of 4 .. 258 bytes inside the block) and a stored block; the output is a pure function
 * of the input.  That is FG_DEFLATE_FIXED, the default.  With FG_DEFLATE_DYNAMIC (fg_set_deflate_mode) every block comes out as the cheapest
 * of a stored, a fixed-Huffman and a dynamic-Huffman block (BTYPE 10: canonical codes of at most 15 bits built per block from the same
 * parse, their lengths run-length coded): about a fifth fewer bytes on text for about twice the compressor's time; a block that does not
 * come out dynamic has the bytes FG_DEFLATE_FIXED gives it, and the output is a pure function of the input in either mode.
 *   fg_deflate_bound    bytes that always suffice for nbytes of input in n_members members
 *   fg_deflate_device   d_z == NULL: a sizing call (*total and d_z_offsets are set).  *total > z_cap: FG_ERR_ENT_OVERFLOW and d_z is
 *                       not written (the contract of fg_encode_device).  FG_ERR_ARG: cuts that do not ascend or go past nbytes, and a
 *                       member of 0x7FE00000 bytes or more (which covers 4 GiB and more: a member's compressed size goes through a
 *                       31-bit scan).  d_z_offsets: n_members + 1 entries.  Synchronises the stream.  FG_ERR_UNSUPPORTED: a build without the kernels. */
typedef enum fg_compression { FG_COMP_NONE = 0, FG_COMP_GZIP = 1 } fg_compression;
/* coalesce = C >= 1 (the reference's kafka_coalesce): member k = messages [k C, min((k + 1) C, n)) by index, dropped lines (empty messages)
 * included.  coalesce = 0: members of about member_bytes bytes cut at message boundaries -- message i starts a member iff i == 0 or
 * floor(out_offsets[i] / B) > floor(out_offsets[i - 1] / B), B = member_bytes (0: fg_deflate_block_bytes()); a message larger than B is a
 * member of its own. */
typedef struct fg_compress_cfg {
    int codec; /* an fg_compression */
    uint32_t coalesce;
    uint32_t member_bytes;
} fg_compress_cfg;
uint32_t fg_deflate_block_bytes(void);
uint64_t fg_deflate_bound(uint64_t nbytes, uint64_t n_members);
int fg_deflate_device(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_cuts, uint64_t n_members, uint8_t* d_z,
                      uint64_t z_cap, uint64_t* d_z_offsets, uint64_t* total, void* stream);
/* Compression of what fg_transcode_batch, fg_transcode_multi_batch and fg_udp_transcode_batch return (NULL or FG_COMP_NONE: off, the
 * default, and then nothing changes by a byte).  A cfg with FG_COMP_NONE is stored as it is given (NULL: {FG_COMP_NONE, 1, 0}): its
 * coalesce / member_bytes compress nothing, and the one thing that reads them is the message-set stage of FG_WIRE_KAFKA_V0
 * (fg_set_output_wire, below), which cuts its uncompressed sets by them; with FG_WIRE_RAW they have no effect.  With FG_COMP_GZIP those calls cut the encoded stream into members by cfg, compress it
 * behind the encoder and do NOT copy the plain stream over the link: their `out` is NULL, out_bytes is the uncompressed total, and
 * out_offsets, meta, enc_status and everything else are as without compression.  fg_last_compressed hands out what the last such call
 * left (pinned host memory owned by ctx, valid until the next host-buffer call on it): z[0 .. z_bytes) the members back to back,
 * z_offsets[n_members + 1] their bounds, member_first[n_members + 1] each member's first message index (the last entry = n),
 * raw_bytes = out_bytes; all zero after a call without compression.  A member is the concatenation of its messages' encoded and framed
 * bytes, not a Kafka message set (fg_set_output_wire below builds that).  With compression set fg_transcode_batch runs in one piece: members are
 * not cut across the slices of its pipelined form. */
int fg_set_output_compression(fg_ctx* ctx, const fg_compress_cfg* cfg);
/* How the compressor codes a block, for fg_deflate_device and for the compress stage of the three transcode calls: a ctx setting like the
 * cfg above (fg_clone copies it), FG_DEFLATE_FIXED by default.  The wire format is gzip in either mode and fg_deflate_bound holds for both (no
 * block exceeds its stored form).  FG_ERR_ARG: a NULL ctx, any other mode.  In a build without the dynamic kernel the calls that would
 * compress answer FG_ERR_UNSUPPORTED while the mode is FG_DEFLATE_DYNAMIC. */
typedef enum fg_deflate_mode { FG_DEFLATE_FIXED = 0, FG_DEFLATE_DYNAMIC = 1 } fg_deflate_mode;
int fg_set_deflate_mode(fg_ctx* ctx, int mode);
typedef struct fg_compressed {
    const uint8_t* z;
    uint64_t z_bytes;
    const uint64_t* z_offsets;
    const uint64_t* member_first;
    uint64_t n_members;
    uint64_t raw_bytes;
} fg_compressed;
int fg_last_compressed(const fg_ctx* ctx, fg_compressed* out);

/* KAFKA v0 MESSAGE SETS ON THE GPU (additive under the same FG_ABI_VERSION).  The reference's Kafka output hands every encoded line to
 * the producer as a record with a null key (output/kafka_output.rs:68-112); the producer renders a request's records as a v0 MessageSet
 * and, with compression on, compresses THAT set and sends it as the value of one wrapper message.  This builds both in HBM, between the
 * encoder and the compressor.  All integers big-endian; a message is
 *     offset 8 (0: the broker assigns) | message_size 4 (14 + value length) | crc 4 | magic 1 (0) | attributes 1 | key length 4 (-1:
 *     a null key, no key bytes) | value length 4 | value
 * 26 bytes (fg_kafka_message_overhead()) around the value; crc = CRC-32 (IEEE, zlib's) of magic .. the value's end.  A message set is
 * messages back to back.  A gzip wrapper is one message with attributes = 1 whose value is a complete gzip member (what fg_deflate_device
 * makes of the inner set).  The format is the Kafka protocol guide's MessageSet v0; the producer crate's source was not compared against.
 *   fg_kafka_messageset_device   message i's value = d_bytes[d_offsets[i] .. d_offsets[i + 1]) (an encoder's out / out_offsets, merger
 *                       bytes included); d_skip: NULL, or n bytes, nonzero = the row is NOT in the set (an encoder's enc_status: the reference
 *                       never sends a line that failed); a row that is not skipped and has an empty value is a message with value length 0.
 *                       d_set_offsets[n + 1]: where each message lies in the set (a skipped row: an empty range).  d_set == NULL: a sizing
 *                       call (*total and d_set_offsets are set).  *total > set_cap: FG_ERR_ENT_OVERFLOW and d_set is not written.
 *                       FG_ERR_ARG: offsets that do not ascend or go past nbytes, a message whose wire size does not fit int32.
 *                       Synchronises the stream.  FG_ERR_UNSUPPORTED: a build without the kernels.
 *   fg_kafka_wrap_device   member m = d_z[d_z_offsets[m] .. d_z_offsets[m + 1]) (fg_deflate_device's z / z_offsets) -> one wrapper message
 *                       per NON-EMPTY member in d_w, d_w_offsets[n_members + 1] their bounds; an empty member produces no byte.  The same
 *                       contract: the sizing call, FG_ERR_ENT_OVERFLOW, FG_ERR_ARG for offsets that do not ascend or a member that does
 *                       not fit int32, the stream synchronised.
 *   fg_kafka_bound      bytes that always suffice for the plain set of n messages over nbytes AND for its n_members compressed members
 *                       in their wrappers
 * A caller with resident data composes fg_encode_device -> fg_kafka_messageset_device -> fg_deflate_device (cuts =
 * d_set_offsets[member_first[k]]) -> fg_kafka_wrap_device.  The output is a pure function of the input. */
uint32_t fg_kafka_message_overhead(void);
uint64_t fg_kafka_bound(uint64_t nbytes, uint64_t n, uint64_t n_members);
int fg_kafka_messageset_device(fg_ctx* ctx, const uint8_t* d_bytes, uint64_t nbytes, const uint64_t* d_offsets, const uint8_t* d_skip, uint64_t n,
                               uint8_t* d_set, uint64_t set_cap, uint64_t* d_set_offsets, uint64_t* total, void* stream);
int fg_kafka_wrap_device(fg_ctx* ctx, const uint8_t* d_z, const uint64_t* d_z_offsets, uint64_t n_members, uint8_t* d_w, uint64_t w_cap,
                         uint64_t* d_w_offsets, uint64_t* total, void* stream);
/* What the three transcode calls hand out: a ctx setting like fg_set_deflate_mode (fg_clone copies it), FG_WIRE_RAW by default, and then
 * nothing changes by a byte.  With FG_WIRE_KAFKA_V0 the calls run in one piece and build the message set behind the encoder: members are
 * cut by the ctx's fg_compress_cfg policy (coalesce / member_bytes over out_offsets, counted over ALL rows, skipped ones included; a cfg
 * with codec FG_COMP_NONE carries its policy too; no cfg or NULL: coalesce = 1), rows with enc_status != 0 are not in the set, and
 * fg_last_compressed hands out
 *     FG_COMP_GZIP   z = one wrapper message per non-empty member (the set deflated member by member, byte cuts
 *                    set_offsets[member_first[k]]), z_offsets their bounds
 *     FG_COMP_NONE   z = the plain message set, z_offsets[n_members + 1] the members' bounds in it
 * `out` is NULL, out_bytes and raw_bytes stay the encoder's total, out_offsets, meta and enc_status are unchanged.  A member whose rows
 * are all skipped is an empty set: no byte, no wrapper.  FG_ERR_ARG: a NULL ctx, any other value. */
typedef enum fg_output_wire { FG_WIRE_RAW = 0, FG_WIRE_KAFKA_V0 = 1 } fg_output_wire;
int fg_set_output_wire(fg_ctx* ctx, int wire);

/* Host memory for the framer's batch buffers (bytes, offsets): PAGE-LOCKED, through a process-wide pool -- a freed block is kept
 * (up to idle_bytes in total) and handed to the next request it fits, so a framer per connection does not pin and unpin megabytes per
 * connect; the bytes pinned through this allocator are capped at total_bytes, beyond which a request gets PAGEABLE memory (every
 * host-buffer entry point takes either: pinned = zero-copy / link-speed uploads, pageable = the runtime's staged copies).
 * Defaults: 8 GiB in total, 256 MiB idle (a measurement harness that keeps multi-GB batches pinned raises the cap: bench.py does).  Thread-safe.  fg_pinned_stats: what is pinned / idle / handed out right now. */
int fg_alloc_pinned(uint64_t bytes, void** out);
void fg_free_pinned(void* p);
int fg_set_pinned_limits(uint64_t total_bytes, uint64_t idle_bytes);
int fg_pinned_stats(uint64_t* pinned_bytes, uint64_t* idle_bytes, uint64_t* live_blocks);
/* 1: `p` (a pointer fg_alloc_pinned returned) is page-locked; 0: the cap was reached and the block is PAGEABLE memory -- the host-buffer
 * entry points then take their staged-copy forms, silently; -1: not a block of this allocator (fg_free_pinned ignores such a pointer:
 * it is the caller's to free). */
int fg_is_pinned(const void* p);

/* The host <-> device link of ctx's GPU, MEASURED: hipMemcpyAsync of a pinned buffer of `nbytes` (>= 64 MiB for a steady figure;
 * bench.py uses 1 GiB), best of three, in GB/s: gbps[0] host -> device, gbps[1] device -> host, gbps[2] both directions at once
 * on two streams (sum of both).  This is the roof the host-buffer entry points (fg_decode_batch, fg_transcode_batch ...) are
 * priced against -- SURVEY 8d: end-to-end is PCIe-bound -- instead of a nominal Gen5 figure. */
int fg_measure_link(fg_ctx* ctx, uint64_t nbytes, double gbps[3]);

/* CALIBRATION of the memory system the decode kernels run on, in the caller's process and on the caller's own resident buffer: a
 * plain streaming kernel over [d_src, d_src + nbytes) on `stream` (asynchronous; time it with events like a decode launch).
 *   FG_CALIB_COPY  float4 copy into d_dst (nbytes readable / writable, 16-byte aligned): 2 x nbytes of HBM traffic
 *   FG_CALIB_READ  read-only sweep (d_dst ignored): nbytes of traffic -- the roof of a decoder that writes little
 * bench.py reports both beside the decoder's achieved GB/s (roofline.copy_GBps / read_GBps) so that box-to-box variance is not
 * mistaken for a code change.  No reference analogue (measurement support). */
enum { FG_CALIB_COPY = 0, FG_CALIB_READ = 1,
       FG_CALIB_COPY_NT = 2,  /* the copy with non-temporal loads and stores */
       FG_CALIB_COPY_FLAT = 3 /* the copy as one 16-byte element per thread (no grid-stride loop) */ };
int fg_calibrate_device(fg_ctx* ctx, int mode, const uint8_t* d_src, uint8_t* d_dst, uint64_t nbytes, void* stream);

/* The reference's exact &'static str for a status code of a format (0 -> "", unknown -> NULL).
 * FG_CAPNP: 1 "Missing timestamp", 2 "Missing host name" (capnp_splitter.rs:135,140); 3 = the root pointer cannot be read (no
 * segment 0, a root that is not a struct pointer or points outside its segment, 512 or more segments, a message of 4 GiB or
 * more): the reference unwrap()s get_root() (:47), panics and loses the connection thread -- there is no &'static str, the text
 * is this library's own. */
const char* fg_error_string(fg_format fmt, uint8_t status);

/* Materialise rows [i0, i1) of HOST-visible tables into the canonical Record serialisation
 * (format documented in INTEGRATION.md; identical to what oracle/ emits for the reference
 * semantics).  out may be NULL to size; out_offsets (i1-i0+1 entries) may be NULL.
 * cfg supplies the LTSV suffixes (NULL otherwise).  Returns total bytes, or negative FG_ERR_*. */
int64_t fg_tables_serialize(fg_format fmt, const fg_cfg* cfg, const uint8_t* bytes,
                            const uint64_t* offsets, const fg_tables* tables, uint64_t i0,
                            uint64_t i1, uint8_t* out, uint64_t cap, uint64_t* out_offsets);

/* SIDE EFFECTS of decode(): the bytes the reference decoders write to the process's stdout while decoding rows [i0, i1), in row
 * order (SURVEY 8b "Side effects"; today one statement: LTSV's `println!("Missing value for name '{}'", name)`,
 * ltsv_decoder.rs:99 -- rows flagged FG_F_LTSV_NOVALUE).  A drop-in shim writes them to stdout after each batch.
 * `framing` says whether [offsets[i], offsets[i+1]) still carries its terminator (frames of fg_frame_decode_batch: FG_FRAME_LINE /
 * FG_FRAME_NUL) or is a bare line (FG_FRAME_NONE).  out may be NULL to size.  Returns the total bytes (even when > cap), or
 * negative FG_ERR_*.  Only `meta` and `hostname` of `tables` are read; hostname may be NULL (fg_transcode_batch returns the meta
 * column only): the count of a failed row then comes from its facility byte. */
int64_t fg_tables_stdout(fg_format fmt, fg_framing framing, const uint8_t* bytes, const uint64_t* offsets, const fg_tables* tables,
                         uint64_t i0, uint64_t i1, uint8_t* out, uint64_t cap);

/* Multi-GPU sharding plan (host): split n lines into g contiguous ranges balanced by BYTES;
 * line_starts receives g+1 line indices (line_starts[0] = 0, line_starts[g] = n). */
int fg_shard_plan(const uint64_t* offsets, uint64_t n, uint32_t g, uint64_t* line_starts);

/* ORDERED HOST GATHER of the multi-GPU path (order contract: handle_line runs in input order per
 * connection, src/flowgger/splitter/line_splitter.rs:17-54).  Every pointer is HOST memory (pinned or pageable);
 * plain memory moves threaded over row ranges, no GPU involved.
 *   fg_gather_size    sum of rows / used entries over the g parts (the capacity `out` needs)
 *   fg_gather_tables  parts = the tables of the g shards of ONE batch, in shard order (fg_shard_plan): `out` receives
 *                     their concatenation; ent_first is rebased onto the concatenated entry table, spans are
 *                     line-relative and are copied as they are.  out->n >= rows, out->ent_cap >= entries.
 *   fg_merge_tables   parts = sub-batches split off by FORMAT (BASELINE configuration 5: the reference has one decoder
 *                     per input, flowgger/mod.rs:413-422, so a mixed stream is decoded as tagged sub-batches);
 *                     index[k][j] = original position of row j of part k (strictly increasing inside a part, every
 *                     position 0..rows-1 exactly once): rows go back to their original positions;
 *                     src_part[i] (may be NULL) receives the part a row came from (= which decoder's error strings /
 *                     materialisation rules apply to it)
 *   fg_ordered_merge  the same for variable-size byte records (canonical Records, encoded messages): part k holds
 *                     m[k] records, record j = blobs[k][offs[k][j] .. offs[k][j+1]); out_offs receives rows+1 offsets;
 *                     returns the total bytes (call with out == NULL to size), negative FG_ERR_* on bad arguments */
int fg_gather_size(const fg_tables* parts, uint32_t g, uint64_t* n_rows, uint64_t* n_entries);
/* fg_merge_tables ON THE DEVICE (round 4): the parts' tables, index[k] and `out` are device memory (the sub-batches' tables as
 * fg_decode_batch_device left them, at most 8 parts); the rows go back to their arrival positions while everything is still in HBM --
 * ONE merged table then crosses the link instead of g tables plus a pass of the host's cores over all of them.  Round 5: the merged
 * ENTRIES are DENSE and in ARRIVAL order (row i's slice starts where row i-1's ends; ent_used = the sum of ent_count): the slots the
 * decoders' waves reserved but never used -- they lie between the slices of a decoder's own table -- do not cross the link.
 * Asynchronous on `stream`; the parts' entry counters are read on the device.  out->n must be the sum of the
 * parts' rows and out->ent_cap at least the sum of their ent_cap (checked); out->ent_used receives the merged entry count;
 * d_src_part (device, may be NULL) as src_part of fg_merge_tables.  The indices are the caller's contract (every position once) and
 * are not checked on the device.  What the kernels do with indices outside it (tests/merge_model.py): an index >= out->n is skipped;
 * a position NO index names comes back with ent_count = 0 AND ent_first = 0 and owns no entries, its other eight columns and its
 * d_src_part byte keep what they held; a row whose slice does not lie inside [0, min(*ent_used, ent_cap)) of its part (a row of a
 * table that overflowed) keeps its columns and owns no entries; nothing is stored at or behind out->ent_cap, whatever ent_used
 * reports.  A position named TWICE is undefined (two rows race for one set of columns; the entry copy may read outside a part). */
int fg_merge_tables_device(fg_ctx* ctx, const fg_tables* parts, uint32_t g, const uint64_t* const* d_index, const fg_tables* out,
                           uint8_t* d_src_part, void* stream);
int fg_gather_tables(const fg_tables* parts, uint32_t g, fg_tables* out);
int fg_merge_tables(const fg_tables* parts, uint32_t g, const uint64_t* const* index, fg_tables* out, uint8_t* src_part);
int64_t fg_ordered_merge(uint32_t g, const uint64_t* m, const uint64_t* const* index, const uint8_t* const* blobs,
                         const uint64_t* const* offs, uint8_t* out, uint64_t cap, uint64_t* out_offs);

/* Duration in milliseconds of the most recent decode kernel launch(es) of this ctx measured
 * with HIP events on the launch stream (0 when timing is disabled). fg_set_timing(ctx, 1)
 * enables event recording around every launch. */
int fg_set_timing(fg_ctx* ctx, int enabled);
int fg_last_kernel_ms(fg_ctx* ctx, float* ms);

/* Self-check of the dynamic chunk dispatch (round 5): the streaming decode kernels draw their chunks from a per-launch ticket counter
 * -- a word of a ctx-owned ring in device memory that is never reset: the host keeps what every word holds once the launches issued so
 * far have run (a launch adds exactly its number of chunks).  waits for the device, reads the ring back
 * and returns the number of words that differ from the host's books (0 = consistent; negative = an FG_ERR_* code).  A diagnostic
 * for tests and for a shim's debug builds; the decode path never calls it. */
int fg_ticket_ring_check(fg_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* FG_HIP_H */
