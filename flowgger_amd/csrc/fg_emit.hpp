// fg_emit.hpp -- the six Encoder::encode implementations + the three Merger::frame implementations, as
// per-record emitters that read a decode-table row (spans into the packed line bytes + the entry slice)
// and push the output bytes into a sink -- the Record is never materialised.
//
//   GelfEmitter         encoder/gelf_encoder.rs:59-115 (+ serde_json 0.8 serialisation of the BTreeMap)
//   LtsvEmitter         encoder/ltsv_encoder.rs:33-125
//   Rfc5424Emitter      encoder/rfc5424_encoder.rs:28-93  (+ impl Display for StructuredData, record.rs:42-67)
//   Rfc3164Emitter      encoder/rfc3164_encoder.rs:28-101
//   PassthroughEmitter  encoder/passthrough_encoder.rs:24-50
//   CapnpEmitter        encoder/capnp_encoder.rs:36-109 (+ capnp 0.14 serialize::write_message)
//   frame               merger/{line,nul,syslen}_merger.rs
//
// A Record field is a DECODED view of a span: raw bytes (RFC5424 / LTSV sources), unescape_sd_value
// (rfc5424_decoder.rs:105-125) for flagged RFC5424 SD values, JSON string unescaping (serde_json 0.8) for flagged
// spans of GELF-decoded records.  `for_each_decoded` streams that view byte by byte; every emitter is written
// against it, so the three decoders x five encoders all share one code path.
//
// Host + device (no HIP dependency): the kernels in fg_encode.hip instantiate the emitters with a GlobalReader and
// a count / write sink; tests/native/emit_host.cpp instantiates the same code on the CPU against the oracle.
#pragma once
#include <stdint.h>
#include <string.h>

#include "fg_dtoa.hpp"
#include "fg_unicode_ws.hpp"
#include "fg_shortest.hpp"
#include "fg_tables_view.hpp"
#include "fg_timeconv.hpp"

#if defined(__HIPCC__)
#define FGE_HD __host__ __device__ __forceinline__
#define FGE_HD_NOINLINE __host__ __device__
#else
#define FGE_HD inline
#define FGE_HD_NOINLINE inline
#endif

namespace fg {

// static key list entry of the GELF encoder (host-built, sorted by key): what the value is
enum : uint32_t { SK_APP = 0, SK_FULL = 1, SK_HOST = 2, SK_LEVEL = 3, SK_PROC = 4, SK_SDID = 5, SK_SHORT = 6, SK_TS = 7, SK_VERSION = 8, SK_EXTRA = 9 };
struct StaticKey {
    uint32_t key_off, key_len;    // the raw key bytes (for the merge with the record's own keys), into the blob
    uint32_t kind;                // SK_*
    // The member text up to the value's first own byte, TWICE (both 4-byte aligned in the blob, text_len bytes each): at text_off
    // behind a ',' -- `,"key":` with the key JSON-escaped --, at text1_off behind the '{' of an object it opens.  The kinds whose value
    // is always a string carry its opening quote (`,"host":"`), SK_VERSION and SK_EXTRA the whole member (`,"version":"1.1"`,
    // `,"key":"value"`): every byte that does not depend on the record is part of ONE piece (what a piece costs: PackSink::put_part).
    uint32_t text_off, text1_off, text_len;
};
struct EncCfg {
    const uint8_t* blob;       // GELF keys + extra values, LTSV suffixes, the LTSV extras text, the prepend header
    const StaticKey* keys;     // GELF: sorted by key bytes
    uint32_t n_keys;
    // LTSV suffixes of bool, f64, i64, u64 (len 0xFFFFFFFF = not configured).  Named fields, not arrays: ONE dynamically indexed
    // member keeps the whole struct -- a kernel argument -- in scratch memory, and every read of any field then waits behind the
    // lane's output stores (the compiler also turns a chain of selects over array elements back into an indexed load)
    uint32_t suf_off0, suf_off1, suf_off2, suf_off3, suf_len0, suf_len1, suf_len2, suf_len3;
    FGE_HD void set_suffix(uint32_t k, uint32_t off, uint32_t len) {
        if (k == 0u) { suf_off0 = off; suf_len0 = len; }
        else if (k == 1u) { suf_off1 = off; suf_len1 = len; }
        else if (k == 2u) { suf_off2 = off; suf_len2 = len; }
        else { suf_off3 = off; suf_len3 = len; }
    }
    uint32_t src_fmt;          // which decoder produced the tables (fg_format)
    uint32_t enc;              // fg_encoder
    uint32_t merger;           // fg_merger
    uint32_t ltsv_extra_off, ltsv_extra_len;  // "k1:v1\tk2:v2" (already escaped, '_' stripped); len 0 = none.  Capnp: the
                                              // output.capnp_extra list's byte image (8-byte aligned; CapnpEmitter)
    uint32_t prepend_off, prepend_len;        // syslog_prepend_timestamp header; len 0xFFFFFFFF = not configured
    double now_ts;             // Record.ts of rows flagged FG_F_TS_NOW
    uint32_t sort_slots;       // GELF: entries of the per-lane ranking scratch (<= kSortSlots)
    uint64_t out_cap;          // write pass: nonzero = leave the output alone when out_offsets[n] exceeds it (fg_encode_device_async)
};

// encode status per line (fg_encode_error_string)
enum : uint32_t {
    ES_OK = 0,
    ES_DECODE_FAILED = 1,       // the row's decode status is an error: nothing to encode
    ES_5424_DATE = 2,           // "Failed to parse date"                       rfc5424_encoder.rs:46
    ES_5424_FORMAT = 3,         // "Failed to parse date as Rfc3339 format"     rfc5424_encoder.rs:52
    ES_3164_TS = 4,             // "Failed to parse unix timestamp in RFC3164 encoder"  rfc3164_encoder.rs:53
    ES_PASSTHROUGH_EMPTY = 5    // "Cannot output empty raw message"            passthrough_encoder.rs:47
};

namespace emit {

enum : uint32_t { M_RAW = 0, M_SD = 1, M_JSON = 2, M_JSON_RETRY = 3, M_WSJOIN = 4 };

FGE_HD uint32_t hexv(uint32_t c) {
    if (c - '0' <= 9u) return c - '0';
    c |= 0x20u;
    if (c - 'a' <= 5u) return c - 'a' + 10u;
    return 0;
}

// Streams the decoded bytes of rd[off .. off+len) into f(byte).
// Code size matters here: the emitters instantiate this once per call site with the sink's escaping inlined into f,
// so every mode produces "up to four decoded bytes of this step" (w, little-endian; nb) and ALL modes share ONE
// call site of f (M_RAW: its own).
template <class R, class F>
FGE_HD void for_each_decoded(R& rd, uint32_t off, uint32_t len, uint32_t mode, F&& f) {
    if (mode == M_RAW) {
        for (uint32_t i = 0; i < len; ++i) f(rd.byte(off + i));
        return;
    }
    const bool retry = mode == M_JSON_RETRY;
    bool esc = false;                  // M_SD: the previous byte was an unconsumed backslash
    bool in_tok = false, any = false;  // M_WSJOIN
    for (uint32_t i = 0; i < len;) {
        const uint32_t c = rd.byte(off + i);
        uint32_t w = c, nb = 1u;
        if (mode == M_SD) {  // unescape_sd_value: \" \\ \] lose the backslash, any other \x keeps both
            ++i;
            if (!esc) {
                if (c == '\\') {
                    esc = true;
                    nb = 0u;
                }
            } else {
                if (c != '"' && c != '\\' && c != ']') {
                    w = (uint32_t)'\\' | c << 8;
                    nb = 2u;
                }
                esc = false;
            }
        } else if (mode == M_WSJOIN) {  // str::split_whitespace(..).join(" ") (RFC3164 msg, rfc3164_decoder.rs:70)
            const uint32_t ws = r3164::ws_at(rd, off + i, off + len);
            if (ws) {
                in_tok = false;
                i += ws;
                nb = 0u;
            } else {
                ++i;
                if (!in_tok) {
                    if (any) {
                        w = (uint32_t)' ' | c << 8;
                        nb = 2u;
                    }
                    in_tok = any = true;
                }
            }
        } else if (c != '\\' || i + 1 >= len) {  // JSON escapes of an already validated string body: a plain byte
            ++i;
        } else {
            const uint32_t e = rd.byte(off + i + 1);
            i += 2;
            if (retry && e == '\n') {  // the reference replaced LF by "\\n": an escaped backslash, then 'n'
                w = (uint32_t)'\\' | (uint32_t)'n' << 8;
                nb = 2u;
            } else if (e == 'b') w = 8u;
            else if (e == 'f') w = 12u;
            else if (e == 'n') w = 10u;
            else if (e == 'r') w = 13u;
            else if (e == 't') w = 9u;
            else if (e == 'u') {
                if (i + 4 > len) {
                    nb = 0u;
                } else {
                    uint32_t n1 = hexv(rd.byte(off + i)) << 12 | hexv(rd.byte(off + i + 1)) << 8 | hexv(rd.byte(off + i + 2)) << 4 | hexv(rd.byte(off + i + 3));
                    i += 4;
                    if (n1 >= 0xD800u && n1 <= 0xDBFFu && i + 6 <= len) {
                        const uint32_t n2 = hexv(rd.byte(off + i + 2)) << 12 | hexv(rd.byte(off + i + 3)) << 8 | hexv(rd.byte(off + i + 4)) << 4 | hexv(rd.byte(off + i + 5));
                        i += 6;
                        n1 = (((n1 - 0xD800u) << 10) | (n2 - 0xDC00u)) + 0x10000u;
                    }
                    if (n1 < 0x80u) {
                        w = n1;
                    } else if (n1 < 0x800u) {
                        w = (0xC0u | (n1 >> 6)) | (0x80u | (n1 & 0x3Fu)) << 8;
                        nb = 2u;
                    } else if (n1 < 0x10000u) {
                        w = (0xE0u | (n1 >> 12)) | (0x80u | ((n1 >> 6) & 0x3Fu)) << 8 | (0x80u | (n1 & 0x3Fu)) << 16;
                        nb = 3u;
                    } else {
                        w = (0xF0u | (n1 >> 18)) | (0x80u | ((n1 >> 12) & 0x3Fu)) << 8 | (0x80u | ((n1 >> 6) & 0x3Fu)) << 16 | (0x80u | (n1 & 0x3Fu)) << 24;
                        nb = 4u;
                    }
                }
            } else {
                w = e;  // " \ /
            }
        }
        for (uint32_t j = 0; j < nb; ++j) f((w >> (8u * j)) & 0xFFu);
    }
}

// ---- sinks.  Protocol: put(c) one byte; put_word(w, nb) nb = 1..4 bytes, little-endian in w, the bytes above nb zero;
//      finish().  kCount sinks only count (add(n) = n bytes whose values do not matter). -----------------------------
struct CountSink {
    static constexpr bool kCount = true;
    uint32_t n = 0;
    uint32_t slow = 0;  // spans that held a byte to escape (Base::copy_raw): 0 = the write pass may copy this row's spans untested
    FGE_HD void mark_slow() { slow = 1u; }
    FGE_HD void put(uint32_t) { ++n; }
    FGE_HD void put_word(uint32_t, uint32_t nb) { n += nb; }
    FGE_HD void put16(uint32_t, uint32_t, uint32_t, uint32_t) { n += 16u; }
    FGE_HD void put_part(uint32_t, uint32_t, uint32_t, uint32_t, uint32_t nb) { n += nb; }
    FGE_HD void add(uint32_t k) { n += k; }
    FGE_HD void finish() {}
};
// Packs the byte stream into ALIGNED 16-BYTE stores (round 5; rounds 1-4: aligned dword stores).  A lane streams its own message, so
// one store instruction of the wave touches 64 different cache lines whatever its width -- the store path handles those one line per
// cycle: per-lane dword stores ran the write kernel at 0.9 TB/s of output (2.6 ms for the 2.4 GB of the 4 M-line corpus, the whole
// difference between the count pass and the write pass), per-lane 16-byte stores move the same bytes in a quarter of the store
// instructions: 3.0 TB/s (tools/probe/store_patterns.cpp, profiles/r05c_store_patterns.log; staging the bytes through LDS for
// wave-cooperative flushes measured SLOWER than that: 2.5 TB/s).  Messages of neighbouring lines are adjacent in the output and are
// written by other lanes at the same time, so nothing outside [q, q + length) may be touched: the first and the last 16-byte block of
// a message are stored by dwords and bytes, only over bytes that are the message's own.
struct PackSink {
    static constexpr bool kCount = false;
    struct alignas(16) Block { uint32_t x, y, z, w; };
    uint8_t* p;     // 16-byte aligned address of the block being assembled (after finish(): the end of the message)
    uint32_t b0 = 0, b1 = 0, b2 = 0, b3 = 0;  // its completed dwords
    uint32_t acc = 0;  // the dword being assembled: its low (k & 3) bytes are valid (placeholders where `head` says so)
    uint32_t k;        // bytes of the block that are filled, 0..15
    uint32_t head;     // bytes at the start of the FIRST block that belong to the previous message (0 once that block is out)
    FGE_HD explicit PackSink(uint8_t* q) {
        head = (uint32_t)((uintptr_t)q & 15u);
        p = q - head;
        k = head;
    }
    FGE_HD uint32_t dword_of(uint32_t d) const { return d == 0u ? b0 : d == 1u ? b1 : d == 2u ? b2 : b3; }
    // (the output lies in global memory: said explicitly, or the kernels' stores are flat_ instructions -- a slower address path that
    //  also counts against the LDS wait counter)
    template <class T>
    static FGE_HD void st(uint8_t* q, const T& v) {
#if defined(__HIP_DEVICE_COMPILE__)
        *reinterpret_cast<T __attribute__((address_space(1)))*>((uint8_t __attribute__((address_space(1)))*)q) = v;
#else
        *reinterpret_cast<T*>(q) = v;
#endif
    }
    // bytes [lo, hi) of the block at q, from its completed dwords (index < full) and `ac` (index == full): whole dwords as dwords.
    // A message's first and last block only -- ONE copy of the code per kernel, by value (inlined at each of the emitters' ~150 sink
    // calls it was most of the write kernel's 74 000 vector instructions).
#if defined(__HIP_DEVICE_COMPILE__)
    static __device__ __attribute__((noinline))
#else
    static inline
#endif
    void store_part_at(uint8_t* q, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t ac, uint32_t lo, uint32_t hi, uint32_t full) {
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
        for (uint32_t d = 0; d < 4u; ++d) {
            const uint32_t a = d * 4u > lo ? d * 4u : lo, e = d * 4u + 4u < hi ? d * 4u + 4u : hi;
            if (a >= e) continue;
            const uint32_t v = d < full ? (d == 0u ? w0 : d == 1u ? w1 : d == 2u ? w2 : w3) : ac;
            if (e - a == 4u) {
                st<uint32_t>(q + d * 4u, v);
            } else {
                for (uint32_t i = a; i < e; ++i) st<uint8_t>(q + i, (uint8_t)(v >> (8u * (i & 3u))));
            }
        }
    }
    FGE_HD void store_part(uint32_t lo, uint32_t hi, uint32_t full) { store_part_at(p, b0, b1, b2, b3, acc, lo, hi, full); }
    static FGE_HD void st16(uint8_t* q, uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
#if defined(__HIP_DEVICE_COMPILE__)
        typedef uint32_t v4u __attribute__((ext_vector_type(4)));  // (a vector, not a struct: an aggregate copy forgets the address space)
        const v4u v = {x, y, z, w};
        *reinterpret_cast<v4u __attribute__((address_space(1)))*>((uint8_t __attribute__((address_space(1)))*)q) = v;
#else
        *reinterpret_cast<Block*>(q) = Block{x, y, z, w};
#endif
    }
    // 32-bit arithmetic only (64-bit shifts are slow on the vector ALU): w's low bytes complete the dword, its high
    // bytes start the next one
    FGE_HD void put_word(uint32_t w, uint32_t nb) {
        const uint32_t kb = k & 3u, sh = 8u * kb;
        const uint32_t lo = acc | (w << sh);
        if (kb + nb >= 4u) {
            const uint32_t d = k >> 2;  // (selects, not an array: a dynamically indexed local array lives in scratch memory)
            b0 = d == 0u ? lo : b0;
            b1 = d == 1u ? lo : b1;
            b2 = d == 2u ? lo : b2;
            b3 = d == 3u ? lo : b3;
            acc = sh ? w >> (32u - sh) : 0u;
            k += nb;
            if (k >= 16u) {  // the block is complete
                if (head) {
                    store_part(head, 16u, 4u);
                    head = 0;
                } else {
                    st16(p, b0, b1, b2, b3);
                }
                p += 16;
                k -= 16u;
            }
        } else {
            acc = lo;
            k += nb;
        }
    }
    // bytes [4 - sh, 8 - sh) of the eight bytes lo | hi << 32: the dword that a left shift by sh bytes moves across a dword boundary
    static FGE_HD uint32_t carry_bytes(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
        return __builtin_amdgcn_perm(hi, lo, 0x03020100u + (4u - sh) * 0x01010101u);  // (one v_perm_b32; 64-bit shifts are slow)
#else
        return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * (4u - sh)));
#endif
    }
    // SIXTEEN bytes at once (the span copies: one LDS round trip of input): the block position k does not change, so exactly ONE
    // block completes per call -- whatever k is -- and every lane of a wave that copies a span stores its 16 bytes in the SAME store
    // instruction.  (Four put_word calls complete the block at a lane-specific call: four store instructions with a quarter of the
    // lanes each, and the write kernel gained nothing from 16-byte stores that way -- profiles/r05d_*cfg1*.)
    FGE_HD void put16(uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3) {
        const uint32_t d = k >> 2, sh = k & 3u;
        const uint32_t t0 = carry_bytes(q0, 0u, sh), t1 = carry_bytes(q1, q0, sh), t2 = carry_bytes(q2, q1, sh), t3 = carry_bytes(q3, q2, sh),
                       t4 = carry_bytes(0u, q3, sh);
        const uint32_t a0 = acc | t0;  // (acc holds the low sh bytes, t0 the rest: they do not overlap)
        // the block: its first d dwords are there already, then a0, then t1 ...; what does not fit starts the next block
        const uint32_t o0 = d == 0u ? a0 : b0;
        const uint32_t o1 = d == 0u ? t1 : d == 1u ? a0 : b1;
        const uint32_t o2 = d == 0u ? t2 : d == 1u ? t1 : d == 2u ? a0 : b2;
        const uint32_t o3 = d == 0u ? t3 : d == 1u ? t2 : d == 2u ? t1 : a0;
        if (head) {
            b0 = o0;
            b1 = o1;
            b2 = o2;
            b3 = o3;
            store_part(head, 16u, 4u);
            head = 0;
        } else {
            st16(p, o0, o1, o2, o3);
        }
        p += 16;
        b0 = d == 1u ? t3 : d == 2u ? t2 : t1;
        b1 = d == 2u ? t3 : t2;
        b2 = t3;
        acc = t4;
    }
    // ONE TO SIXTEEN bytes at once, nb of them, in q0 .. q3 (little-endian; the bytes beyond nb must be ZERO): the tail of a span, a
    // key's text, a number's digits.  Branch-free but for the store: a message is ~85 short pieces (puts of one to four bytes) around
    // its two dozen 16-byte copies, the lanes of a wave hold their blocks at 64 different fill levels, so some lane completes a block
    // at EVERY short put and the wave runs both sides of put_word's branches every time -- fewer, larger pieces are what the write
    // pass's instruction count is made of.
    FGE_HD void put_part(uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3, uint32_t nb) {
        const uint32_t d = k >> 2, sh = k & 3u;
        const uint32_t t0 = carry_bytes(q0, 0u, sh), t1 = carry_bytes(q1, q0, sh), t2 = carry_bytes(q2, q1, sh), t3 = carry_bytes(q3, q2, sh),
                       t4 = carry_bytes(0u, q3, sh);
        const uint32_t a0 = acc | t0;
        // the stream's dwords 0 .. 7 from the block's start: the d complete ones, a0, t1 .. t4, zeros
        const uint32_t o0 = d == 0u ? a0 : b0;
        const uint32_t o1 = d == 0u ? t1 : d == 1u ? a0 : b1;
        const uint32_t o2 = d == 0u ? t2 : d == 1u ? t1 : d == 2u ? a0 : b2;
        const uint32_t o3 = d == 0u ? t3 : d == 1u ? t2 : d == 2u ? t1 : a0;
        const uint32_t n0 = d == 0u ? t4 : d == 1u ? t3 : d == 2u ? t2 : t1;
        const uint32_t n1 = d == 1u ? t4 : d == 2u ? t3 : d == 3u ? t2 : 0u;
        const uint32_t n2 = d == 2u ? t4 : d == 3u ? t3 : 0u;
        const uint32_t n3 = d == 3u ? t4 : 0u;
        const uint32_t k2 = k + nb;
        const bool full = k2 >= 16u;
        if (full) {
            if (head) {
                b0 = o0;
                b1 = o1;
                b2 = o2;
                b3 = o3;
                store_part(head, 16u, 4u);
                head = 0;
            } else {
                st16(p, o0, o1, o2, o3);
            }
            p += 16;
        }
        b0 = full ? n0 : o0;
        b1 = full ? n1 : o1;
        b2 = full ? n2 : o2;
        b3 = full ? n3 : o3;
        k = full ? k2 - 16u : k2;
        const uint32_t dn = k >> 2;  // (the dword being assembled: its bytes beyond k are zero because q's beyond nb are)
        acc = dn == 0u ? b0 : dn == 1u ? b1 : dn == 2u ? b2 : b3;
    }
    FGE_HD void put(uint32_t c) { put_word(c & 0xFFu, 1u); }
    FGE_HD void add(uint32_t) {}
    FGE_HD void mark_slow() {}
    FGE_HD void finish() {
        if (k > head) store_part(head, k, k >> 2);
        p += k;
        head = 0;
        k = 0;
        acc = 0;
    }
};

// SWAR byte tests on a dword (exact as booleans: nonzero iff some byte matches)
FGE_HD uint32_t swar_zero(uint32_t v) { return (v - 0x01010101u) & ~v & 0x80808080u; }
FGE_HD uint32_t swar_lt20(uint32_t w) { return (w - 0x20202020u) & ~w & 0x80808080u; }
FGE_HD uint32_t swar_has(uint32_t w, uint32_t c) { return swar_zero(w ^ (c * 0x01010101u)); }
enum : uint32_t { ESC_NONE = 0, ESC_JSON = 1, ESC_LTSV_VAL = 2 };
template <uint32_t ESC>
FGE_HD bool word_needs_bytes(uint32_t w) {
    if (ESC == ESC_JSON) return (swar_lt20(w) | swar_has(w, '"') | swar_has(w, '\\')) != 0;
    if (ESC == ESC_LTSV_VAL) return (swar_has(w, '\t') | swar_has(w, '\n')) != 0;
    return false;
}
// the same tests without their final mask (bit 7 of a byte set = candidate): the terms of several dwords are OR-ed and masked ONCE --
// one compare and one branch per sixteen bytes instead of four short-circuit tests
FGE_HD uint32_t swar_zero_raw(uint32_t v) { return (v - 0x01010101u) & ~v; }
template <uint32_t ESC>
FGE_HD uint32_t word_needs_raw(uint32_t w) {
    if (ESC == ESC_JSON) return ((w - 0x20202020u) & ~w) | swar_zero_raw(w ^ 0x22222222u) | swar_zero_raw(w ^ 0x5C5C5C5Cu);
    if (ESC == ESC_LTSV_VAL) return swar_zero_raw(w ^ 0x09090909u) | swar_zero_raw(w ^ 0x0A0A0A0Au);
    return 0u;
}
template <uint32_t ESC>
FGE_HD bool any16_needs_bytes(uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3) {
    return ((word_needs_raw<ESC>(q0) | word_needs_raw<ESC>(q1) | word_needs_raw<ESC>(q2) | word_needs_raw<ESC>(q3)) & 0x80808080u) != 0u;
}

// decimal text of v through f(char code), without a digit buffer (a dynamically indexed local array is scratch
// memory on the GPU): 2 + 9 + 9 digits, leading zeros suppressed
template <class F>
FGE_HD void u64_digits(uint64_t v, F&& f) {
    const uint32_t c0 = (uint32_t)(v % 1000000000ull);
    const uint64_t r = v / 1000000000ull;
    const uint32_t c1 = (uint32_t)(r % 1000000000ull), c2 = (uint32_t)(r / 1000000000ull);  // c2 <= 18
    bool started = false;
    for (uint32_t chunk = 0; chunk < 3u; ++chunk) {
        const uint32_t c = chunk == 0 ? c2 : chunk == 1 ? c1 : c0;
        for (uint32_t p = chunk == 0 ? 10u : 100000000u; p; p /= 10u) {
            const uint32_t d = c / p % 10u;
            if (d || started || (chunk == 2u && p == 1u)) {
                f((uint32_t)'0' + d);
                started = true;
            }
        }
    }
}

// A line's table row in registers.  The kernel fetches it BEFORE it stages the tile (every load in flight, hidden
// behind the staging) and hands it to the emitter; without it the emitter fetches the row itself (load_row()).
struct RowRegs {
    fg_span s0, s1, s2, s3, s4, s5;
    double ts;
    uint32_t ef, ec;
    uint32_t plain = 0;  // write pass: the count pass found no byte to escape in any span it tested (row_size's *plain)
    FGE_HD void load(const DevTables& t, uint64_t li) {
        s0 = t.span[0][li];
        s1 = t.span[1][li];
        s2 = t.span[2][li];
        s3 = t.span[3][li];
        s4 = t.span[4][li];
        s5 = t.span[5][li];
        ts = t.ts[li];
        ef = t.ent_first[li];
        ec = t.ent_count[li];
    }
};

// a sink over a per-byte functor (a pair's value on its way through an escaper): pieces are taken apart again
template <class F>
struct FnSinkT {
    static constexpr bool kCount = false;
    F& f;
    FGE_HD void put(uint32_t c) { f(c); }
    FGE_HD void add(uint32_t) {}
    FGE_HD void put_part(uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3, uint32_t nb) {
        for (uint32_t i = 0; i < nb; ++i) f(((i < 4u ? q0 : i < 8u ? q1 : i < 12u ? q2 : q3) >> (8u * (i & 3u))) & 0xFFu);
    }
    FGE_HD void put16(uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3) { put_part(q0, q1, q2, q3, 16u); }
};

// Everything the emitters share: the row, the field views, the number formats.
template <class S, class R>
struct Base {
    S& out;
    const EncCfg& cfg;
    R rd;  // the line's bytes
    const DevTables& t;
    uint64_t li;
    uint32_t meta;
    // the line's table row, fetched ONCE with every load in flight (load_row(), first thing the emitters do): fetched
    // where they are used, each of the ~10 fields costs the wave a dependent HBM round trip
    fg_span s0{}, s1{}, s2{}, s3{}, s4{}, s5{};
    double row_ts = 0.0;
    uint32_t row_ef = 0, row_ec = 0;
    // The count pass has tested every span copy_raw moves and found no byte that needs escaping: the write pass copies them untested
    // (the three SWAR tests are 52 of the ~95 instructions a 16-byte step costs).  False = test, as the count pass itself does.
    bool plain = false;
    FGE_HD void load_row(const RowRegs* pre) {
        if (pre) {
            plain = pre->plain != 0u;
            s0 = pre->s0;
            s1 = pre->s1;
            s2 = pre->s2;
            s3 = pre->s3;
            s4 = pre->s4;
            s5 = pre->s5;
            row_ts = pre->ts;
            row_ef = pre->ef;
            row_ec = pre->ec;
            return;
        }
        s0 = t.span[0][li];
        s1 = t.span[1][li];
        s2 = t.span[2][li];
        s3 = t.span[3][li];
        s4 = t.span[4][li];
        s5 = t.span[5][li];
        row_ts = t.ts[li];
        row_ef = t.ent_first[li];
        row_ec = t.ent_count[li];
    }
    FGE_HD fg_span span(int col) const {  // scalar selects (a ternary chain over the structs kept the emitter in memory)
        fg_span r;
        r.off = col == 0 ? s0.off : col == 1 ? s1.off : col == 2 ? s2.off : col == 3 ? s3.off : col == 4 ? s4.off : s5.off;
        r.len = col == 0 ? s0.len : col == 1 ? s1.len : col == 2 ? s2.len : col == 3 ? s3.len : col == 4 ? s4.len : s5.len;
        return r;
    }

    FGE_HD uint32_t flags() const { return FG_META_FLAGS(meta); }
    FGE_HD uint32_t json_mode() const { return (flags() & FG_F_GELF_RETRY) ? (uint32_t)M_JSON_RETRY : (uint32_t)M_JSON; }
    // decode mode of a top-level string field
    FGE_HD uint32_t field_mode(int col) const {
        if (cfg.src_fmt == FG_RFC3164) return (col == S_MSG && (flags() & FG_F_MSG_JOIN)) ? (uint32_t)M_WSJOIN : (uint32_t)M_RAW;
        if (cfg.src_fmt != FG_GELF) return M_RAW;
        const uint32_t bit = col == S_HOST ? FG_F_HOST_ESC : col == S_MSG ? FG_F_MSG_ESC : col == S_FULL ? FG_F_FULLMSG_ESC : 0u;
        return (flags() & bit) ? json_mode() : (uint32_t)M_RAW;
    }
    FGE_HD uint32_t value_mode(uint32_t e) const {
        if (!(t.ent_flags[e] & FG_EF_VAL_ESC)) return M_RAW;
        return cfg.src_fmt == FG_RFC5424 ? (uint32_t)M_SD : cfg.src_fmt == FG_GELF ? json_mode() : (uint32_t)M_RAW;
    }
    FGE_HD double record_ts() const { return (flags() & FG_F_TS_NOW) ? cfg.now_ts : row_ts; }

    // a literal (n <= 32 bytes, known at the call site: the words below fold into constants), as ONE piece per sixteen bytes -- and
    // with the byte `lead` in front of it when the caller has one (a separator: a put of its own costs what a piece does)
    FGE_HD void lit(const char* s, uint32_t n, uint32_t lead = 0u) {
        if (S::kCount) {
            out.add(n + (lead ? 1u : 0u));
            return;
        }
        uint32_t q[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u}, p[8] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};  // without / behind the lead byte
        for (uint32_t i = 0; i < n && i < 31u; ++i) {
            q[i >> 2] |= (uint32_t)(uint8_t)s[i] << (8u * (i & 3u));
            p[(i + 1u) >> 2] |= (uint32_t)(uint8_t)s[i] << (8u * ((i + 1u) & 3u));
        }
        const bool ld = lead != 0u;
        const uint32_t m = n + (ld ? 1u : 0u);
        const uint32_t w0 = ld ? (p[0] | lead) : q[0], w1 = ld ? p[1] : q[1], w2 = ld ? p[2] : q[2], w3 = ld ? p[3] : q[3];
        if (m <= 16u) {
            out.put_part(w0, w1, w2, w3, m);
        } else {
            out.put16(w0, w1, w2, w3);
            out.put_part(ld ? p[4] : q[4], ld ? p[5] : q[5], ld ? p[6] : q[6], ld ? p[7] : q[7], m - 16u);
        }
    }
    // a piece of the configuration blob; every piece starts 4-byte aligned and is followed by readable padding
    FGE_HD void blob(uint32_t off, uint32_t len) {
        if (S::kCount) {
            out.add(len);
            return;
        }
        const uint32_t* w = reinterpret_cast<const uint32_t*>(cfg.blob + off);
        uint32_t i = 0;
        for (; i + 16u <= len; i += 16u) out.put16(w[i >> 2], w[(i >> 2) + 1u], w[(i >> 2) + 2u], w[(i >> 2) + 3u]);
        if (i < len) {  // (the blob ends in sixteen bytes of padding: fg_enc_cfg.hpp)
            uint32_t q[4] = {w[i >> 2], w[(i >> 2) + 1u], w[(i >> 2) + 2u], w[(i >> 2) + 3u]};
            keep_low(q, len - i);
            out.put_part(q[0], q[1], q[2], q[3], len - i);
        }
    }
    // rd[off .. off+len) copied through the per-byte functor `fb` only where a dword holds a byte that needs it
    // (ESC): everything else moves four bytes at a time
    // the low nb (0 .. 16) of the sixteen bytes q[0 .. 3]; the rest zero
    static FGE_HD void keep_low(uint32_t* q, uint32_t nb) {
#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll
#endif
        for (uint32_t j = 0; j < 4u; ++j) {
            const uint32_t v = nb > 4u * j ? nb - 4u * j : 0u;  // this dword's bytes
            q[j] = v >= 4u ? q[j] : (q[j] & ((1u << (8u * v)) - 1u));
        }
    }
    // byte c becomes byte `at` (0 .. 15) of the sixteen bytes q[0 .. 3] (which is zero there)
    static FGE_HD void set_byte(uint32_t* q, uint32_t at, uint32_t c) {
        const uint32_t w = c << (8u * (at & 3u)), j = at >> 2;
        q[0] |= j == 0u ? w : 0u;
        q[1] |= j == 1u ? w : 0u;
        q[2] |= j == 2u ? w : 0u;
        q[3] |= j == 3u ? w : 0u;
    }
    // rd[off .. off+len) copied through the per-byte functor `fb` only where a dword holds a byte that needs it
    // (ESC): everything else moves sixteen bytes at a time, the span's last 1 .. 15 bytes as ONE piece -- with the byte `sfx` behind
    // them when the caller has one (a string's closing quote: a put of its own costs what a whole piece does, PackSink::put_part)
    template <uint32_t ESC, class FB>
    FGE_HD void copy_raw(uint32_t off, uint32_t len, FB&& fb, uint32_t sfx = 0u) {
        if (ESC == ESC_NONE && S::kCount) {
            out.add(len + (sfx ? 1u : 0u));
            return;
        }
        uint32_t i = 0;
        for (; i + 16u <= len; i += 16u) {  // 16 bytes per LDS round trip (the copy is latency-bound: one wave or two per SIMD)
            uint32_t q[4];
            rd.load16(off + i, q);
            if (plain || !any16_needs_bytes<ESC>(q[0], q[1], q[2], q[3])) {
                out.put16(q[0], q[1], q[2], q[3]);
                continue;
            }
            out.mark_slow();
            slow16<ESC>(q, 16u, fb);
        }
        const uint32_t nb = len - i;  // 0 .. 15
        if (nb == 0u && !sfx) return;
        uint32_t q[4] = {0u, 0u, 0u, 0u};
        if (nb) {
            rd.load16p(off + i, nb, q);
            keep_low(q, nb);
            // (the bytes beyond nb are zero: for the escape test they read as plain letters)
            const uint32_t fill = 0x61616161u;
            const uint32_t f0 = nb >= 4u ? 0u : fill << (8u * nb), f1 = nb >= 8u ? 0u : nb <= 4u ? fill : fill << (8u * (nb - 4u)),
                           f2 = nb >= 12u ? 0u : nb <= 8u ? fill : fill << (8u * (nb - 8u)), f3 = nb <= 12u ? fill : fill << (8u * (nb - 12u));
            if (!plain && any16_needs_bytes<ESC>(q[0] | f0, q[1] | f1, q[2] | f2, q[3] | f3)) {
                out.mark_slow();
                slow16<ESC>(q, nb, fb);
                if (sfx) out.put(sfx);
                return;
            }
        }
        if (sfx) set_byte(q, nb, sfx);
        out.put_part(q[0], q[1], q[2], q[3], nb + (sfx ? 1u : 0u));
    }
    // nb (1 .. 16) bytes in q with a byte that needs fb among them: dword by dword, byte-wise only where it is
    template <uint32_t ESC, class FB>
    FGE_HD void slow16(const uint32_t* q, uint32_t nb, FB&& fb) {
        for (uint32_t j = 0; j < 4u && 4u * j < nb; ++j) {
            const uint32_t w = j == 0u ? q[0] : j == 1u ? q[1] : j == 2u ? q[2] : q[3];
            const uint32_t m = nb - 4u * j < 4u ? nb - 4u * j : 4u;
            if (m == 4u && !word_needs_bytes<ESC>(w)) {
                out.put_word(w, 4u);
                continue;
            }
            for (uint32_t b = 0; b < m; ++b) fb((w >> (8u * b)) & 0xFFu);
        }
    }
    FGE_HD void raw_field(int col, uint32_t sfx = 0u) {  // a top-level field, decoded, unmodified [+ the separator behind it]
        const fg_span s = this->span(col);
        const uint32_t mode = field_mode(col);
        if (mode == M_RAW) {
            copy_raw<ESC_NONE>(s.off, s.len, [&](uint32_t c) { out.put(c); }, sfx);
            return;
        }
        for_each_decoded(rd, s.off, s.len, mode, [&](uint32_t c) { out.put(c); });
        if (sfx) out.put(sfx);
    }
    // two decimal digits as two ASCII bytes (the tens in the low byte), v < 100
    static FGE_HD uint32_t d2(uint32_t v) { return ((uint32_t)'0' + v / 10u) | ((uint32_t)'0' + v % 10u) << 8; }
    FGE_HD void u64_text(uint64_t v) {
        if (v < 1000u) {  // level, facility, small typed values: the common case, one piece
            const uint32_t x = (uint32_t)v, nd = x >= 100u ? 3u : x >= 10u ? 2u : 1u;
            const uint32_t h = (uint32_t)'0' + x / 100u, m = (uint32_t)'0' + x / 10u % 10u, l = (uint32_t)'0' + x % 10u;
            out.put_part(nd == 3u ? (h | m << 8 | l << 16) : nd == 2u ? (m | l << 8) : l, 0u, 0u, 0u, nd);
            return;
        }
        u64_digits(v, [&](uint32_t c) { out.put(c); });
    }
    FGE_HD void i64_text(int64_t x) {
        if (x < 0) {
            out.put('-');
            u64_text(0ull - (uint64_t)x);
        } else {
            u64_text((uint64_t)x);
        }
    }
    FGE_HD void pad2(uint32_t v) {
        out.put('0' + v / 10u);
        out.put('0' + v % 10u);
    }
    // <pri>: ((facility << 3) & 0xF8) + (severity & 7) in u8 arithmetic
    FGE_HD void pri() {  // "<" + 1..3 digits + ">": one piece
        const uint32_t npri = (((FG_META_FACILITY(meta) << 3) & 0xF8u) + (FG_META_SEVERITY(meta) & 7u)) & 0xFFu;
        const uint32_t nd = npri >= 100u ? 3u : npri >= 10u ? 2u : 1u;
        const uint32_t h = npri / 100u, m = npri / 10u % 10u, l = npri % 10u;
        // bytes: '<' d.. '>'
        const uint32_t digits = nd == 3u ? (('0' + h) | ('0' + m) << 8 | ('0' + l) << 16) : nd == 2u ? (('0' + m) | ('0' + l) << 8) : ('0' + l);
        const uint32_t w0 = (uint32_t)'<' | digits << 8;                 // '<' + up to three digits
        const uint32_t gt = (uint32_t)'>';
        // '>' lands at byte 1 + nd: in w0 for nd <= 2, in w1 for nd == 3
        out.put_part(nd == 3u ? w0 : (w0 | gt << (8u * (1u + nd))), nd == 3u ? gt : 0u, 0u, 0u, nd + 2u);
    }
    FGE_HD bool has_pri() const { return FG_META_FACILITY(meta) != 0xFFu && FG_META_SEVERITY(meta) != 0xFFu; }

    // ---- entry names: the Record key is '_' + name [+ LTSV suffix]; for GELF-decoded records the '_' is only added
    //      when the (decoded) key does not start with one (gelf_decoder.rs:99-103) ------------------------------------
    struct Dyn {
        uint32_t off, len;  // raw name span
        uint32_t mode;      // M_RAW / M_JSON*
        uint32_t skip;      // decoded bytes to skip: 1 when a GELF key already starts with '_'
        uint32_t dlen;      // decoded length after the skip
        uint32_t so, sl;    // suffix in the blob (sl = 0: none)
        uint32_t pfx;       // 1: the Record key is '_' + these bytes; 0: the bytes alone -- an FG_CAPNP `extra` whose key starts
                            //    with no '_' (FG_EF_NAME_VERBATIM, capnp_splitter.rs:104-108)
    };
    FGE_HD Dyn dyn_of(uint32_t e) {
        const fg_span nm = t.ent_name[e];
        Dyn d{nm.off, nm.len, M_RAW, 0u, nm.len, 0u, 0u, 1u};
        const uint32_t ty = t.ent_type[e];
        const uint32_t ef = t.ent_flags[e];
        if (cfg.src_fmt == FG_GELF) {
            if (ef & FG_EF_NAME_ESC) {
                d.mode = json_mode();
                uint32_t n = 0, first = 0x100u;
                for_each_decoded(rd, nm.off, nm.len, d.mode, [&](uint32_t c) {
                    if (n == 0) first = c;
                    ++n;
                });
                d.skip = first == '_' ? 1u : 0u;
                d.dlen = n - d.skip;
            } else if (nm.len && rd.byte(nm.off) == '_') {
                d.skip = 1;
                d.dlen = nm.len - 1u;
            }
        } else if (cfg.src_fmt == FG_CAPNP) {  // the same rule (capnp_splitter.rs:80-87); spans are never escaped
            if (nm.len && rd.byte(nm.off) == '_') {
                d.skip = 1;
                d.dlen = nm.len - 1u;
            } else if (ef & FG_EF_NAME_VERBATIM) {
                d.pfx = 0u;
            }
        }
        const uint32_t si = ty - FG_T_BOOL;
        // (mask-and-or, each term ONE field: `c ? field_a : field_b` is folded into a load through a selected pointer before
        //  this function is inlined into the kernel -- which is the dynamically indexed access again)
        const uint32_t m0 = 0u - (uint32_t)(si == 0u), m1 = 0u - (uint32_t)(si == 1u), m2 = 0u - (uint32_t)(si == 2u), m3 = 0u - (uint32_t)(si == 3u);
        const uint32_t sl = (cfg.suf_len0 & m0) | (cfg.suf_len1 & m1) | (cfg.suf_len2 & m2) | (cfg.suf_len3 & m3);
        const uint32_t so = (cfg.suf_off0 & m0) | (cfg.suf_off1 & m1) | (cfg.suf_off2 & m2) | (cfg.suf_off3 & m3);
        if ((ef & FG_EF_SUFFIX) && ty >= FG_T_BOOL && ty <= FG_T_U64 && sl != 0xFFFFFFFFu) {
            d.so = so;
            d.sl = sl;
        }
        return d;
    }
    // streams the key WITHOUT its leading '_' (name after the skip, then the suffix)
    template <class F>
    FGE_HD void dyn_stream(const Dyn& d, F&& f) {
        uint32_t k = 0;
        for_each_decoded(rd, d.off, d.len, d.mode, [&](uint32_t c) {
            if (k++ >= d.skip) f(c);
        });
        for (uint32_t i = 0; i < d.sl; ++i) f((uint32_t)cfg.blob[d.so + i]);
    }
    // byte k of the key WITHOUT its leading '_' (k < dlen + sl); escaped names (rare) decode from the start
    FGE_HD uint32_t dyn_byte(const Dyn& d, uint32_t k) {
        if (k >= d.dlen) return cfg.blob[d.so + (k - d.dlen)];
        if (d.mode == M_RAW) return rd.byte(d.off + d.skip + k);
        uint32_t i = 0, r = 0;
        const uint32_t want = k + d.skip;
        for_each_decoded(rd, d.off, d.len, d.mode, [&](uint32_t c) {
            if (i++ == want) r = c;
        });
        return r;
    }
    // a pair's value as `{}` prints it (impl Display for SDValue's payload; Null prints nothing)
    template <class F>
    FGE_HD void value_display(uint32_t e, F&& f) {
        const uint32_t ty = t.ent_type[e];
        const uint64_t v = t.ent_val[e];
        FnSinkT<F> fs{f};
        if (ty == FG_T_STRING) {
            for_each_decoded(rd, (uint32_t)v, (uint32_t)(v >> 32), value_mode(e), f);
        } else if (ty == FG_T_BOOL) {
            const char* s = v ? "true" : "false";
            for (uint32_t i = 0; s[i]; ++i) f((uint32_t)(uint8_t)s[i]);
        } else if (ty == FG_T_F64) {
            double d;
            memcpy(&d, &v, 8);
            shortest::display_f64(d, fs);
        } else if (ty == FG_T_I64 || ty == FG_T_U64) {
            uint64_t m = v;
            if (ty == FG_T_I64 && (int64_t)v < 0) {
                f((uint32_t)'-');
                m = 0ull - v;
            }
            u64_digits(m, f);
        }
    }
    // every StructuredData of the record through `impl Display` (record.rs:42-67), concatenated
    FGE_HD void sd_display() {
        const uint32_t first = this->row_ef, cnt = this->row_ec;
        bool open = false;
        for (uint32_t e = first; e < first + cnt; ++e) {
            if (t.ent_type[e] == FG_T_SDID) {
                if (open) out.put(']');
                out.put('[');
                open = true;
                const fg_span id = t.ent_name[e];
                if (id.len != FG_NONE)  // (FG_CAPNP: sd_id None prints as "")
                    for (uint32_t i = 0; i < id.len; ++i) out.put(rd.byte(id.off + i));
                continue;
            }
            if (!open) {  // LTSV / GELF records: one element, sd_id None
                out.put('[');
                open = true;
            }
            out.put(' ');
            const Dyn d = dyn_of(e);
            dyn_stream(d, [&](uint32_t c) { out.put(c); });
            if (t.ent_type[e] != FG_T_NULL) {
                out.put('=');
                out.put('"');
                if (t.ent_type[e] == FG_T_STRING && value_mode(e) == M_RAW) {
                    const uint64_t v = t.ent_val[e];
                    copy_raw<ESC_NONE>((uint32_t)v, (uint32_t)(v >> 32), [&](uint32_t c) { out.put(c); });
                } else {
                    value_display(e, [&](uint32_t c) { out.put(c); });
                }
                out.put('"');
            }
        }
        if (open) out.put(']');
    }
    FGE_HD bool has_sd() const { return this->row_ec != 0; }
    FGE_HD bool some(int col) const { return this->span(col).len != FG_NONE; }
};

// =================================================================================================
// GELF
// =================================================================================================
constexpr uint32_t kSortSlots = 32;

template <class S, class R>
struct GelfEmitter : Base<S, R> {
    using B = Base<S, R>;
    using typename B::Dyn;
    using B::cfg;
    using B::li;
    using B::meta;
    using B::out;
    using B::rd;
    using B::t;
    bool first_member = true;

    FGE_HD GelfEmitter(S& o, const EncCfg& c, R r, const DevTables& tb, uint64_t l, uint32_t m, const RowRegs* pre) : B{o, c, r, tb, l, m} { this->load_row(pre); }

    FGE_HD void esc_byte(uint32_t c) {  // serde_json 0.8 escape_str; one or two put_word sites (code size)
        uint32_t w = c, nb = 1u;
        if (c == '"' || c == '\\') {
            w = (uint32_t)'\\' | c << 8;
            nb = 2u;
        } else if (c < 0x20u) {
            const uint32_t x = c == 8u ? 'b' : c == 9u ? 't' : c == 10u ? 'n' : c == 12u ? 'f' : c == 13u ? 'r' : 0u;
            if (x) {
                w = (uint32_t)'\\' | x << 8;
            } else {  // \u00XX
                out.put_word((uint32_t)'\\' | (uint32_t)'u' << 8 | (uint32_t)'0' << 16 | (uint32_t)'0' << 24, 4u);
                const uint32_t lo = c & 15u;
                w = (c >> 4 ? (uint32_t)'1' : (uint32_t)'0') | (lo < 10u ? '0' + lo : 'a' + lo - 10u) << 8;
            }
            nb = 2u;
        }
        out.put_word(w, nb);
    }
    FGE_HD void member_start() {  // (the object's '{' comes with its first member)
        out.put(first_member ? (uint32_t)'{' : (uint32_t)',');
        first_member = false;
    }
    FGE_HD void key_static(const StaticKey& k) {  // `,"key":` / `{"key":` (StaticKey: with everything behind it that is constant)
        this->blob(first_member ? k.text1_off : k.text_off, k.text_len);
        first_member = false;
    }
    FGE_HD void str_span(uint32_t off, uint32_t len, uint32_t mode, bool open_quote = true) {
        if (open_quote) out.put('"');
        if (mode == M_RAW) {  // (the closing quote rides on the span's last piece)
            this->template copy_raw<ESC_JSON>(off, len, [&](uint32_t c) { esc_byte(c); }, (uint32_t)'"');
            return;
        }
        for_each_decoded(rd, off, len, mode, [&](uint32_t c) { esc_byte(c); });
        out.put('"');
    }
    FGE_HD void str_field(int col) {  // (a static key's value: the key's text ends in the opening quote)
        const fg_span s = this->span(col);
        str_span(s.off, s.len, this->field_mode(col), false);
    }
    FGE_HD void f64_text(double d) {
        uint64_t b;
        memcpy(&b, &d, 8);
        if (((b >> 52) & 0x7FFu) == 0x7FFu) {  // NaN / inf
            this->lit("null", 4);
            return;
        }
        dtoa::write_pieces(d, out);  // digits in registers, as one piece or two where the shape allows (no char buffer: that would be scratch memory)
    }
    // the FULL key (with its '_' where it has one): only FG_CAPNP rows hold keys without
    FGE_HD uint32_t fk_len(const Dyn& d) const { return d.pfx + d.dlen + d.sl; }
    FGE_HD uint32_t fk_byte(const Dyn& d, uint32_t k) { return (d.pfx && k == 0u) ? (uint32_t)'_' : this->dyn_byte(d, k - d.pfx); }
    FGE_HD int cmp_full(const Dyn& a, const Dyn& b) {
        const uint32_t la = fk_len(a), lb = fk_len(b), n = la < lb ? la : lb;
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t x = fk_byte(a, k), y = fk_byte(b, k);
            if (x != y) return x < y ? -1 : 1;
        }
        return la == lb ? 0 : (la < lb ? -1 : 1);
    }
    FGE_HD int cmp_dyn(const Dyn& a, const Dyn& b) {
        if (!(a.pfx & b.pfx)) return cmp_full(a, b);
        const uint32_t la = a.dlen + a.sl, lb = b.dlen + b.sl, n = la < lb ? la : lb;
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t x = this->dyn_byte(a, k), y = this->dyn_byte(b, k);
            if (x != y) return x < y ? -1 : 1;
        }
        return la == lb ? 0 : (la < lb ? -1 : 1);
    }
    // full key ('_' + ...) against a static key
    FGE_HD int cmp_dyn_static(const Dyn& a, const StaticKey& s) {
        if (s.key_len == 0) return 1;
        if (!a.pfx) {  // a key without '_': byte by byte
            const uint32_t la = fk_len(a), lb = s.key_len, n = la < lb ? la : lb;
            for (uint32_t k = 0; k < n; ++k) {
                const uint32_t x = this->dyn_byte(a, k), y = cfg.blob[s.key_off + k];
                if (x != y) return x < y ? -1 : 1;
            }
            return la == lb ? 0 : (la < lb ? -1 : 1);
        }
        const uint32_t s0 = cfg.blob[s.key_off];
        if (s0 != '_') return '_' < s0 ? -1 : 1;
        const uint32_t la = a.dlen + a.sl, lb = s.key_len - 1u, n = la < lb ? la : lb;
        for (uint32_t k = 0; k < n; ++k) {
            const uint32_t x = this->dyn_byte(a, k), y = cfg.blob[s.key_off + 1u + k];
            if (x != y) return x < y ? -1 : 1;
        }
        return la == lb ? 0 : (la < lb ? -1 : 1);
    }
    FGE_HD void emit_dyn(uint32_t e) {
        const Dyn d = this->dyn_of(e);
        member_start();
        out.put('"');
        if (d.pfx) out.put('_');
        this->dyn_stream(d, [&](uint32_t c) { esc_byte(c); });
        out.put('"');
        out.put(':');
        const uint32_t ty = t.ent_type[e];
        const uint64_t v = t.ent_val[e];
        if (ty == FG_T_STRING) {
            str_span((uint32_t)v, (uint32_t)(v >> 32), this->value_mode(e));
        } else if (ty == FG_T_BOOL) {
            if (v) this->lit("true", 4);
            else this->lit("false", 5);
        } else if (ty == FG_T_NULL) {
            this->lit("null", 4);
        } else if (ty == FG_T_U64) {
            this->u64_text(v);
        } else if (ty == FG_T_I64) {
            this->i64_text((int64_t)v);
        } else {
            double d2;
            memcpy(&d2, &v, 8);
            f64_text(d2);
        }
    }
    FGE_HD void emit_static(const StaticKey& k, uint32_t sdid_entry) {
        switch (k.kind) {
            case SK_APP: if (!this->some(S_APP)) return; break;
            case SK_FULL: if (!this->some(S_FULL)) return; break;
            case SK_PROC: if (!this->some(S_PROC)) return; break;
            case SK_LEVEL: if (FG_META_SEVERITY(meta) == 0xFFu) return; break;
            case SK_SDID: if (sdid_entry == 0xFFFFFFFFu || t.ent_name[sdid_entry].len == FG_NONE) return; break;
            default: break;
        }
        key_static(k);
        int col = -1;  // a string field: ONE str_field call site below
        switch (k.kind) {
            case SK_APP: col = S_APP; break;
            case SK_FULL: col = S_FULL; break;
            case SK_PROC: col = S_PROC; break;
            case SK_HOST: {
                const fg_span s = this->span(S_HOST);
                if (s.len == 0u || s.len == FG_NONE) {
                    this->lit("unknown\"", 8);
                } else {
                    col = S_HOST;
                }
                break;
            }
            case SK_LEVEL: out.put('0' + FG_META_SEVERITY(meta)); break;
            case SK_SDID: {
                const fg_span id = t.ent_name[sdid_entry];
                for (uint32_t i = 0; i < id.len; ++i) esc_byte(rd.byte(id.off + i));
                out.put('"');
                break;
            }
            case SK_SHORT: {
                if (!this->some(S_MSG)) {
                    out.put('-');
                    out.put('"');
                } else {
                    col = S_MSG;
                }
                break;
            }
            case SK_TS: f64_text(this->record_ts()); break;
            default: break;  // SK_VERSION, SK_EXTRA: the value is part of the precomputed member text
        }
        if (col >= 0) str_field(col);
    }

    // keys64 / slot_ent / order: this lane's scratch (kSortSlots each)
    FGE_HD uint32_t run(uint64_t* keys64, uint8_t* slot_ent, uint8_t* order) {
        const uint32_t first = this->row_ef, cnt = this->row_ec;
        // pairs -> slots (and the LAST sd_id: every element's insert replaces the previous one)
        uint32_t sdid_entry = 0xFFFFFFFFu, np = 0;
        bool ranked = cnt <= 255u;
        for (uint32_t e = first; e < first + cnt; ++e) {
            if (t.ent_type[e] == FG_T_SDID) {
                sdid_entry = e;
                continue;
            }
            if (np < cfg.sort_slots && ranked) {
                const Dyn d = this->dyn_of(e);
                uint64_t pre = 0;
                if (cfg.src_fmt == FG_CAPNP) {  // (keys with and without '_' in one row: the prefix of the FULL key)
                    for (uint32_t k = 0; k < 7u; ++k) pre = (pre << 8) | (k < fk_len(d) ? fk_byte(d, k) : 0u);
                } else {
                    for (uint32_t k = 0; k < 7u; ++k) pre = (pre << 8) | (k < d.dlen + d.sl ? this->dyn_byte(d, k) : 0u);
                }
                keys64[np] = (pre << 8) | np;  // 7 key bytes big-endian, then the slot: equal keys keep insertion order
                slot_ent[np] = (uint8_t)(e - first);
            } else {
                ranked = false;
            }
            ++np;
        }
        if (ranked) {
            uint64_t k[kSortSlots];
#pragma unroll
            for (uint32_t j = 0; j < kSortSlots; ++j) k[j] = j < np ? keys64[j] : ~0ull;
            for (uint32_t i = 0; i < np; ++i) {  // (k[] stays in registers: only the inner loop is unrolled)
                const uint64_t ki = keys64[i];
                uint32_t rank = 0;
#pragma unroll
                for (uint32_t j = 0; j < kSortSlots; ++j) rank += k[j] < ki ? 1u : 0u;
                order[rank] = (uint8_t)i;
            }
            // adjacent equal 7-byte prefixes: duplicates (keep the later insert) or an unresolved order
            for (uint32_t r = 0; r + 1u < np && ranked; ++r) {
                const uint32_t sa = order[r], sb = order[r + 1u];
                if ((keys64[sa] >> 8) != (keys64[sb] >> 8)) continue;
                const int c = cmp_dyn(this->dyn_of(first + slot_ent[sa]), this->dyn_of(first + slot_ent[sb]));
                if (c == 0) order[r] = 0xFFu;
                else ranked = false;  // two different names share 7 bytes: exact selection below
            }
        }
        // ONE member loop for both orders (one emit_static / emit_dyn call site each: code size): the next entry in
        // key order comes from the ranking or, when that is not available, from an exact selection -- repeatedly the
        // smallest key greater than the previous one, among equal keys the LAST entry (the later insert)
        const uint32_t kNone = 0xFFFFFFFFu;
        uint32_t sk = 0;  // next static key
        uint32_t r = 0, prev = kNone;
        for (;;) {
            uint32_t e = kNone;
            if (ranked) {
                while (r < np && order[r] == 0xFFu) ++r;
                if (r < np) e = first + slot_ent[order[r++]];
            } else {
                for (uint32_t c = first; c < first + cnt; ++c) {
                    if (t.ent_type[c] == FG_T_SDID) continue;
                    const Dyn dc = this->dyn_of(c);
                    if (prev != kNone && cmp_dyn(dc, this->dyn_of(prev)) <= 0) continue;
                    if (e == kNone || cmp_dyn(dc, this->dyn_of(e)) <= 0) e = c;
                }
                prev = e;
            }
            // the static keys that sort before the entry (an equal one replaces it: gelf_extra is inserted last);
            // all the remaining ones once the entries are exhausted
            Dyn d{};
            if (e != kNone) d = this->dyn_of(e);
            bool shadowed = false;
            while (sk < cfg.n_keys) {
                if (e != kNone) {
                    const int c = cmp_dyn_static(d, cfg.keys[sk]);
                    if (c < 0) break;
                    if (c == 0) {
                        // gelf_extra is inserted last and replaces the pair; a fixed member ("host", "sd_id" ...) is inserted FIRST, so a
                        // pair of that name -- only an FG_CAPNP extra can have one -- replaces IT (gelf_encoder.rs:60-110)
                        if (cfg.keys[sk].kind == SK_EXTRA) {
                            shadowed = true;
                        } else {
                            ++sk;
                            continue;
                        }
                    }
                }
                emit_static(cfg.keys[sk], sdid_entry);
                ++sk;
            }
            if (e == kNone) break;
            if (!shadowed) emit_dyn(e);
        }
        if (first_member) out.put('{');  // (no member at all)
        out.put('}');
        return ES_OK;
    }
};

// =================================================================================================
// LTSV
// =================================================================================================
template <class S, class R>
struct LtsvEmitter : Base<S, R> {
    using B = Base<S, R>;
    using B::cfg;
    using B::li;
    using B::meta;
    using B::out;
    using B::rd;
    using B::t;
    bool first = true;
    FGE_HD LtsvEmitter(S& o, const EncCfg& c, R r, const DevTables& tb, uint64_t l, uint32_t m, const RowRegs* pre) : B{o, c, r, tb, l, m} { this->load_row(pre); }

    FGE_HD void key_byte(uint32_t c) { out.put(c == '\n' || c == '\t' ? (uint32_t)' ' : c == ':' ? (uint32_t)'_' : c); }
    FGE_HD void val_byte(uint32_t c) { out.put(c == '\n' || c == '\t' ? (uint32_t)' ' : c); }
    // LTSVString::insert up to and including ':' -- `key` includes its ':' -- behind the TAB of every entry but the first: one piece
    FGE_HD void start(const char* key, uint32_t n) {
        this->lit(key, n, first ? 0u : (uint32_t)'\t');
        first = false;
    }
    FGE_HD void val_span(uint32_t off, uint32_t len, uint32_t mode) {
        if (mode == M_RAW) this->template copy_raw<ESC_LTSV_VAL>(off, len, [&](uint32_t c) { val_byte(c); });
        else for_each_decoded(rd, off, len, mode, [&](uint32_t c) { val_byte(c); });
    }
    FGE_HD void field(const char* key, uint32_t n, int col) {
        start(key, n);
        const fg_span s = this->span(col);
        val_span(s.off, s.len, this->field_mode(col));
    }
    FGE_HD uint32_t run() {
        const uint32_t ef = this->row_ef, cnt = this->row_ec;
        for (uint32_t e = ef; e < ef + cnt; ++e) {
            if (t.ent_type[e] == FG_T_SDID) continue;
            if (!first) out.put('\t');
            first = false;
            const typename B::Dyn d = this->dyn_of(e);
            this->dyn_stream(d, [&](uint32_t c) { key_byte(c); });
            out.put(':');
            if (t.ent_type[e] == FG_T_STRING) {
                const uint64_t v = t.ent_val[e];
                val_span((uint32_t)v, (uint32_t)(v >> 32), this->value_mode(e));
            } else {
                this->value_display(e, [&](uint32_t c) { val_byte(c); });
            }
        }
        if (cfg.ltsv_extra_len) {
            if (!first) out.put('\t');
            first = false;
            this->blob(cfg.ltsv_extra_off, cfg.ltsv_extra_len);
        }
        start("host:", 5);
        if (this->some(S_HOST)) {
            const fg_span s = this->span(S_HOST);
            val_span(s.off, s.len, this->field_mode(S_HOST));
        }
        start("time:", 5);
        shortest::display_f64(this->record_ts(), out);
        if (this->some(S_MSG)) field("message:", 8, S_MSG);
        if (this->some(S_FULL)) field("full_message:", 13, S_FULL);
        if (FG_META_SEVERITY(meta) != 0xFFu) {
            start("level:", 6);
            this->u64_text(FG_META_SEVERITY(meta));
        }
        if (FG_META_FACILITY(meta) != 0xFFu) {
            start("facility:", 9);
            this->u64_text(FG_META_FACILITY(meta));
        }
        if (this->some(S_APP)) field("appname:", 8, S_APP);
        if (this->some(S_PROC)) field("procid:", 7, S_PROC);
        if (this->some(S_MSGID)) field("msgid:", 6, S_MSGID);
        return ES_OK;
    }
};

// =================================================================================================
// RFC5424 / RFC3164 / passthrough
// =================================================================================================
constexpr int64_t kMinUnix = -377705116800ll, kMaxUnix = 253402300799ll;  // time 0.3: years -9999 ..= 9999

// ((ts * 1000.0) as i128) * 1_000_000 (release build: saturating cast, wrapping multiplication), then
// OffsetDateTime::from_unix_timestamp_nanos: false = out of range ("Failed to parse date").
FGE_HD bool rfc5424_ts_split(double ts, int64_t* secs, uint32_t* nanos) {
    const double x = ts * 1000.0;
    // i128 two's complement as (hi, lo)
    uint64_t hi, lo;
    if (x != x) {
        hi = lo = 0;
    } else if (x >= 170141183460469231731687303715884105728.0) {
        hi = 0x7FFFFFFFFFFFFFFFull;
        lo = ~0ull;
    } else if (x <= -170141183460469231731687303715884105728.0) {
        hi = 0x8000000000000000ull;
        lo = 0;
    } else {
        const double a = x < 0 ? -x : x;
        uint64_t mh, ml;
        if (a < 18446744073709551616.0) {
            mh = 0;
            ml = (uint64_t)a;  // truncates
        } else {  // an integer m * 2^e with e >= 12
            uint64_t b;
            memcpy(&b, &a, 8);
            const uint64_t m = (b & 0x000FFFFFFFFFFFFFull) | 0x0010000000000000ull;
            const int sh = (int)((b >> 52) & 0x7FFu) - 1075;  // 12 .. 74
            if (sh >= 64) {
                mh = m << (sh - 64);
                ml = 0;
            } else {
                mh = m >> (64 - sh);
                ml = m << sh;
            }
        }
        if (x < 0) {  // negate
            ml = ~ml + 1u;
            mh = ~mh + (ml == 0 ? 1u : 0u);
        }
        hi = mh;
        lo = ml;
    }
    // * 1_000_000 mod 2^128
    uint64_t ph, pl;
    shortest::mul64(lo, 1000000u, &ph, &pl);
    const uint64_t rh = ph + hi * 1000000u, rl = pl;
    // the valid range needs |ns| < 2^79: hi must be a sign extension with small magnitude
    const bool neg = (rh >> 63) != 0;
    uint64_t ah = rh, al = rl;
    if (neg) {
        al = ~al + 1u;
        ah = ~ah + (al == 0 ? 1u : 0u);
    }
    if (ah >= (1ull << 20)) return false;  // |ns| >= 2^84: far outside
    // |ns| = ah * 2^64 + al with ah < 2^20  ->  seconds and nanoseconds: long division by 10^9 in two 32-bit steps
    const uint64_t d = 1000000000ull;
    const uint64_t c1 = (ah << 32) | (al >> 32);  // < 2^52
    const uint64_t qh = c1 / d;                   // < 2^23
    const uint64_t c0 = ((c1 % d) << 32) | (al & 0xFFFFFFFFull);  // < 10^9 * 2^32
    const uint64_t q = (qh << 32) + c0 / d;       // c0 / d < 2^32
    const uint64_t rem = c0 % d;
    int64_t s = (int64_t)q;
    uint32_t ns = (uint32_t)rem;
    if (neg) {
        s = -s;
        if (ns) {
            s -= 1;
            ns = 1000000000u - ns;
        }
    }
    if (s < kMinUnix || s > kMaxUnix) return false;
    *secs = s;
    *nanos = ns;
    return true;
}
FGE_HD int64_t f64_as_i64(double x) {  // Rust `as i64`: truncating, saturating, NaN -> 0
    if (x != x) return 0;
    if (x >= 9223372036854775808.0) return INT64_MAX;
    if (x <= -9223372036854775808.0) return INT64_MIN;
    return (int64_t)x;
}
struct Civil {
    int y, m, d;
    uint32_t hh, mm, ss;
};
FGE_HD Civil civil_of(int64_t secs) {
    const int64_t days = secs >= 0 ? secs / 86400 : -((-secs + 86399) / 86400);
    const uint32_t sod = (uint32_t)(secs - days * 86400);
    Civil c;
    civil_from_days(days, &c.y, &c.m, &c.d);
    c.hh = sod / 3600u;
    c.mm = sod / 60u % 60u;
    c.ss = sod % 60u;
    return c;
}

template <class S, class R>
struct Rfc5424Emitter : Base<S, R> {
    using B = Base<S, R>;
    using B::li;
    using B::meta;
    using B::out;
    using B::t;
    FGE_HD Rfc5424Emitter(S& o, const EncCfg& c, R r, const DevTables& tb, uint64_t l, uint32_t m, const RowRegs* pre) : B{o, c, r, tb, l, m} { this->load_row(pre); }
    FGE_HD uint32_t run() {
        int64_t secs;
        uint32_t nanos;
        if (!rfc5424_ts_split(this->record_ts(), &secs, &nanos)) return ES_5424_DATE;
        const Civil c = civil_of(secs);
        if (c.y < 0 || c.y > 9999) return ES_5424_FORMAT;
        if (this->has_pri()) this->pri();
        else this->lit("<13>", 4);
        // "1 YYYY-MM-DDTHH:" (sixteen bytes) + "MM:SS" [+ "." + the nanoseconds without trailing zeros: time 0.3 Rfc3339] + "Z ": three
        // pieces (two without a fraction) instead of ~thirty one-byte puts
        {
            const uint32_t yh = B::d2((uint32_t)c.y / 100u), yl = B::d2((uint32_t)c.y % 100u), mo = B::d2((uint32_t)c.m), dd = B::d2((uint32_t)c.d);
            const uint32_t hh = B::d2(c.hh), mi = B::d2(c.mm), ss = B::d2(c.ss);
            out.put16((uint32_t)'1' | (uint32_t)' ' << 8 | yh << 16, yl | (uint32_t)'-' << 16 | (mo & 0xFFu) << 24,
                      (mo >> 8) | (uint32_t)'-' << 8 | dd << 16, (uint32_t)'T' | hh << 8 | (uint32_t)':' << 24);
            const uint32_t t0 = mi | (uint32_t)':' << 16 | (ss & 0xFFu) << 24, t1 = ss >> 8;  // "MM:SS"
            if (!nanos) {
                out.put_part(t0, t1 | (uint32_t)'Z' << 8 | (uint32_t)' ' << 16, 0u, 0u, 7u);
            } else {
                out.put_part(t0, t1, 0u, 0u, 5u);
                uint32_t digs = 9, v = nanos;
                while (v % 10u == 0) {
                    v /= 10u;
                    --digs;
                }
                // '.' + nine digits, cut behind `digs` of them, "Z " behind the cut
                const uint32_t lo8 = dtoa::Bcd17::bcd8(nanos % 100000000u);
                uint32_t q[4] = {(uint32_t)'.' | ((uint32_t)'0' + nanos / 100000000u) << 8, 0u, 0u, 0u};
                const uint32_t a = dtoa::ascii4(lo8 >> 16), b = dtoa::ascii4(lo8 & 0xFFFFu);  // digits 2..5, 6..9
                q[0] |= a << 16;
                q[1] = a >> 16 | b << 16;
                q[2] = b >> 16;
                B::keep_low(q, 1u + digs);
                B::set_byte(q, 1u + digs, (uint32_t)'Z');
                B::set_byte(q, 2u + digs, (uint32_t)' ');
                out.put_part(q[0], q[1], q[2], q[3], 3u + digs);
            }
        }
        if (this->some(S_HOST)) this->raw_field(S_HOST, (uint32_t)' ');
        else out.put(' ');
        if (this->some(S_APP)) this->raw_field(S_APP, (uint32_t)' ');
        if (this->some(S_PROC)) this->raw_field(S_PROC, (uint32_t)' ');
        else this->lit("- ", 2);
        if (this->some(S_MSGID)) this->raw_field(S_MSGID, (uint32_t)' ');
        else this->lit("- ", 2);
        if (this->has_sd()) {
            this->sd_display();
            out.put(' ');
        } else {
            this->lit("- ", 2);
        }
        if (this->some(S_MSG)) this->raw_field(S_MSG);
        return ES_OK;
    }
};

template <class S, class R>
struct Rfc3164Emitter : Base<S, R> {
    using B = Base<S, R>;
    using B::cfg;
    using B::out;
    FGE_HD Rfc3164Emitter(S& o, const EncCfg& c, R r, const DevTables& tb, uint64_t l, uint32_t m, const RowRegs* pre) : B{o, c, r, tb, l, m} { this->load_row(pre); }
    FGE_HD uint32_t run() {
        const int64_t secs = f64_as_i64(this->record_ts());
        if (secs < kMinUnix || secs > kMaxUnix) return ES_3164_TS;
        if (cfg.prepend_len != 0xFFFFFFFFu) this->blob(cfg.prepend_off, cfg.prepend_len);
        if (this->has_pri()) this->pri();
        const Civil c = civil_of(secs);
        // "[month repr:short]  [day padding:none] [hour]:[minute]:[second] "
        const char* mon = "JanFebMarAprMayJunJulAugSepOctNovDec" + 3 * (c.m - 1);
        {   // "Mon  " (two spaces) + the day without padding + " ", then "hh:mm:ss ": two pieces
            const uint32_t day = (uint32_t)c.d, nd = day >= 10u ? 2u : 1u;
            const uint32_t m4 = (uint32_t)(uint8_t)mon[0] | (uint32_t)(uint8_t)mon[1] << 8 | (uint32_t)(uint8_t)mon[2] << 16 | (uint32_t)' ' << 24;
            out.put_part(m4, nd == 2u ? ((uint32_t)' ' | B::d2(day) << 8 | (uint32_t)' ' << 24) : ((uint32_t)' ' | ((uint32_t)'0' + day) << 8 | (uint32_t)' ' << 16),
                         0u, 0u, 6u + nd);
            const uint32_t hh = B::d2(c.hh), mi = B::d2(c.mm), ss = B::d2(c.ss);
            out.put_part(hh | (uint32_t)':' << 16 | (mi & 0xFFu) << 24, (mi >> 8) | (uint32_t)':' << 8 | ss << 16, (uint32_t)' ', 0u, 9u);
        }
        if (this->some(S_HOST)) this->raw_field(S_HOST, (uint32_t)' ');
        else out.put(' ');
        if (this->some(S_APP)) this->raw_field(S_APP);
        if (this->some(S_PROC)) {
            out.put('[');
            this->raw_field(S_PROC, (uint32_t)']');
            this->lit(": ", 2);
        }
        if (this->some(S_MSGID)) this->raw_field(S_MSGID, (uint32_t)' ');
        if (this->has_sd()) {
            this->sd_display();
            out.put(' ');
        }
        if (this->some(S_MSG)) this->raw_field(S_MSG);
        return ES_OK;
    }
};

template <class S, class R>
struct PassthroughEmitter : Base<S, R> {
    using B = Base<S, R>;
    using B::cfg;
    FGE_HD PassthroughEmitter(S& o, const EncCfg& c, R r, const DevTables& tb, uint64_t l, uint32_t m, const RowRegs* pre) : B{o, c, r, tb, l, m} { this->load_row(pre); }
    FGE_HD uint32_t run() {
        if (!this->some(S_FULL)) return ES_PASSTHROUGH_EMPTY;
        if (cfg.prepend_len != 0xFFFFFFFFu) this->blob(cfg.prepend_off, cfg.prepend_len);
        this->raw_field(S_FULL);
        return ES_OK;
    }
};

// =================================================================================================
// Cap'n Proto (encoder/capnp_encoder.rs: build_record + capnp::serialize::write_message, schema record.capnp)
// =================================================================================================
// A message is the segment table, then the segments.  Segment 0 starts with the root pointer and the Record struct (2 data words,
// 9 pointers: words 0 .. 11); every text / list the builder allocates follows in allocation order.  Texts are the DECODED bytes, a
// NUL and zero padding to a whole word.  Pointers are relative, so the output.capnp_extra list -- tag, pair structs, texts -- is
// the same byte image for every row: fg_enc_cfg.hpp builds it once (cfg.ltsv_extra_off / _len carry it for this encoder).
// A row whose objects exceed the first segment's 1024 words takes capnp_multi (out of line): the allocator of capnp 0.14, far
// pointers and landing pads included (the rules are not pinned by a reference vector).
constexpr uint32_t kCapnpSeg0Words = 1024;  // capnp::message::SUGGESTED_FIRST_SEGMENT_WORDS
constexpr uint32_t kCapnpMaxSegs = 32;      // segment k > 0 holds >= 1024 * 2^k words (GrowHeuristically): never reached
constexpr uint32_t kCapnpNone = 0xFFFFFFFFu;

// where an object landed: its first word (far: its landing pad is the word before it)
struct CapnpPlace {
    uint32_t seg, pos, far;
};
// message::HeapAllocator + private/arena.rs BuilderArenaImpl: an object is tried in the segment that holds its pointer (`home`),
// else it takes one more word (the landing pad) in the first segment with room, else in a new segment of max(that, next_size)
struct CapnpArena {
    uint32_t cap[kCapnpMaxSegs], used[kCapnpMaxSegs];
    uint32_t nseg;
    uint64_t next;
    FGE_HD void init() {  // segment 0 (allocate_segment: next_size 1024 -> 2048), the root pointer and the Record struct
        nseg = 1;
        cap[0] = kCapnpSeg0Words;
        used[0] = 12u;
        next = 2u * kCapnpSeg0Words;
    }
    FGE_HD CapnpPlace alloc(uint32_t home, uint32_t a) {
        if (cap[home] - used[home] >= a) {
            const CapnpPlace p{home, used[home], 0u};
            used[home] += a;
            return p;
        }
        for (uint32_t s = 0; s < nseg; ++s) {
            if (cap[s] - used[s] >= a + 1u) {
                const CapnpPlace p{s, used[s] + 1u, 1u};
                used[s] += a + 1u;
                return p;
            }
        }
        const uint32_t s = nseg < kCapnpMaxSegs ? nseg++ : kCapnpMaxSegs - 1u;
        const uint64_t c = (uint64_t)a + 1u > next ? (uint64_t)a + 1u : next;
        next += c;
        cap[s] = (uint32_t)c;
        used[s] = a + 1u;
        return CapnpPlace{s, 1u, 1u};
    }
};

template <class S, class R>
struct CapnpEmitter;
// the multi-segment form: its own function, everything by value (as encode_lane_global in fg_encode.hip) -- the arena is a
// dynamically indexed array, i.e. scratch memory, and must not reach the single-segment path
template <class S, class R>
#if defined(__HIPCC__)
__host__ __device__ __attribute__((noinline))
#else
inline
#endif
S capnp_multi(S sink, EncCfg cfg, R rd, DevTables t, uint64_t li, uint32_t meta, RowRegs row) {
    CapnpEmitter<S, R> em(sink, cfg, rd, t, li, meta, &row);
    em.run_multi();
    return sink;
}

template <class S, class R>
struct CapnpEmitter : Base<S, R> {
    using B = Base<S, R>;
    using typename B::Dyn;
    using B::cfg;
    using B::li;
    using B::meta;
    using B::out;
    using B::rd;
    using B::t;
    uint32_t plo = 0, phi = 0;  // a word waiting for its partner: pointer and struct words go out two at a time
    bool pend = false;
    FGE_HD CapnpEmitter(S& o, const EncCfg& c, R r, const DevTables& tb, uint64_t l, uint32_t m, const RowRegs* pre) : B{o, c, r, tb, l, m} { this->load_row(pre); }

    static FGE_HD uint32_t tw(uint32_t len) { return (len + 8u) >> 3; }                 // words of a text: bytes + NUL, padded
    static FGE_HD uint32_t text_hi(uint32_t len) { return 2u | (len + 1u) << 3; }       // list pointer, element size byte
    static FGE_HD uint32_t list_hi(uint32_t n) { return 7u | (4u * n) << 3; }           // list pointer, inline composite: 4 words a pair
    static FGE_HD uint32_t near_lo(uint32_t ptr_word, uint32_t target) { return 1u | (target - ptr_word - 1u) << 2; }

    FGE_HD void word(uint32_t lo, uint32_t hi) {
        if (pend) {
            out.put16(plo, phi, lo, hi);
            pend = false;
        } else {
            plo = lo;
            phi = hi;
            pend = true;
        }
    }
    FGE_HD void flush() {
        if (pend) out.put_part(plo, phi, 0u, 0u, 8u);
        pend = false;
    }
    // ---- the record's texts and their decoded lengths ----
    FGE_HD uint32_t dec_len(uint32_t off, uint32_t len, uint32_t mode) {
        if (mode == M_RAW) return len;
        uint32_t n = 0;
        for_each_decoded(rd, off, len, mode, [&](uint32_t) { ++n; });
        return n;
    }
    FGE_HD bool field_on(int col) const { return col == S_HOST || this->some(col); }  // Record.hostname is a String: always set
    FGE_HD uint32_t field_len(int col) {
        const fg_span s = this->span(col);
        return s.len == FG_NONE ? 0u : dec_len(s.off, s.len, this->field_mode(col));
    }
    FGE_HD uint32_t key_len(uint32_t e) {  // '_' + name [+ LTSV suffix]
        const Dyn d = this->dyn_of(e);
        return d.pfx + d.dlen + d.sl;
    }
    FGE_HD uint32_t val_len(uint32_t e) {
        const uint64_t v = t.ent_val[e];
        return dec_len((uint32_t)v, (uint32_t)(v >> 32), this->value_mode(e));
    }
    FGE_HD bool is_str(uint32_t e) const { return t.ent_type[e] == FG_T_STRING; }
    // only sd[0] is encoded (capnp_encoder.rs:79-81): its sd_id entry (kCapnpNone: None) and its pairs [lo, hi)
    FGE_HD void sd0(uint32_t& sdid, uint32_t& lo, uint32_t& hi) const {
        const uint32_t end = this->row_ef + this->row_ec;
        uint32_t e = this->row_ef;
        sdid = kCapnpNone;
        if ((cfg.src_fmt == FG_RFC5424 || cfg.src_fmt == FG_CAPNP) && e < end && t.ent_type[e] == FG_T_SDID) {  // (other sources: one element, sd_id None)
            sdid = e++;
            if (t.ent_name[sdid].len == FG_NONE) sdid = kCapnpNone;  // (FG_CAPNP: the element of a message whose sd_id getter failed)
        }
        lo = e;
        while (e < end && t.ent_type[e] != FG_T_SDID) ++e;
        hi = e;
    }
    // output.capnp_extra, prebuilt: dword k of its image
    FGE_HD uint32_t xd(uint32_t k) const { return reinterpret_cast<const uint32_t*>(cfg.blob + cfg.ltsv_extra_off)[k]; }
    FGE_HD uint32_t extra_n() const { return cfg.ltsv_extra_len ? xd(0) >> 2 : 0u; }

    FGE_HD void pad(uint32_t len) { out.put_part(0u, 0u, 0u, 0u, 8u * tw(len) - len); }  // the NUL and the padding: one piece
    FGE_HD void raw_bytes(uint32_t off, uint32_t len) {
        uint32_t i = 0;
        for (; i + 16u <= len; i += 16u) {
            uint32_t q[4];
            rd.load16(off + i, q);
            out.put16(q[0], q[1], q[2], q[3]);
        }
        const uint32_t nb = len - i;
        if (nb) {
            uint32_t q[4];
            rd.load16p(off + i, nb, q);
            B::keep_low(q, nb);
            out.put_part(q[0], q[1], q[2], q[3], nb);
        }
    }
    // a text from the line (dlen: its decoded length): sixteen bytes per piece, the last 0 .. 15 bytes together with the NUL and
    // the padding as ONE piece of 8 or 16 bytes
    FGE_HD void text(uint32_t off, uint32_t len, uint32_t mode, uint32_t dlen) {
        if (mode != M_RAW) {
            for_each_decoded(rd, off, len, mode, [&](uint32_t c) { out.put(c); });
            pad(dlen);
            return;
        }
        uint32_t i = 0;
        for (; i + 16u <= len; i += 16u) {
            uint32_t q[4];
            rd.load16(off + i, q);
            out.put16(q[0], q[1], q[2], q[3]);
        }
        const uint32_t nb = len - i;
        uint32_t q[4] = {0u, 0u, 0u, 0u};
        if (nb) {
            rd.load16p(off + i, nb, q);
            B::keep_low(q, nb);
        }
        out.put_part(q[0], q[1], q[2], q[3], nb < 8u ? 8u : 16u);
    }
    FGE_HD void field_text(int col, uint32_t dlen) {
        const fg_span s = this->span(col);
        if (s.len == FG_NONE) {  // hostname None in the table: "" in the Record
            out.put_part(0u, 0u, 0u, 0u, 8u);
            return;
        }
        text(s.off, s.len, this->field_mode(col), dlen);
    }
    FGE_HD void sdid_text(uint32_t e) {
        const fg_span id = t.ent_name[e];
        text(id.off, id.len, M_RAW, id.len);
    }
    FGE_HD void key_text(uint32_t e) {
        const Dyn d = this->dyn_of(e);
        if (d.pfx) out.put('_');
        if (d.mode == M_RAW) {
            raw_bytes(d.off + d.skip, d.dlen);
            for (uint32_t i = 0; i < d.sl; ++i) out.put((uint32_t)cfg.blob[d.so + i]);
        } else {
            this->dyn_stream(d, [&](uint32_t c) { out.put(c); });
        }
        pad(d.pfx + d.dlen + d.sl);
    }
    FGE_HD void val_text(uint32_t e) {
        const uint64_t v = t.ent_val[e];
        const uint32_t mode = this->value_mode(e);
        text((uint32_t)v, (uint32_t)(v >> 32), mode, mode == M_RAW ? 0u : val_len(e));
    }
    // a Pair struct: data word 0 = the union's discriminant (SDValue order = FG_T_*) [+ the bool at bit 16], data word 1 = the
    // number's bits, pointer 0 = the key, pointer 1 = the string
    FGE_HD void pair_struct(uint32_t e, uint32_t klo, uint32_t khi, uint32_t vlo, uint32_t vhi) {
        const uint32_t ty = t.ent_type[e];
        const uint64_t v = t.ent_val[e];
        const bool num = ty == FG_T_F64 || ty == FG_T_I64 || ty == FG_T_U64;
        word(ty | ((ty == FG_T_BOOL && v != 0u) ? 1u << 16 : 0u), 0u);
        word(num ? (uint32_t)v : 0u, num ? (uint32_t)(v >> 32) : 0u);
        word(klo, khi);
        word(ty == FG_T_STRING ? vlo : 0u, ty == FG_T_STRING ? vhi : 0u);
    }
    FGE_HD void data_words() {
        const double ts = this->record_ts();
        uint64_t b;
        memcpy(&b, &ts, 8);
        word((uint32_t)b, (uint32_t)(b >> 32));
        word((uint32_t)FG_META_FACILITY(meta) | (uint32_t)FG_META_SEVERITY(meta) << 8, 0u);
    }

    FGE_HD uint32_t run() {
        uint32_t sdid, elo, ehi;
        sd0(sdid, elo, ehi);
        const bool sd = this->row_ec != 0u;
        const uint32_t lh = field_len(S_HOST), la = field_len(S_APP), lp = field_len(S_PROC), lm = field_len(S_MSGID), lg = field_len(S_MSG),
                       lf = field_len(S_FULL);
        const uint32_t ls = sdid != kCapnpNone ? t.ent_name[sdid].len : 0u;
        const uint32_t np = ehi - elo;
        uint32_t wt = 0;  // the pairs' texts
        if (sd) {
            for (uint32_t e = elo; e < ehi; ++e) wt += tw(key_len(e)) + (is_str(e) ? tw(val_len(e)) : 0u);
        }
        const uint32_t xn = extra_n();
        // the objects in allocation order, one segment
        uint32_t p = 12u;
        const uint32_t ph = p;
        p += tw(lh);
        const uint32_t pa = p;
        p += this->some(S_APP) ? tw(la) : 0u;
        const uint32_t pp = p;
        p += this->some(S_PROC) ? tw(lp) : 0u;
        const uint32_t pm = p;
        p += this->some(S_MSGID) ? tw(lm) : 0u;
        const uint32_t pg = p;
        p += this->some(S_MSG) ? tw(lg) : 0u;
        const uint32_t pf = p;
        p += this->some(S_FULL) ? tw(lf) : 0u;
        const uint32_t ps = p;
        p += sdid != kCapnpNone ? tw(ls) : 0u;
        const uint32_t pl = p;
        p += sd ? 1u + 4u * np + wt : 0u;
        const uint32_t px = p;
        p += cfg.ltsv_extra_len >> 3;
        if (p > kCapnpSeg0Words) {
            RowRegs rr;
            rr.s0 = this->s0;
            rr.s1 = this->s1;
            rr.s2 = this->s2;
            rr.s3 = this->s3;
            rr.s4 = this->s4;
            rr.s5 = this->s5;
            rr.ts = this->row_ts;
            rr.ef = this->row_ef;
            rr.ec = this->row_ec;
            R r2 = rd;
#if defined(__HIP_DEVICE_COMPILE__)
            // (the reader's pointer made opaque: otherwise the compiler carries "this is the LDS tile" into the out-of-line function
            //  and emits an address-space compare gfx950 cannot encode -- "Illegal instruction detected", V_CMP with src_shared_base)
            uint64_t w = (uint64_t)(uintptr_t)r2.words;
            asm volatile("" : "+v"(w));
            r2.words = reinterpret_cast<const uint32_t*>((uintptr_t)w);
#endif
            out = capnp_multi<S, R>(out, cfg, r2, t, li, meta, rr);
            return ES_OK;
        }
        if (S::kCount) {
            out.add(8u + 8u * p);
            return ES_OK;
        }
        out.put16(0u, p, 0u, 0x00090002u);  // segment table (one segment of p words), root pointer: struct, 2 data words, 9 pointers
        data_words();
        word(near_lo(3u, ph), text_hi(lh));
        if (this->some(S_APP)) word(near_lo(4u, pa), text_hi(la));
        else word(0u, 0u);
        if (this->some(S_PROC)) word(near_lo(5u, pp), text_hi(lp));
        else word(0u, 0u);
        if (this->some(S_MSGID)) word(near_lo(6u, pm), text_hi(lm));
        else word(0u, 0u);
        if (this->some(S_MSG)) word(near_lo(7u, pg), text_hi(lg));
        else word(0u, 0u);
        if (this->some(S_FULL)) word(near_lo(8u, pf), text_hi(lf));
        else word(0u, 0u);
        if (sdid != kCapnpNone) word(near_lo(9u, ps), text_hi(ls));
        else word(0u, 0u);
        if (sd) word(near_lo(10u, pl), list_hi(np));
        else word(0u, 0u);
        if (xn) word(near_lo(11u, px), list_hi(xn));
        else word(0u, 0u);
        flush();
        field_text(S_HOST, lh);
        if (this->some(S_APP)) field_text(S_APP, la);
        if (this->some(S_PROC)) field_text(S_PROC, lp);
        if (this->some(S_MSGID)) field_text(S_MSGID, lm);
        if (this->some(S_MSG)) field_text(S_MSG, lg);
        if (this->some(S_FULL)) field_text(S_FULL, lf);
        if (sdid != kCapnpNone) sdid_text(sdid);
        if (sd) {
            word(np << 2, 2u | 2u << 16);  // the tag: n elements of 2 data words + 2 pointers
            uint32_t q = pl + 1u + 4u * np;  // where the next key / value goes
            for (uint32_t e = elo; e < ehi; ++e) {
                const uint32_t sw = pl + 1u + 4u * (e - elo);
                const uint32_t kl = key_len(e);
                const uint32_t klo = near_lo(sw + 2u, q);
                q += tw(kl);
                uint32_t vlo = 0u, vhi = 0u;
                if (is_str(e)) {
                    const uint32_t vl = val_len(e);
                    vlo = near_lo(sw + 3u, q);
                    vhi = text_hi(vl);
                    q += tw(vl);
                }
                pair_struct(e, klo, text_hi(kl), vlo, vhi);
            }
            flush();
            for (uint32_t e = elo; e < ehi; ++e) {
                key_text(e);
                if (is_str(e)) val_text(e);
            }
        }
        if (xn) this->blob(cfg.ltsv_extra_off, cfg.ltsv_extra_len);
        return ES_OK;
    }

    // ---- the multi-segment form ----
    enum : uint32_t { K_ROOT = 0, K_FIELD = 1, K_SDID = 2, K_PAIRS = 3, K_KEY = 4, K_VAL = 5, K_EXTRA = 6, K_XKEY = 7, K_XVAL = 8 };
    // extra pair i's key (v = 0) or value (v = 1) in the image: its length and its first word there
    FGE_HD uint32_t xtext_len(uint32_t i, uint32_t v) const { return (xd(2u * (3u + 4u * i + v) + 1u) >> 3) - 1u; }
    FGE_HD uint32_t xtext_word(uint32_t i, uint32_t v) const { return 3u + 4u * i + v + 1u + (xd(2u * (3u + 4u * i + v)) >> 2); }
    // the pairs' texts in allocation order (each pair: key, then its string value), from the state right after their list
    template <class F>
    FGE_HD void pair_objs(CapnpArena& ar, uint32_t seg, uint32_t elo, uint32_t ehi, F&& f) {
        for (uint32_t e = elo; e < ehi; ++e) {
            const uint32_t kl = key_len(e);
            const CapnpPlace kp = ar.alloc(seg, tw(kl));
            CapnpPlace vp{0u, 0u, 0u};
            uint32_t vl = 0u;
            if (is_str(e)) {
                vl = val_len(e);
                vp = ar.alloc(seg, tw(vl));
            }
            f(e - elo, e, kp, kl, vp, vl);
        }
    }
    template <class F>
    FGE_HD void extra_objs(CapnpArena& ar, uint32_t seg, uint32_t xn, F&& f) {
        for (uint32_t i = 0; i < xn; ++i) {
            const uint32_t kl = xtext_len(i, 0u), vl = xtext_len(i, 1u);
            const CapnpPlace kp = ar.alloc(seg, tw(kl));
            const CapnpPlace vp = ar.alloc(seg, tw(vl));
            f(i, i, kp, kl, vp, vl);
        }
    }
    // every object of the message in allocation order: f(kind, index, place, length or count, arena after the allocation)
    template <class F>
    FGE_HD void walk(CapnpArena& ar, uint32_t sdid, uint32_t elo, uint32_t ehi, uint32_t xn, F&& f) {
        ar.init();
        f(K_ROOT, 0u, CapnpPlace{0u, 0u, 0u}, 0u, ar);
        for (int col = S_HOST; col <= S_FULL; ++col) {
            if (!field_on(col)) continue;
            const uint32_t l = field_len(col);
            f(K_FIELD, (uint32_t)col, ar.alloc(0u, tw(l)), l, ar);
        }
        if (sdid != kCapnpNone) {
            const uint32_t l = t.ent_name[sdid].len;
            f(K_SDID, sdid, ar.alloc(0u, tw(l)), l, ar);
        }
        if (this->row_ec != 0u) {
            const CapnpPlace lp = ar.alloc(0u, 1u + 4u * (ehi - elo));
            f(K_PAIRS, 0u, lp, ehi - elo, ar);
            pair_objs(ar, lp.seg, elo, ehi, [&](uint32_t, uint32_t e, const CapnpPlace& kp, uint32_t kl, const CapnpPlace& vp, uint32_t vl) {
                f(K_KEY, e, kp, kl, ar);
                if (is_str(e)) f(K_VAL, e, vp, vl, ar);
            });
        }
        if (xn) {
            const CapnpPlace lp = ar.alloc(0u, 1u + 4u * xn);
            f(K_EXTRA, 0u, lp, xn, ar);
            extra_objs(ar, lp.seg, xn, [&](uint32_t, uint32_t i, const CapnpPlace& kp, uint32_t kl, const CapnpPlace& vp, uint32_t vl) {
                f(K_XKEY, i, kp, kl, ar);
                f(K_XVAL, i, vp, vl, ar);
            });
        }
    }
    // the pointer at word `pw` of its segment to the object at p: near, or far to p's landing pad
    FGE_HD void ptr(const CapnpPlace& p, uint32_t pw, uint32_t hi) {
        if (p.far) word(2u | (p.pos - 1u) << 3, p.seg);
        else word(near_lo(pw, p.pos), hi);
    }
    FGE_HD void list_words(const CapnpPlace& lp, uint32_t n, bool extra, uint32_t elo, uint32_t ehi, const CapnpArena& after) {
        word(n << 2, 2u | 2u << 16);
        CapnpArena sub = after;
        auto st = [&](uint32_t i, uint32_t e, const CapnpPlace& kp, uint32_t kl, const CapnpPlace& vp, uint32_t vl) {
            const uint32_t sw = lp.pos + 1u + 4u * i;
            if (extra) {
                word(0u, 0u);
                word(0u, 0u);
                ptr(kp, sw + 2u, text_hi(kl));
                ptr(vp, sw + 3u, text_hi(vl));
                return;
            }
            const uint32_t ty = t.ent_type[e];
            const uint64_t v = t.ent_val[e];
            const bool num = ty == FG_T_F64 || ty == FG_T_I64 || ty == FG_T_U64;
            word(ty | ((ty == FG_T_BOOL && v != 0u) ? 1u << 16 : 0u), 0u);
            word(num ? (uint32_t)v : 0u, num ? (uint32_t)(v >> 32) : 0u);
            ptr(kp, sw + 2u, text_hi(kl));
            if (ty == FG_T_STRING) ptr(vp, sw + 3u, text_hi(vl));
            else word(0u, 0u);
        };
        if (extra) extra_objs(sub, lp.seg, n, st);
        else pair_objs(sub, lp.seg, elo, ehi, st);
        flush();
    }
    FGE_HD void run_multi() {
        uint32_t sdid, elo, ehi;
        sd0(sdid, elo, ehi);
        const uint32_t xn = extra_n();
        // pass 1: the segments, and where the root's nine pointers go
        CapnpArena ar;
        CapnpPlace rp[9];
        uint32_t rhi[9], ron[9];
        for (uint32_t j = 0; j < 9u; ++j) ron[j] = 0u;
        walk(ar, sdid, elo, ehi, xn, [&](uint32_t kind, uint32_t idx, const CapnpPlace& p, uint32_t n, const CapnpArena&) {
            const uint32_t j = kind == K_FIELD ? idx : kind == K_SDID ? 6u : kind == K_PAIRS ? 7u : kind == K_EXTRA ? 8u : 9u;
            if (j == 9u) return;
            rp[j] = p;
            rhi[j] = (kind == K_PAIRS || kind == K_EXTRA) ? list_hi(n) : text_hi(n);
            ron[j] = 1u;
        });
        const uint32_t nseg = ar.nseg;
        uint32_t words = (nseg + 2u) >> 1;  // the segment table: count - 1, one size per segment, padded to a whole word
        for (uint32_t s = 0; s < nseg; ++s) words += ar.used[s];
        if (S::kCount) {
            out.add(8u * words);
            return;
        }
        for (uint32_t k = 0; k < nseg + 1u; k += 2u) word(k == 0u ? nseg - 1u : ar.used[k - 1u], k < nseg ? ar.used[k] : 0u);
        flush();
        // pass 2 per segment: its objects in allocation order are its words in order
        for (uint32_t s = 0; s < nseg; ++s) {
            CapnpArena cur;
            walk(cur, sdid, elo, ehi, xn, [&](uint32_t kind, uint32_t idx, const CapnpPlace& p, uint32_t n, const CapnpArena& after) {
                if (p.seg != s) return;
                if (kind == K_ROOT) {
                    word(0u, 0x00090002u);
                    data_words();
                    for (uint32_t j = 0; j < 9u; ++j) {
                        if (ron[j]) ptr(rp[j], 3u + j, rhi[j]);
                        else word(0u, 0u);
                    }
                    flush();
                    return;
                }
                const bool list = kind == K_PAIRS || kind == K_EXTRA;
                if (p.far) {  // the landing pad: the object's own pointer, offset 0
                    word(1u, list ? list_hi(n) : text_hi(n));
                    flush();
                }
                if (list) list_words(p, n, kind == K_EXTRA, elo, ehi, after);
                else if (kind == K_FIELD) field_text((int)idx, n);
                else if (kind == K_SDID) sdid_text(idx);
                else if (kind == K_KEY) key_text(idx);
                else if (kind == K_VAL) val_text(idx);
                else this->blob(cfg.ltsv_extra_off + 8u * xtext_word(idx, kind == K_XVAL ? 1u : 0u), 8u * tw(n));
            });
        }
    }
};

// ---- mergers ------------------------------------------------------------------------------------
FGE_HD uint32_t dec_digits(uint64_t v) {
    uint32_t n = 1;
    while (v >= 10u) {
        v /= 10u;
        ++n;
    }
    return n;
}
// framed size of an encoded message of `n` bytes
FGE_HD uint64_t framed_size(uint32_t merger, uint64_t n) {
    switch (merger) {
        case FG_MERGE_LINE:
        case FG_MERGE_NUL: return n + 1u;
        case FG_MERGE_SYSLEN: return n + 2u + dec_digits(n + 1u);  // "{n+1} " + bytes + "\n"
        default: return n;
    }
}
// the encoded size of a syslen frame of `total` bytes (framed_size is strictly increasing: unique)
FGE_HD uint64_t syslen_payload(uint64_t total) {
    for (uint32_t d = 1; d <= 20u; ++d) {
        if (total < 2u + d) break;
        const uint64_t n = total - 2u - d;
        if (dec_digits(n + 1u) == d) return n;
    }
    return 0;
}


// ---- one row through encoder ENC (+ merger): the per-line body of the count and the write kernels, shared with the
//      host tests.  keys64 / slot_ent / order: kSortSlots scratch entries each (used by the GELF emitter only). ------
template <uint32_t ENC, class S, class R>
FGE_HD uint32_t encode_row(S& sink, const EncCfg& cfg, R rd, const DevTables& t, uint64_t li, uint32_t meta, uint64_t* keys64,
                           uint8_t* slot_ent, uint8_t* order, const RowRegs* pre = nullptr) {
    if (ENC == FG_ENC_GELF) {
        GelfEmitter<S, R> em(sink, cfg, rd, t, li, meta, pre);
        return em.run(keys64, slot_ent, order);
    } else if (ENC == FG_ENC_LTSV) {
        LtsvEmitter<S, R> em(sink, cfg, rd, t, li, meta, pre);
        return em.run();
    } else if (ENC == FG_ENC_RFC5424) {
        Rfc5424Emitter<S, R> em(sink, cfg, rd, t, li, meta, pre);
        return em.run();
    } else if (ENC == FG_ENC_RFC3164) {
        Rfc3164Emitter<S, R> em(sink, cfg, rd, t, li, meta, pre);
        return em.run();
    } else if (ENC == FG_ENC_CAPNP) {
        CapnpEmitter<S, R> em(sink, cfg, rd, t, li, meta, pre);
        return em.run();
    } else {
        PassthroughEmitter<S, R> em(sink, cfg, rd, t, li, meta, pre);
        return em.run();
    }
}
// count pass: the framed size of row li (0 when nothing is produced) and its encode status
template <uint32_t ENC, class R>
FGE_HD uint32_t row_size(const EncCfg& cfg, R rd, const DevTables& t, uint64_t li, uint32_t meta, uint64_t* keys64, uint8_t* slot_ent,
                         uint8_t* order, uint32_t* status, const RowRegs* pre = nullptr, uint32_t* plain = nullptr) {
    if (plain) *plain = 0u;
    if (FG_META_STATUS(meta) != 0u) {
        *status = ES_DECODE_FAILED;
        return 0;
    }
    CountSink cs;
    const uint32_t st = encode_row<ENC>(cs, cfg, rd, t, li, meta, keys64, slot_ent, order, pre);
    *status = st;
    if (plain) *plain = cs.slow ? 0u : 1u;  // (RowRegs::plain of the write pass)
    return st == ES_OK ? (uint32_t)framed_size(cfg.merger, cs.n) : 0u;
}
// write pass: `total` = the framed size the count pass returned for this row (the sink starts at the row's offset)
template <uint32_t ENC, class W, class R>
FGE_HD void row_write(W& sink, uint64_t total, const EncCfg& cfg, R rd, const DevTables& t, uint64_t li, uint32_t meta, uint64_t* keys64,
                      uint8_t* slot_ent, uint8_t* order, const RowRegs* pre = nullptr) {
    if (total == 0 || FG_META_STATUS(meta) != 0u) return;
    if (cfg.merger == FG_MERGE_SYSLEN) {  // "{len + 1} " in front (syslen_merger.rs:18-20)
        u64_digits(syslen_payload(total) + 1u, [&](uint32_t c) { sink.put(c); });
        sink.put(' ');
    }
    (void)encode_row<ENC>(sink, cfg, rd, t, li, meta, keys64, slot_ent, order, pre);
    if (cfg.merger == FG_MERGE_LINE || cfg.merger == FG_MERGE_SYSLEN) sink.put('\n');
    else if (cfg.merger == FG_MERGE_NUL) sink.put(0u);
    sink.finish();
}

}  // namespace emit
}  // namespace fg
