// fg_inflate.hpp -- the inflate core of the UDP input: the reference's gate (handle_record_maybe_compressed,
// src/flowgger/input/udp_input.rs:100-143), the RFC 1950 (zlib) and RFC 1952 (gzip) wrappers and RFC 1951 (deflate: stored, fixed and
// dynamic blocks) for ONE datagram, walked by one lane.  No HIP, no wave primitives: hipcc compiles it into the kernels of fg_udp.hip
// and g++ into tests/native/inflate_host.cpp, so the CPU suite runs what the GPU runs.
//
// The semantics are zlib's inflate(), down to which malformations are errors:
//   oversubscribed code sets; incomplete ones, except a code set whose only codes are one bit long (literal/length or distance) and
//   a distance set without any code; a missing end-of-block code; HLIT > 286 or HDIST > 30; a repeat without a previous length or
//   past the last length; length symbols 286 / 287 and distance symbols 30 / 31; a distance beyond the bytes produced so far; a
//   stored block whose LEN is not ~NLEN; block type 3; reserved gzip flag bits; a wrong FHCRC; input that ends before the final
//   block's end or before the whole trailer.  Only the first gzip member is read; bytes behind either trailer are ignored.
//
// The walk runs in three forms.  WRITE = false produces no byte: lengths and distances need the symbol stream alone, so it yields the
// inflated size or a verdict.  WRITE = true produces the bytes (back-references read the lane's own earlier output), accumulates
// Adler-32 / CRC-32 and compares the trailer.  STAGED is both in one walk: it writes and sums like WRITE while what the stream
// produces fits a stage of `w` bytes, and from the first piece that would not fit it goes on like the count walk (nothing written,
// nothing summed: the bytes are then owed, and the write walk produces them once the slot is known).
//
// Termination: every loop below either consumes input bits or produces output, the input is bounded by the datagram and the output
// by `lim`; running out of either is a verdict.  Nothing here waits on anything.
//
// Tables are canonical, in the style of Mark Adler's puff: count[16] + symbol[288] for literal/length, count[16] + symbol[30] for
// distance, the code lengths as bytes.  They live behind `Tabs`, a strided view: stride 1 over local arrays on the host, stride 64
// over LDS on the device (lane-interleaved, so that the 64 lanes reading count[k] hit 64 different addresses in 32 dwords).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FG_INF __host__ __device__ inline
#else
#define FG_INF inline
#endif

namespace fg {
namespace inflate {

// fg_udp_status (include/fg_hip.h)
enum { UDP_RAW = 0, UDP_ZLIB = 1, UDP_GZIP = 2, UDP_BAD_ZLIB = 3, UDP_BAD_GZIP = 4, UDP_BAD_UTF8 = 5, UDP_TOO_LARGE = 6 };
// how a walk ended
enum { R_OK = 0, R_BAD = 1, R_TRUNC = 2, R_TOO_LARGE = 3, R_BAD_CHECK = 4 };

constexpr uint32_t kHalfWords = 16u + 288u + 16u + 30u;  // u16 per lane: lcount, lsym, dcount, dsym
constexpr uint32_t kLenBytes = 320u;                     // u8 per lane: the code lengths of a dynamic block (286 + 30, rounded)
constexpr uint32_t kLCount = 0u, kLSym = 16u, kDCount = 304u, kDSym = 320u;
constexpr uint32_t kTabBytesPerLane = kHalfWords * 2u + kLenBytes;  // 1020

// the reference's gate: which inflater a datagram goes to (udp_input.rs:104-127)
FG_INF uint32_t classify(const uint8_t* p, uint64_t len) {
    if (len >= 8u && p[0] == 0x78u && (p[1] == 0x01u || p[1] == 0x9cu || p[1] == 0xdau)) return UDP_ZLIB;
    if (len >= 24u && p[0] == 0x1fu && p[1] == 0x8bu && p[2] == 0x08u) return UDP_GZIP;
    return UDP_RAW;
}

struct Tabs {
    uint16_t* h;  // kHalfWords entries, `stride` apart
    uint8_t* b;   // kLenBytes entries, `stride` apart
    uint32_t stride;
    FG_INF uint16_t& H(uint32_t k) const { return h[k * stride]; }
    FG_INF uint8_t& B(uint32_t k) const { return b[k * stride]; }
};

// LSB-first bit reader over [p, p + end): a 64-bit buffer refilled four bytes at a time by unaligned loads while four bytes are
// left, byte by byte behind that (never a byte past the datagram)
struct Bits {
    const uint8_t* p;
    uint32_t pos, end;
    uint64_t buf;
    uint32_t cnt;
    FG_INF void refill() {
        while (cnt <= 32u && pos < end) {
            if (end - pos >= 4u) {
                uint32_t v;
                __builtin_memcpy(&v, p + pos, 4);
                buf |= (uint64_t)v << cnt;
                pos += 4u;
                cnt += 32u;
            } else {
                buf |= (uint64_t)p[pos++] << cnt;
                cnt += 8u;
            }
        }
    }
    FG_INF bool need(uint32_t n) {  // n <= 32
        if (cnt < n) refill();
        return cnt >= n;
    }
    FG_INF uint32_t get(uint32_t n) {  // after need(n)
        const uint32_t v = (uint32_t)(buf & ((1ull << n) - 1ull));
        buf >>= n;
        cnt -= n;
        return v;
    }
    FG_INF void to_bytes() {  // drop the rest of the current byte and hand the whole bytes of the buffer back
        pos -= cnt >> 3;  // (the buffer was filled bytewise: cnt & 7 bits are what is left of the current byte)
        buf = 0;
        cnt = 0;
    }
};

// the canonical code of n symbols whose lengths are B(first .. first + n): counts at H(c0 + 0..15), symbols from H(s0).
// Returns what is left of the code space (< 0 oversubscribed, 0 complete, > 0 incomplete); *maxlen = the longest code (0: no code).
FG_INF int build(const Tabs& t, uint32_t c0, uint32_t s0, uint32_t first, uint32_t n, uint32_t* maxlen) {
    for (uint32_t l = 0; l < 16u; ++l) t.H(c0 + l) = 0;
    for (uint32_t s = 0; s < n; ++s) t.H(c0 + t.B(first + s)) += 1u;
    int left = 1;
    uint32_t mx = 0;
    for (uint32_t l = 1; l < 16u; ++l) {
        const uint32_t c = t.H(c0 + l);
        left = (left << 1) - (int)c;
        if (left < 0) return left;
        if (c) mx = l;
    }
    *maxlen = mx;
    // symbols sorted by length, by symbol inside a length.  The counts double as the insertion cursors: turned into starts, advanced
    // by the fill, they end as the starts of the NEXT length, from which the counts come back.
    uint32_t run = 0;
    for (uint32_t l = 1; l < 16u; ++l) {
        const uint32_t c = t.H(c0 + l);
        t.H(c0 + l) = (uint16_t)run;
        run += c;
    }
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t l = t.B(first + s);
        if (l) {
            const uint32_t at = t.H(c0 + l);
            t.H(s0 + at) = (uint16_t)s;
            t.H(c0 + l) = (uint16_t)(at + 1u);
        }
    }
    t.H(c0) = 0;
    for (uint32_t l = 15u; l >= 1u; --l) t.H(c0 + l) = (uint16_t)(t.H(c0 + l) - t.H(c0 + l - 1u));
    return left;
}

// one symbol of the code at (c0, s0): >= 0 the symbol, -1 no such code (zlib: "invalid code"), -2 the input ended
FG_INF int decode(Bits& br, const Tabs& t, uint32_t c0, uint32_t s0, uint32_t maxlen) {
    br.refill();
    if (maxlen == 0u) return br.cnt ? -1 : -2;  // (zlib's table of an empty code set: one-bit entries that are all invalid)
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t l = 1; l <= maxlen; ++l) {
        if (br.cnt == 0u) return -2;
        code |= (uint32_t)(br.buf & 1ull);
        br.buf >>= 1;
        br.cnt -= 1u;
        const uint32_t c = t.H(c0 + l);
        if (code < first + c) return (int)t.H(s0 + index + (code - first));  // (code >= first always)
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return -1;
}

FG_INF uint32_t clen_order(uint32_t k) {  // 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 |
                        5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((k < 12u ? lo >> (5u * k) : hi >> (5u * (k - 12u))) & 31ull);
}

struct Sums {  // of the bytes produced (WRITE)
    uint32_t a1, a2, crc;
    FG_INF void add(uint32_t b, bool gz) {
        if (gz) {
            uint32_t c = crc ^ b;
            for (int k = 0; k < 8; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
            crc = c;
        } else {
            a1 += b;
            if (a1 >= 65521u) a1 -= 65521u;
            a2 += a1;
            if (a2 >= 65521u) a2 -= 65521u;
        }
    }
};

struct Lens {  // what the two codes of the current block look like
    uint32_t lmax, dmax;
    bool fixed;  // the tables hold the fixed codes (not rebuilt for the next fixed block)
};

// the fixed codes of RFC 1951 3.2.6 into the tables
FG_INF void build_fixed(const Tabs& t, Lens* ln) {
    for (uint32_t s = 0; s < 288u; ++s) t.B(s) = (uint8_t)(s < 144u ? 8u : s < 256u ? 9u : s < 280u ? 7u : 8u);
    (void)build(t, kLCount, kLSym, 0u, 288u, &ln->lmax);
    for (uint32_t s = 0; s < 30u; ++s) t.B(s) = 5u;
    (void)build(t, kDCount, kDSym, 0u, 30u, &ln->dmax);  // (30 and 31 have no entry: decode() answers "invalid code" for them)
    ln->fixed = true;
}

// the header of a dynamic block: R_OK with both codes built, or a verdict
FG_INF int build_dynamic(Bits& br, const Tabs& t, Lens* ln) {
    ln->fixed = false;
    if (!br.need(14u)) return R_TRUNC;
    const uint32_t nlen = br.get(5u) + 257u, ndist = br.get(5u) + 1u, ncode = br.get(4u) + 4u;
    if (nlen > 286u || ndist > 30u) return R_BAD;
    for (uint32_t k = 0; k < 19u; ++k) t.B(k) = 0;
    for (uint32_t k = 0; k < ncode; ++k) {
        if (!br.need(3u)) return R_TRUNC;
        t.B(clen_order(k)) = (uint8_t)br.get(3u);
    }
    uint32_t cmax = 0;
    const int cleft = build(t, kLCount, kLSym, 0u, 19u, &cmax);  // (the code-length code borrows the literal/length tables)
    if (cleft < 0 || (cleft > 0 && cmax != 0u)) return R_BAD;
    const uint32_t total = nlen + ndist;
    if (cmax == 0u) {
        // zlib's table for a code-length code without codes answers length 0 for one bit each, and the block then has no
        // end-of-block code: an error, but only once the bits were there
        for (uint32_t k = 0; k < total; ++k) {
            if (!br.need(1u)) return R_TRUNC;
            (void)br.get(1u);
        }
        return R_BAD;
    }
    uint32_t have = 0, prev = 0;
    while (have < total) {
        const int sym = decode(br, t, kLCount, kLSym, cmax);
        if (sym == -2) return R_TRUNC;
        if (sym < 0) return R_BAD;
        if (sym < 16) {
            prev = (uint32_t)sym;
            t.B(have++) = (uint8_t)sym;
            continue;
        }
        uint32_t rep, val = 0;
        if (sym == 16) {
            if (!br.need(2u)) return R_TRUNC;
            if (have == 0u) return R_BAD;
            val = prev;
            rep = 3u + br.get(2u);
        } else if (sym == 17) {
            if (!br.need(3u)) return R_TRUNC;
            rep = 3u + br.get(3u);
        } else {
            if (!br.need(7u)) return R_TRUNC;
            rep = 11u + br.get(7u);
        }
        if (have + rep > total) return R_BAD;
        prev = val;
        for (uint32_t k = 0; k < rep; ++k) t.B(have++) = (uint8_t)val;
    }
    if (t.B(256u) == 0u) return R_BAD;  // no end-of-block code
    const int lleft = build(t, kLCount, kLSym, 0u, nlen, &ln->lmax);
    if (lleft < 0 || (lleft > 0 && ln->lmax != 1u)) return R_BAD;
    const int dleft = build(t, kDCount, kDSym, nlen, ndist, &ln->dmax);
    if (dleft < 0 || (dleft > 0 && ln->dmax > 1u)) return R_BAD;
    return R_OK;
}

// the forms of the walk (inflate_blocks<false> and <true> are the first two)
enum { COUNT = 0, WRITE_ALL = 1, STAGED = 2 };

// The deflate stream at the reader's position into out[0 .. lim): R_OK at the end of the final block (the reader stands at the next
// whole byte), R_TOO_LARGE when a byte beyond `lim` was asked for.  *produced = the bytes produced (counted, when MODE == COUNT).
// STAGED: out[0 .. w) is the stage and *live says whether every byte so far went into it (a piece -- literal, match, stored run --
// that would end beyond w is not written at all, and nothing is after it; the sums then stop too).
template <int MODE>
FG_INF int inflate_blocks(Bits& br, const Tabs& t, uint8_t* out, uint32_t lim, bool gz, Sums* sums, uint32_t* produced, uint32_t w = 0u,
                          bool* live = nullptr) {
    uint32_t o = 0;
    bool wr = MODE != COUNT;  // (a constant in the first two forms)
    Lens ln{0u, 0u, false};
    int rc = R_OK;
    for (;;) {  // (every block consumes its three header bits)
        if (!br.need(3u)) { rc = R_TRUNC; break; }
        const uint32_t last = br.get(1u), type = br.get(2u);
        if (type == 0u) {
            br.to_bytes();  // (to the byte boundary; the block is read bytewise)
            if (br.end - br.pos < 4u) { rc = R_TRUNC; break; }
            const uint32_t len = br.p[br.pos] | (uint32_t)br.p[br.pos + 1u] << 8;
            const uint32_t nlen = br.p[br.pos + 2u] | (uint32_t)br.p[br.pos + 3u] << 8;
            if (len != (nlen ^ 0xFFFFu)) { rc = R_BAD; break; }
            br.pos += 4u;
            const uint32_t avail = br.end - br.pos, take = len < avail ? len : avail;
            if (take) {
                if (take > lim - o) { rc = R_TOO_LARGE; break; }
                if (MODE == STAGED && wr && (o > w || take > w - o)) wr = false;
                if (MODE != COUNT && wr)
                    for (uint32_t k = 0; k < take; ++k) {
                        const uint32_t b = br.p[br.pos + k];
                        out[o + k] = (uint8_t)b;
                        sums->add(b, gz);
                    }
                o += take;
                br.pos += take;
            }
            if (take < len) { rc = R_TRUNC; break; }
        } else if (type == 3u) {
            rc = R_BAD;
            break;
        } else {
            if (type == 1u) {
                if (!ln.fixed) build_fixed(t, &ln);
            } else if ((rc = build_dynamic(br, t, &ln)) != R_OK) {
                break;
            }
            for (;;) {  // (every symbol consumes at least one bit)
                const int sym = decode(br, t, kLCount, kLSym, ln.lmax);
                if (sym < 0) { rc = sym == -2 ? R_TRUNC : R_BAD; break; }
                if (sym < 256) {
                    if (o == lim) { rc = R_TOO_LARGE; break; }
                    if (MODE == STAGED && wr && o >= w) wr = false;
                    if (MODE != COUNT && wr) {
                        out[o] = (uint8_t)sym;
                        sums->add((uint32_t)sym, gz);
                    }
                    ++o;
                    continue;
                }
                if (sym == 256) break;
                if (sym >= 286) { rc = R_BAD; break; }
                const uint32_t i = (uint32_t)sym - 257u;
                uint32_t len;
                if (i < 8u) {
                    len = 3u + i;
                } else if (i == 28u) {
                    len = 258u;
                } else {
                    const uint32_t eb = (i - 4u) >> 2;
                    if (!br.need(eb)) { rc = R_TRUNC; break; }
                    len = 3u + ((4u + (i & 3u)) << eb) + br.get(eb);
                }
                const int ds = decode(br, t, kDCount, kDSym, ln.dmax);
                if (ds < 0) { rc = ds == -2 ? R_TRUNC : R_BAD; break; }
                const uint32_t d = (uint32_t)ds;
                if (d >= 30u) { rc = R_BAD; break; }
                uint32_t dist;
                if (d < 4u) {
                    dist = 1u + d;
                } else {
                    const uint32_t eb = (d >> 1) - 1u;
                    if (!br.need(eb)) { rc = R_TRUNC; break; }
                    dist = 1u + ((2u + (d & 1u)) << eb) + br.get(eb);
                }
                if (o == lim) { rc = R_TOO_LARGE; break; }  // (zlib stops for room before it looks at the distance)
                if (dist > o) { rc = R_BAD; break; }
                if (len > lim - o) { rc = R_TOO_LARGE; break; }
                if (MODE == STAGED && wr && (o > w || len > w - o)) wr = false;
                if (MODE != COUNT && wr)
                    for (uint32_t k = 0; k < len; ++k) {  // (overlapping on purpose: distance 1 repeats the last byte)
                        const uint32_t b = out[o + k - dist];
                        out[o + k] = (uint8_t)b;
                        sums->add(b, gz);
                    }
                o += len;
            }
            if (rc != R_OK) break;
        }
        if (last) {
            br.to_bytes();
            break;
        }
    }
    *produced = o;
    if (MODE == STAGED) *live = wr;
    return rc;
}

// One datagram that classify() sent to an inflater (kind = UDP_ZLIB / UDP_GZIP), into out[0 .. lim).  Returns R_*; *produced = the
// bytes produced.  COUNT: nothing is written, the trailer only has to be there.  WRITE_ALL: R_BAD_CHECK when the trailer disagrees with
// the bytes (which stay).  STAGED (stage out[0 .. w), *live as inflate_blocks leaves it): the trailer is compared while *live, only
// looked for otherwise.
template <int MODE>
FG_INF int inflate_datagram(const uint8_t* p, uint32_t len, uint32_t kind, const Tabs& t, uint8_t* out, uint32_t lim, uint32_t* produced,
                            uint32_t w = 0u, bool* live = nullptr) {
    *produced = 0;
    if (MODE == STAGED) *live = true;
    const bool gz = kind == UDP_GZIP;
    uint32_t pos;
    if (!gz) {
        if (len < 2u) return R_TRUNC;
        const uint32_t cmf = p[0], flg = p[1];
        if (((cmf << 8) | flg) % 31u != 0u || (cmf & 15u) != 8u || (cmf >> 4) > 7u || (flg & 0x20u)) return R_BAD;  // FCHECK, CM, CINFO, FDICT
        pos = 2u;
    } else {
        if (len < 10u) return R_TRUNC;
        if (p[0] != 0x1fu || p[1] != 0x8bu || p[2] != 8u) return R_BAD;
        const uint32_t flg = p[3];
        if (flg & 0xE0u) return R_BAD;  // reserved flag bits
        pos = 10u;
        if (flg & 4u) {  // FEXTRA
            if (len - pos < 2u) return R_TRUNC;
            const uint32_t xlen = p[pos] | (uint32_t)p[pos + 1u] << 8;
            pos += 2u;
            if (len - pos < xlen) return R_TRUNC;
            pos += xlen;
        }
        for (uint32_t f = 8u; f <= 16u; f <<= 1) {  // FNAME, FCOMMENT: zero-terminated
            if (!(flg & f)) continue;
            while (pos < len && p[pos] != 0u) ++pos;
            if (pos == len) return R_TRUNC;
            ++pos;
        }
        if (flg & 2u) {  // FHCRC: the low half of the CRC-32 of the header so far
            if (len - pos < 2u) return R_TRUNC;
            Sums h{0u, 0u, 0xFFFFFFFFu};
            for (uint32_t k = 0; k < pos; ++k) h.add(p[k], true);
            if (((h.crc ^ 0xFFFFFFFFu) & 0xFFFFu) != (p[pos] | (uint32_t)p[pos + 1u] << 8)) return R_BAD;
            pos += 2u;
        }
    }
    Bits br{p, pos, len, 0ull, 0u};
    Sums sums{1u, 0u, 0xFFFFFFFFu};
    const int rc = inflate_blocks<MODE>(br, t, out, lim, gz, &sums, produced, w, live);
    if (rc != R_OK) return rc;
    const uint32_t tail = gz ? 8u : 4u;
    if (br.end - br.pos < tail) return R_TRUNC;
    if (MODE == WRITE_ALL || (MODE == STAGED && *live)) {
        const uint8_t* q = p + br.pos;
        if (gz) {
            const uint32_t crc = q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
            const uint32_t isz = q[4] | (uint32_t)q[5] << 8 | (uint32_t)q[6] << 16 | (uint32_t)q[7] << 24;
            if (crc != (sums.crc ^ 0xFFFFFFFFu) || isz != *produced) return R_BAD_CHECK;
        } else {
            const uint32_t ad = (uint32_t)q[0] << 24 | (uint32_t)q[1] << 16 | (uint32_t)q[2] << 8 | q[3];
            if (ad != (sums.a2 << 16 | sums.a1)) return R_BAD_CHECK;
        }
    }
    return R_OK;
}

// what a walk with max_inflated + 1 bytes of room that ended with rc after `produced` bytes means for the datagram (rc is not
// R_BAD_CHECK): its fg_udp_status so far, *size = the bytes its slot needs
FG_INF uint32_t count_verdict(uint32_t kind, int rc, uint32_t produced, uint32_t max_inflated, uint32_t* size) {
    *size = 0;
    const uint32_t bad = kind == UDP_GZIP ? UDP_BAD_GZIP : UDP_BAD_ZLIB;
    if (rc == R_BAD) return bad;
    if (rc == R_OK && produced == max_inflated + 1u) {
        // One byte too many AND complete: zlib had the room to reach the trailer, so a wrong checksum is still its error.  The row
        // is dropped either way; it keeps a slot so that the write pass can tell which.
        *size = produced;
        return UDP_TOO_LARGE;
    }
    if (rc == R_TOO_LARGE || produced > max_inflated) return UDP_TOO_LARGE;
    if (rc == R_TRUNC) return bad;
    *size = produced;
    return kind;
}

// The count pass's answer for one datagram: *size = the bytes its slot needs, returns the fg_udp_status so far (the write pass may
// still find a wrong checksum, the UTF-8 pass invalid text).  max_inflated < 2^31.
FG_INF uint32_t count_datagram(const uint8_t* p, uint64_t len, uint32_t max_inflated, const Tabs& t, uint32_t* size) {
    *size = 0;
    const uint32_t kind = classify(p, len);
    if (kind == UDP_RAW) {
        if (len > 0x7FFFFFFFull) return UDP_TOO_LARGE;
        *size = (uint32_t)len;
        return UDP_RAW;
    }
    if (len > 0xFFFFFFF0ull) return UDP_TOO_LARGE;
    // zlib with max_inflated + 1 bytes of room: a stream that wants more stops there, one that ends or breaks first does that
    uint32_t produced = 0;
    const int rc = inflate_datagram<false>(p, (uint32_t)len, kind, t, nullptr, max_inflated + 1u, &produced);
    return count_verdict(kind, rc, produced, max_inflated, size);
}

// The write pass for one datagram the count pass gave `size` bytes at `out` (not for a bare record: the wave copies those):
// returns the status it leaves with -- the count pass's, or BAD_* when the trailer disagrees with the bytes.
FG_INF uint32_t write_datagram(const uint8_t* p, uint64_t len, uint32_t st, uint32_t size, const Tabs& t, uint8_t* out) {
    if (!(st == UDP_ZLIB || st == UDP_GZIP || (st == UDP_TOO_LARGE && size != 0u))) return st;
    const uint32_t kind = classify(p, len);
    uint32_t produced = 0;
    const int rc = inflate_datagram<true>(p, (uint32_t)len, kind, t, out, size, &produced);
    if (rc != R_OK || produced != size) return kind == UDP_GZIP ? UDP_BAD_GZIP : UDP_BAD_ZLIB;
    return st;
}

// ---- the one-walk form: count and write in one pass over the stream, into a stage whose size is guessed from the datagram's length
// The stage of a datagram of `len` bytes: what a compressed record of that length usually inflates to, and never more than zlib is
// given room for.  A bare record takes none (the wave copies it from the datagram).  K = 4, C = 64: one record per datagram
// compresses about 1.3 times, so a stream that outgrows four times its length is a run-length case, and those pay the
// second walk.  A multiple of 16 unless it is the cap itself.
constexpr uint32_t kStageK = 4u, kStageC = 64u;
FG_INF uint32_t stage_capacity(const uint8_t* p, uint64_t len, uint32_t max_inflated) {
    if (classify(p, len) == UDP_RAW) return 0u;
    const uint64_t guess = ((uint64_t)kStageK * len + kStageC + 15ull) & ~15ull, cap = (uint64_t)max_inflated + 1ull;
    return (uint32_t)(guess < cap ? guess : cap);
}

// One datagram in one walk, with the stage out[0 .. w): returns the fg_udp_status, *size = the bytes of its slot, *spilled = whether
// they did not fit the stage.  Not spilled: status and size are what count_datagram followed by write_datagram leave (the trailer's
// verdict included) and out[0 .. size) holds the slot's bytes.  Spilled: they are count_datagram's, and write_datagram still has to
// run on the slot.  A bare record is neither staged nor spilled: size = len.  max_inflated < 2^31.
FG_INF uint32_t stage_datagram(const uint8_t* p, uint64_t len, uint32_t max_inflated, uint32_t w, const Tabs& t, uint8_t* out, uint32_t* size,
                               uint32_t* spilled) {
    *size = 0;
    *spilled = 0;
    const uint32_t kind = classify(p, len);
    if (kind == UDP_RAW) {
        if (len > 0x7FFFFFFFull) return UDP_TOO_LARGE;
        *size = (uint32_t)len;
        return UDP_RAW;
    }
    if (len > 0xFFFFFFF0ull) return UDP_TOO_LARGE;
    uint32_t produced = 0;
    bool live = true;
    const int rc = inflate_datagram<STAGED>(p, (uint32_t)len, kind, t, out, max_inflated + 1u, &produced, w, &live);
    if (rc == R_BAD_CHECK) {  // (live, so the bytes are in the stage: they keep their slot, as behind write_datagram)
        *size = produced;
        return kind == UDP_GZIP ? UDP_BAD_GZIP : UDP_BAD_ZLIB;
    }
    const uint32_t st = count_verdict(kind, rc, produced, max_inflated, size);
    *spilled = *size != 0u && !live ? 1u : 0u;  // (a stream without a slot owes nothing)
    return st;
}

}  // namespace inflate
}  // namespace fg
