// fg_kafka.hpp -- Kafka v0 message sets over a resident byte buffer: every message of an encoder's output behind its 26-byte header with
// its own CRC-32, and a compressed member inside its wrapper message (attributes = 1).  No HIP beyond fg_wave.hpp's vocabulary, in the
// way of fg_deflate.hpp: hipcc compiles it into the kernels of fg_kafka.hip and g++ into tests/native/kafka_host.cpp, where a wave is
// 64 fibers, so the CPU suite runs what the GPU runs and both produce the same bytes.
//
// A message (all integers big-endian):  offset 8 (0) | message_size 4 (14 + value) | crc 4 | magic 1 (0) | attributes 1 | key length 4
// (-1: null) | value length 4 | value.  The CRC-32 (IEEE, zlib's) covers magic .. the value's end.
//
// copy_crc() is the one pass that touches the bytes: a GROUP of lanes (a row of sixteen for a message of at most kRowMax bytes, four
// messages a wave; the whole wave beyond that and for a piece of a compressed member) copies the value and leaves the CRC register:
//   pieces    the destination decides them: up to fifteen head bytes to its first 16-byte boundary, then quads (16 bytes, one aligned
//             store each, the source read unaligned), then up to fifteen tail bytes.  Every lane takes c = ceil(quads / lanes) quads in
//             a row, the LAST lane ending at the last quad -- so all chunks are 16 c bytes long and what is missing lies in front of
//             the first one, where zero bytes do not change a register that starts at zero.
//   register  the lane that holds quad 0 starts from the seed (the register after the ten header bytes behind the crc field, which
//             depend on the length alone) and takes the head bytes first; every other lane starts from zero.  A word is four lookups in
//             a 4 x 256 table in LDS (slicing by four), a byte one.
//             The head's and the tail's bytes come from ONE 16-byte load each, asked for with the first quad before anything goes
//             through the register: no loop waits for memory once per byte.
//   fold      crc(A || B) = crc(A) * x^(8 |B|) xor crc(B): with equal chunks a tree -- lane i takes lane i - d's register times
//             x^(8 * 16 c d) for d = 1, 2, 4 .. --, log2(lanes) multiplications a group; the powers for c <= 16 (a row always, the
//             wave up to 16 KiB) from a table in LDS.  The group's last lane then takes the tail bytes.
// Nothing depends on the order the hardware runs lanes or waves in: every byte and every register is a function of the input.
#pragma once
#include <stdint.h>

#include "fg_deflate.hpp"  // gf_mul, x_pow8, Quad, member_of

namespace fg {
namespace kafka {

using fg::deflate::gf_mul;
using fg::deflate::x_pow8;

constexpr uint32_t kOverhead = 26u;       // fg_kafka_message_overhead(): a message's bytes beyond its value
constexpr uint32_t kCrcFrom = 16u;        // where the bytes the CRC covers start (magic)
constexpr uint32_t kRowLanes = 16u;
constexpr uint32_t kRowQuads = 16u;       // the most quads a lane of a row takes ...
constexpr uint32_t kRowMax = kRowLanes * kRowQuads * 16u;  // ... so a row takes a value of at most 4096 bytes, the wave a longer one
constexpr uint32_t kRowsPerWave = wv::kLanes / kRowLanes;
constexpr uint32_t kPiece = 16384u;       // a compressed member's bytes per wave (the wrapper's CRC is folded per member)
constexpr uint64_t kMaxValue = 0x7FFFFFFFull - kOverhead;  // a message's wire size fits int32
constexpr uint32_t kTabWords = 1024u;     // the slicing tables
constexpr uint32_t kXStride = 20u, kXWords = 4u * kXStride;  // x^(8 * 16 c * 2^level) mod P for c = 0 .. kRowQuads, level = 0 .. 3
constexpr uint32_t kLdsWords = kTabWords + kXWords;
static_assert(kRowQuads < kXStride, "a level's powers fit its stride");

FG_WVH uint64_t wire_size(uint64_t len, bool skip) { return skip ? 0u : kOverhead + len; }
// bytes that always suffice for the plain set of n messages over nbytes and for its compressed members in their wrappers
FG_WVH uint64_t bound(uint64_t nbytes, uint64_t n, uint64_t n_members) {
    return fg::deflate::bound(nbytes + (uint64_t)kOverhead * n, n_members) + (uint64_t)kOverhead * n_members;
}
FG_WVH uint64_t pieces_of(uint64_t len) { return (len + kPiece - 1u) / kPiece; }
// byte k < 26 of the header of a message with `len` value bytes
FG_WVH uint8_t header_byte(uint32_t k, uint32_t len, uint32_t attr, uint32_t crc) {
    if (k < 8u) return 0u;
    if (k < 12u) return (uint8_t)((len + 14u) >> (8u * (11u - k)));
    if (k < 16u) return (uint8_t)(crc >> (8u * (15u - k)));
    if (k == 16u) return 0u;
    if (k == 17u) return (uint8_t)attr;
    if (k < 22u) return 0xFFu;
    return (uint8_t)(len >> (8u * (25u - k)));
}
// ... and the CRC register behind its last ten bytes, bit by bit (per member, and what the tests hold the table against)
FG_WVH uint32_t header_state_bits(uint32_t len, uint32_t attr) {
    uint32_t st = 0xFFFFFFFFu;
    for (uint32_t k = kCrcFrom; k < kOverhead; ++k) {
        st ^= header_byte(k, len, attr, 0u);
        for (uint32_t b = 0; b < 8u; ++b) st = (st >> 1) ^ (0xEDB88320u & (0u - (st & 1u)));
    }
    return st;
}

struct Lds {
    const uint32_t* tab;  // kTabWords: T0 | T1 | T2 | T3
    const uint32_t* xq;   // x^(8 * 16 c) mod P, c = 0 .. kRowQuads
};
FG_WV Lds lds_of(const uint32_t* base) { return Lds{base, base + kTabWords}; }
// the tables, by the wave
FG_WV void build_tables(uint32_t* base) {
    const uint32_t l = wv::lane();
    for (uint32_t b = l; b < 256u; b += wv::kLanes) {
        uint32_t c = b;
        for (uint32_t k = 0; k < 8u; ++k) c = (c >> 1) ^ (0xEDB88320u & (0u - (c & 1u)));
        base[b] = c;
    }
    wv::sync();
    for (uint32_t t = 1; t < 4u; ++t) {
        for (uint32_t b = l; b < 256u; b += wv::kLanes) {
            const uint32_t p = base[(t - 1u) * 256u + b];
            base[t * 256u + b] = (p >> 8) ^ base[p & 0xFFu];
        }
        wv::sync();
    }
    // x^(8 * 16 c): the unit through 16 c zero bytes, four a step; then squared for the tree's further steps
    uint32_t x = 0x80000000u;
    const uint32_t c = l <= kRowQuads ? l : 0u;
    for (uint32_t k = 0; k < 4u * c; ++k) x = base[768u + (x & 0xFFu)] ^ base[512u + ((x >> 8) & 0xFFu)] ^ base[256u + ((x >> 16) & 0xFFu)] ^ base[x >> 24];
    for (uint32_t lv = 0; lv < 4u; ++lv) {
        if (l <= kRowQuads) base[kTabWords + lv * kXStride + l] = x;
        x = gf_mul(x, x);
    }
    wv::sync();
}
FG_WV uint32_t crc_byte(uint32_t st, uint32_t b, const uint32_t* tab) { return tab[(st ^ b) & 0xFFu] ^ (st >> 8); }
FG_WV uint32_t crc_word(uint32_t st, uint32_t w, const uint32_t* tab) {
    st ^= w;
    return tab[768u + (st & 0xFFu)] ^ tab[512u + ((st >> 8) & 0xFFu)] ^ tab[256u + ((st >> 16) & 0xFFu)] ^ tab[st >> 24];
}
FG_WV uint32_t header_state(uint32_t len, uint32_t attr, const uint32_t* tab) {
    // magic 0, attributes, key length -1 | value length
    uint32_t st = crc_word(0xFFFFFFFFu, 0xFFFF0000u | attr << 8, tab);
    st = crc_word(st, 0x0000FFFFu | (len >> 24) << 16 | ((len >> 16) & 0xFFu) << 24, tab);
    st = crc_byte(st, (len >> 8) & 0xFFu, tab);
    return crc_byte(st, len & 0xFFu, tab);
}

// the first cnt <= 15 bytes of the sixteen in w0 .. w3 (little-endian) to dst and through the register: words, then bytes; no load
FG_WV uint32_t put_bytes(uint8_t* dst, uint32_t w0, uint32_t w1, uint32_t w2, uint32_t w3, uint32_t cnt, uint32_t st, const uint32_t* tab) {
    uint32_t k = 0;
    for (; k + 4u <= cnt; k += 4u) {
        st = crc_word(st, w0, tab);
        dst[k] = (uint8_t)w0;
        dst[k + 1u] = (uint8_t)(w0 >> 8);
        dst[k + 2u] = (uint8_t)(w0 >> 16);
        dst[k + 3u] = (uint8_t)(w0 >> 24);
        w0 = w1;
        w1 = w2;
        w2 = w3;
    }
    for (; k < cnt; ++k) {
        st = crc_byte(st, w0 & 0xFFu, tab);
        dst[k] = (uint8_t)w0;
        w0 >>= 8;
    }
    return st;
}

// dst[0 .. n) = src[0 .. n) by the (1 << lg) lanes of this lane's group, lg = 4 (the row) or 6 (the wave); returns, to the group's
// LAST lane, the CRC register behind the n bytes when it held `seed` in front of them.  Every lane of the wave calls it (a group with
// nothing to do: n = 0); lg and, for lg = 6, every argument are wave-uniform.  A row takes n <= kRowMax.
FG_WV uint32_t copy_crc(uint8_t* dst, const uint8_t* src, uint32_t n, uint32_t seed, uint32_t lg, const Lds& s) {
    const uint32_t l = wv::lane(), lanes = 1u << lg, g = l & (lanes - 1u);
    uint32_t head = (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u;
    if (head > n) head = n;
    const uint32_t nq = (n - head) >> 4, tail = n - head - (nq << 4);
    const uint32_t c = (nq + lanes - 1u) >> lg;
    // this lane's quads [a, b) of [0, nq), the last lane's ending at nq
    const int32_t b = (int32_t)nq - (int32_t)((lanes - 1u - g) * c), a = b - (int32_t)c;
    const bool owner = nq == 0u ? g == lanes - 1u : (a <= 0 && b > 0);
    // Every load this lane needs is asked for before a byte goes through the register: the head's and the tail's sixteen bytes (a value
    // of sixteen bytes or more has them inside it; a shorter one takes the byte loops), the first quad.  A loop that waits for memory
    // once per byte is what this pass must not have.
    using fg::deflate::Quad;
    const bool last = g == lanes - 1u, wide = n >= 16u;
    const int32_t q0 = a < 0 ? 0 : a;
    Quad hq{}, tq{}, cur{};
    if (owner && wide && head) __builtin_memcpy(&hq, src, 16);
    if (last && wide && tail) __builtin_memcpy(&tq, src + (n - 16u), 16);
    if (q0 < b) __builtin_memcpy(&cur, src + head + ((uint32_t)q0 << 4), 16);
    uint32_t st = 0u;
    if (owner) {
        st = seed;
        if (wide) {
            st = put_bytes(dst, hq.q[0], hq.q[1], hq.q[2], hq.q[3], head, st, s.tab);
        } else {
            for (uint32_t k = 0; k < head; ++k) {
                const uint32_t v = src[k];
                dst[k] = (uint8_t)v;
                st = crc_byte(st, v, s.tab);
            }
        }
    }
    for (int32_t q = q0; q < b; ++q) {  // (the next quad is on its way while this one goes through the table)
        const uint32_t at = head + ((uint32_t)q << 4);
        Quad nxt = cur;
        if (q + 1 < b) __builtin_memcpy(&nxt, src + at + 16u, 16);
        *(Quad*)(dst + at) = cur;
        st = crc_word(crc_word(crc_word(crc_word(st, cur.q[0], s.tab), cur.q[1], s.tab), cur.q[2], s.tab), cur.q[3], s.tab);
        cur = nxt;
    }
    // the tree: behind the step of distance d, a lane whose low bits below 2 d are all set holds the register of its 2 d chunks
    // (a lane without bytes holds zero, and zero times anything is zero: idle lanes and idle rows fold along)
    uint32_t x[4];
    if (c <= kRowQuads) {  // (a row always; the wave up to 16 KiB: every piece of a compressed member)
#pragma unroll
        for (uint32_t lv = 0; lv < 4u; ++lv) x[lv] = s.xq[lv * kXStride + c];
    } else {
        x[0] = x_pow8(16ull * c);
#pragma unroll
        for (uint32_t lv = 1; lv < 4u; ++lv) x[lv] = gf_mul(x[lv - 1u], x[lv - 1u]);
    }
    {
        uint32_t r = wv::row_ror<1>(gf_mul(st, x[0]));
        if ((g & 1u) == 1u) st ^= r;
        r = wv::row_ror<2>(gf_mul(st, x[1]));
        if ((g & 3u) == 3u) st ^= r;
        r = wv::row_ror<4>(gf_mul(st, x[2]));
        if ((g & 7u) == 7u) st ^= r;
        r = wv::row_ror<8>(gf_mul(st, x[3]));
        if ((g & 15u) == 15u) st ^= r;
        if (lg == 6u) {
            uint32_t xx = gf_mul(x[3], x[3]);
            r = wv::shfl(gf_mul(st, xx), (l - 16u) & 63u);
            if ((g & 31u) == 31u) st ^= r;
            xx = gf_mul(xx, xx);
            r = wv::shfl(gf_mul(st, xx), (l - 32u) & 63u);
            if (g == 63u) st ^= r;
        }
    }
    if (last) {
        const uint32_t at = head + (nq << 4);
        if (wide) {  // the last `tail` of the sixteen bytes that end the value: down by 16 - tail bytes, words first
            uint32_t w0 = tq.q[0], w1 = tq.q[1], w2 = tq.q[2], w3 = tq.q[3];
            const uint32_t sh = 16u - tail;
            if (sh & 8u) {
                w0 = w2;
                w1 = w3;
                w2 = w3 = 0u;
            }
            if (sh & 4u) {
                w0 = w1;
                w1 = w2;
                w2 = w3;
                w3 = 0u;
            }
            w0 = wv::alignbyte(w1, w0, sh & 3u);
            w1 = wv::alignbyte(w2, w1, sh & 3u);
            w2 = wv::alignbyte(w3, w2, sh & 3u);
            w3 = wv::alignbyte(0u, w3, sh & 3u);
            st = put_bytes(dst + at, w0, w1, w2, w3, tail, st, s.tab);
        } else {
            for (uint32_t k = 0; k < tail; ++k) {
                const uint32_t v = src[at + k];
                dst[at + k] = (uint8_t)v;
                st = crc_byte(st, v, s.tab);
            }
        }
    }
    return st;
}

// the header of the message at dst by this lane's group: `st` = what copy_crc returned (its last lane's counts)
FG_WV void put_header(uint8_t* dst, uint32_t len, uint32_t attr, uint32_t st, uint32_t lg, bool live) {
    const uint32_t l = wv::lane(), lanes = 1u << lg, g = l & (lanes - 1u);
    const uint32_t crc = ~wv::shfl(st, l | (lanes - 1u));
    if (live) {
        if (g < kOverhead) dst[g] = header_byte(g, len, attr, crc);
        if (lg == 4u && g + 16u < kOverhead) dst[g + 16u] = header_byte(g + 16u, len, attr, crc);
    }
}

// whether offsets a, b bound a value the set takes
FG_WVH bool value_ok(uint64_t a, uint64_t b, uint64_t nbytes) { return a <= b && b <= nbytes && b - a <= kMaxValue; }

// One step of k_kf_write by one wave: the kRowsPerWave messages from `first` on, values bytes[off[i] .. off[i + 1]), to set_off[i] in
// set[0 .. set_cap).  skip: null, or nonzero for a row that is not in the set.  Writes only inside [set_off[i], set_off[i + 1]) and only
// when that is the message's size and lies inside set_cap.
FG_WV void write_step(const uint8_t* bytes, const uint64_t* off, const uint8_t* skip, uint64_t n, uint64_t first, const uint64_t* set_off, uint8_t* set,
                      uint64_t set_cap, const Lds& s) {
    const uint32_t l = wv::lane();
    const uint64_t i = first + (l >> 4);
    bool live = i < n && !(skip && skip[i]);
    uint64_t a = 0, so = 0;
    uint32_t len = 0;
    if (live) {
        a = off[i];
        so = set_off[i];
        const uint64_t vl = off[i + 1] - a, end = set_off[i + 1];
        if (vl > kMaxValue || end < so || end - so != kOverhead + vl || end > set_cap) live = false;  // (never: the offsets are the scan of these sizes)
        else len = (uint32_t)vl;
    }
    const bool big = live && len > kRowMax, row = live && !big;
    const uint32_t seed = header_state(len, 0u, s.tab);
    const uint32_t st = copy_crc(set + so + kOverhead, bytes + a, row ? len : 0u, seed, 4u, s);
    put_header(set + so, len, 0u, st, 4u, row);
    // the long ones of the four, one after the other by the whole wave
    uint64_t m = wv::ballot(big && (l & 15u) == 0u);
    while (m) {  // (wave-uniform)
        const uint32_t r = wv::ctz64(m);
        m &= m - 1u;
        const uint64_t ra = (uint64_t)wv::bcast((uint32_t)a, r) | (uint64_t)wv::bcast((uint32_t)(a >> 32), r) << 32;
        const uint64_t rso = (uint64_t)wv::bcast((uint32_t)so, r) | (uint64_t)wv::bcast((uint32_t)(so >> 32), r) << 32;
        const uint32_t rlen = wv::bcast(len, r), rseed = wv::bcast(seed, r);
        const uint32_t rst = copy_crc(set + rso + kOverhead, bytes + ra, rlen, rseed, 6u, s);
        put_header(set + rso, rlen, 0u, rst, 6u, true);
    }
}
FG_WVH uint64_t write_steps(uint64_t n) { return (n + kRowsPerWave - 1u) / kRowsPerWave; }

// ---- the wrapper: member m's gzip bytes z[z_off[m] .. z_off[m + 1]) behind a header with attributes = 1, nothing for an empty member.
// One piece (global index g; piece_first[n_members + 1] = the scan of pieces_of) into its place by one wave, its register to piece_crc[g].
FG_WV void wrap_piece(const uint8_t* z, const uint64_t* z_off, const uint64_t* piece_first, uint64_t n_members, uint64_t g, const uint64_t* w_off,
                      uint8_t* w, uint64_t w_cap, uint32_t* piece_crc, const Lds& s) {
    const uint64_t m = fg::deflate::member_of(piece_first, n_members, g), j = g - piece_first[m];
    const uint64_t z0 = z_off[m], zlen = z_off[m + 1] - z0, at = j * kPiece;
    const uint64_t w0 = w_off[m], w1 = w_off[m + 1];
    if (at >= zlen || w1 > w_cap || w1 < w0 || w1 - w0 != kOverhead + zlen) return;  // (never: the offsets are the scan of these sizes.  Wave-uniform)
    const uint32_t len = (uint32_t)(zlen - at < kPiece ? zlen - at : kPiece);
    const uint32_t st = copy_crc(w + w0 + kOverhead + at, z + z0 + at, len, 0u, 6u, s);
    if (wv::lane() == wv::kLanes - 1u) piece_crc[g] = st;
}
// ... and per member, by one lane: the pieces' registers folded behind the header's, the header
FG_WVH void wrap_finish(const uint64_t* z_off, const uint64_t* piece_first, uint64_t m, const uint32_t* piece_crc, const uint64_t* w_off, uint8_t* w,
                        uint64_t w_cap) {
    const uint64_t zlen = z_off[m + 1] - z_off[m], w0 = w_off[m], w1 = w_off[m + 1];
    if (zlen == 0u || zlen > kMaxValue || w1 > w_cap || w1 < w0 || w1 - w0 != kOverhead + zlen) return;
    const uint64_t p0 = piece_first[m], p1 = piece_first[m + 1];
    const uint32_t x_full = p1 - p0 > 1u ? x_pow8(kPiece) : 0u;
    uint32_t st = header_state_bits((uint32_t)zlen, 1u);
    for (uint64_t g = p0; g < p1; ++g) st = gf_mul(g + 1u == p1 ? x_pow8(zlen - (p1 - 1u - p0) * kPiece) : x_full, st) ^ piece_crc[g];
    for (uint32_t k = 0; k < kOverhead; ++k) w[w0 + k] = header_byte(k, (uint32_t)zlen, 1u, ~st);
}

}  // namespace kafka
}  // namespace fg
