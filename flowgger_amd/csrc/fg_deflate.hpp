// fg_deflate.hpp -- the output side's compressor: gzip members (RFC 1952) around raw deflate (RFC 1951: fixed-Huffman blocks from a
// greedy LZ77 parse, or stored blocks) over a resident byte buffer cut into members.  No HIP beyond fg_wave.hpp's vocabulary: hipcc
// compiles it into the kernels of fg_deflate.hip and g++ into tests/native/deflate_host.cpp, where a wave is 64 fibers, so the CPU
// suite runs what the GPU runs and both produce the same bytes.
//
// A member is cut into blocks of at most kBlock bytes and ONE WAVE compresses one block; blocks share nothing (the hash table is
// cleared per block, no match leaves its block), so a batch is as parallel as it has blocks.  Every block but a member's last ends on
// a byte boundary of the deflate stream (the empty stored block 00 00 ff ff of a sync flush behind a fixed block; a stored block ends
// on one anyway), which is what lets the blocks of a member be produced apart and packed back to back.
//
// A step of compress_block() takes the 64 positions [w, w + 64) of the block, one per lane:
//   hash      the lane's four bytes -> a slot of the LDS table; the candidate is READ, then (behind a barrier) every lane publishes
//             its own position with an LDS max.  Candidates therefore come from earlier steps only and the table after a step is the
//             per-slot maximum of what was there and what the step published: nothing depends on the order the hardware runs lanes in.
//   extend    the candidate and the distance-1 candidate (a run) are compared eight bytes at a time, bounded by 258 and the block's
//             end; the source is the input itself, so distance < length needs nothing special.  Minimum match 4.
//   select    greedy: next[p] = p + max(1, len[p]).  The positions on the chain from the window's first one are found by pointer
//             doubling (<= 6 rounds: the lanes on the chain mark their 2^r-th successor in an LDS bitmap, every lane squares its
//             jump); the chain's exit is where the next window starts.  A window without a match skips this: every lane is on it.
//   emit      the lanes on the chain build their token (<= 31 bits, Huffman codes bit-reversed: they go in MSB first, extra bits LSB
//             first), a wave prefix sum of the bit counts gives each its offset, the tokens are OR-ed into an LDS bit buffer and the
//             whole dwords of it are stored to the block's slot, one dword a lane.
// The slot is len + kSlotPad bytes of scratch: a block that outgrows its stored form (len + 5) is given up at the end of the step
// where it does and comes out stored.  CRC-32 is per block (64 lane chunks, folded by multiplication with x^(8 tail) mod P) and the
// blocks' are folded the same way per member by finish_member(); the byte-wise CRC itself is fg_inflate.hpp's.
//
// Three passes over a batch, sizes being unknown up front (the encoders' shape): compress every block into its slot -> per member,
// the blocks' offsets, the CRC and the size -> (scan) -> pack_block() copies each block behind its member's header.
#pragma once
#include <stdint.h>

#include "fg_inflate.hpp"
#include "fg_wave.hpp"

namespace fg {
namespace deflate {

constexpr uint32_t kBlock = 16384u;       // fg_deflate_block_bytes(): input bytes per block (and the farthest a match may reach)
constexpr uint32_t kHashBits = 12u;       // 4096 u32 slots = 16 KiB of LDS per wave
constexpr uint32_t kHashSize = 1u << kHashBits;
constexpr uint32_t kSmallBits = 9u;       // ... of which a block of at most kSmallLen bytes clears and uses 512
constexpr uint32_t kSmallLen = 2048u;
constexpr uint32_t kBufWords = 68u;       // the bit buffer: < 32 carried bits + 64 tokens of <= 31 bits, and the epilogue
constexpr uint32_t kMiscWords = 4u;       // chain bitmap (2), the chain's exit, the CRC fold
constexpr uint32_t kLdsWords = kHashSize + kBufWords + kMiscWords;
constexpr uint32_t kMinMatch = 4u, kMaxMatch = 258u;
constexpr uint32_t kSlotPad = 320u;       // slot bytes beyond the block's length (see compress_block)
constexpr uint32_t kStored = 0x80000000u; // in a block's size word: it comes out stored
constexpr uint32_t kHeader = 10u, kTrailer = 8u;
constexpr uint64_t kMaxMember = 0x7FE00000ull;  // a member's bytes: its compressed size goes through the encoders' scan, which takes 31 bits

FG_WVH uint64_t blocks_of(uint64_t len) { return (len + kBlock - 1u) / kBlock; }
// whether cuts a, b bound a member the compressor takes
FG_WVH bool member_ok(uint64_t a, uint64_t b, uint64_t nbytes) { return a <= b && b <= nbytes && b - a < kMaxMember; }
// bytes that always suffice: the frame per member, five bytes per block over its input
FG_WVH uint64_t bound(uint64_t nbytes, uint64_t n_members) {
    return nbytes + (uint64_t)(kHeader + kTrailer) * n_members + 5ull * (nbytes / kBlock + n_members);
}
// where the slot of global block g, which starts at input byte `start`, lies in the slot scratch (4-aligned; disjoint because
// starts ascend), and what the scratch holds for a batch
FG_WVH uint64_t slot_offset(uint64_t start, uint64_t g) { return (start & ~3ull) + g * kSlotPad; }
FG_WVH uint64_t slot_bytes(uint64_t nbytes, uint64_t n_blocks) { return nbytes + (n_blocks + 1u) * kSlotPad; }

struct Lds {
    uint32_t* table;  // kHashSize
    uint32_t* buf;    // kBufWords
    uint32_t* misc;   // kMiscWords
};
FG_WV Lds lds_of(uint32_t* base) { return Lds{base, base + kHashSize, base + kHashSize + kBufWords}; }

FG_WV uint32_t ld32(const uint8_t* p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
FG_WV uint64_t ld64(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return v;
}

// ---- CRC-32 in pieces: crc(A || B) = crc(A) * x^(8 |B|) mod P  xor  crc(B), in the reflected representation zlib uses
FG_WVH uint32_t gf_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t i = 0; i < 32u; ++i) {
        p ^= b & (0u - ((a >> (31u - i)) & 1u));
        b = (b >> 1) ^ (0xEDB88320u & (0u - (b & 1u)));
    }
    return p;
}
FG_WVH uint32_t x_pow8(uint64_t n) {  // x^(8 n) mod P
    uint32_t r = 0x80000000u, base = 0x00800000u;
    while (n) {
        if (n & 1u) r = gf_mul(r, base);
        base = gf_mul(base, base);
        n >>= 1;
    }
    return r;
}
FG_WVH uint32_t crc_bytes(const uint8_t* p, uint32_t n) {
    fg::inflate::Sums s{1u, 0u, 0xFFFFFFFFu};
    for (uint32_t k = 0; k < n; ++k) s.add(p[k], true);
    return s.crc ^ 0xFFFFFFFFu;
}

// ---- tokens
FG_WV uint32_t rev_bits(uint32_t x, uint32_t n) {  // the low n <= 16 bits of x, reversed
    x = ((x & 0x5555u) << 1) | ((x >> 1) & 0x5555u);
    x = ((x & 0x3333u) << 2) | ((x >> 2) & 0x3333u);
    x = ((x & 0x0F0Fu) << 4) | ((x >> 4) & 0x0F0Fu);
    x = ((x & 0x00FFu) << 8) | ((x >> 8) & 0x00FFu);
    return x >> (16u - n);
}
FG_WV uint32_t log2u(uint32_t x) { return 31u - (uint32_t)__builtin_clz(x); }  // x != 0
FG_WV uint32_t literal_token(uint32_t b, uint32_t* nbits) {
    if (b < 144u) {
        *nbits = 8u;
        return rev_bits(0x30u + b, 8u);
    }
    *nbits = 9u;
    return rev_bits(0x190u + (b - 144u), 9u);
}
// a match of len in 4 .. 258 at dist in 1 .. 32768, in stream order from bit 0
FG_WV uint32_t match_token(uint32_t len, uint32_t dist, uint32_t* nbits) {
    uint32_t sym, leb = 0, lex = 0;
    const uint32_t l = len - 3u;
    if (len == kMaxMatch) {
        sym = 285u;
    } else if (l < 8u) {
        sym = 257u + l;
    } else {
        leb = log2u(l) - 2u;
        sym = 257u + 4u * leb + (l >> leb);
        lex = l & ((1u << leb) - 1u);
    }
    uint32_t bits, n;
    if (sym < 280u) {
        bits = rev_bits(sym - 256u, 7u);
        n = 7u;
    } else {
        bits = rev_bits(0xC0u + (sym - 280u), 8u);
        n = 8u;
    }
    bits |= lex << n;
    n += leb;
    const uint32_t d = dist - 1u;
    uint32_t code = d, deb = 0, dex = 0;
    if (d >= 4u) {
        deb = log2u(d) - 1u;
        code = 2u * deb + (d >> deb);
        dex = d & ((1u << deb) - 1u);
    }
    bits |= rev_bits(code, 5u) << n;
    n += 5u;
    bits |= dex << n;
    n += deb;
    *nbits = n;
    return bits;
}

// how many bytes a[0 ..) and b[0 ..) share, at most maxl; reads nothing beyond either's first maxl bytes
FG_WV uint32_t match_len(const uint8_t* a, const uint8_t* b, uint32_t maxl) {
    uint32_t l = 0;
    while (l + 8u <= maxl) {
        const uint64_t d = ld64(a + l) ^ ld64(b + l);
        if (d) return l + (wv::ctz64(d) >> 3);
        l += 8u;
    }
    while (l < maxl && a[l] == b[l]) ++l;
    return l;
}

// One block by one wave: src[0 .. len), 1 <= len <= kBlock, into out32 (its slot: 4-aligned, len + kSlotPad bytes), last = the
// member's last block.  Returns (to every lane) the block's bytes in the deflate stream, | kStored when it comes out stored (then the
// slot's content is not used: the pack pass copies the input behind a five-byte header); *crc = the CRC-32 of src[0 .. len).
// Slot room: a step starts with at most len + 8 bytes stored (else the block is given up) and stores at most 63 dwords, the epilogue
// three more.
FG_WV uint32_t compress_block(const uint8_t* src, uint32_t len, bool last, uint32_t* out32, const Lds& s, uint32_t* crc) {
    const uint32_t l = wv::lane();
    const uint32_t hbits = len > kSmallLen ? kHashBits : kSmallBits;
    for (uint32_t k = l; k < (1u << hbits); k += wv::kLanes) s.table[k] = 0u;
    for (uint32_t k = l; k < kBufWords; k += wv::kLanes) s.buf[k] = 0u;
    if (l == 0u) {
        s.buf[0] = (last ? 1u : 0u) | 2u;  // BFINAL, BTYPE 01
        s.misc[3] = 0u;
    }
    wv::sync();
    {  // the CRC: 64 chunks, each shifted to its place
        const uint32_t c = (len + wv::kLanes - 1u) / wv::kLanes;
        const uint32_t a = l * c < len ? l * c : len, b = a + c < len ? a + c : len;
        if (b > a) wv::lds_xor(&s.misc[3], gf_mul(x_pow8(len - b), crc_bytes(src + a, b - a)));
    }
    uint32_t carry = 3u, outdw = 0u, w = 0u;
    bool given_up = false;
    while (w < len) {  // (wave-uniform: w, carry, outdw are)
        const uint32_t p = w + l;
        const bool valid = p < len, hashed = p + kMinMatch <= len;
        uint32_t v = 0, h = 0, cand = 0;
        if (hashed) {
            v = ld32(src + p);
            h = (v * 2654435761u) >> (32u - hbits);
            cand = s.table[h];  // position + 1 of an earlier step's, or 0
        }
        wv::sync();
        if (hashed) wv::lds_max(&s.table[h], p + 1u);
        uint32_t mlen = 0, mdist = 0;
        if (hashed) {
            const uint32_t maxl = len - p < kMaxMatch ? len - p : kMaxMatch;
            if (cand != 0u && ld32(src + cand - 1u) == v) {
                mlen = match_len(src + cand - 1u, src + p, maxl);
                mdist = p - (cand - 1u);
            }
            if (p >= 1u && v == (uint32_t)src[p - 1u] * 0x01010101u) {  // a run: the byte before repeats
                const uint32_t rl = match_len(src + p - 1u, src + p, maxl);
                if (rl >= mlen) {
                    mlen = rl;
                    mdist = 1u;
                }
            }
            if (mlen < kMinMatch) mlen = 0u;
        }
        // the greedy chain from the window's first position
        const uint32_t nxt = valid ? l + (mlen ? mlen : 1u) : wv::kLanes;
        bool on = true;
        uint32_t exit_at = w + wv::kLanes;
        const bool chained = wv::any(mlen != 0u);
        if (chained) {
            if (l < 2u) s.misc[l] = l == 0u ? 1u : 0u;
            wv::sync();
            uint32_t jmp = nxt < wv::kLanes ? nxt : wv::kLanes;
            uint64_t have = 1ull;
            on = l == 0u;
            for (uint32_t r = 0; r < 6u; ++r) {
                if (on && jmp < wv::kLanes) wv::lds_or(&s.misc[jmp >> 5], 1u << (jmp & 31u));
                wv::sync();
                const uint64_t m = (uint64_t)s.misc[0] | (uint64_t)s.misc[1] << 32;
                on = ((m >> l) & 1ull) != 0ull;
                if (m == have) break;
                have = m;
                const uint32_t j2 = wv::shfl(jmp, jmp & 63u);
                if (jmp < wv::kLanes) jmp = j2;
            }
            if (on && nxt >= wv::kLanes) s.misc[2] = w + nxt;  // (the chain's last lane, the only one)
        }
        // tokens -> bit offsets -> the bit buffer
        uint32_t nbits = 0, bits = 0;
        if (on && valid) bits = mlen ? match_token(mlen, mdist, &nbits) : literal_token(hashed ? v & 0xFFu : src[p], &nbits);
        uint32_t total;
        const uint32_t bp = carry + wv::excl_sum(nbits, &total);
        if (nbits) {
            wv::lds_or(&s.buf[bp >> 5], bits << (bp & 31u));
            if ((bp & 31u) + nbits > 32u) wv::lds_or(&s.buf[(bp >> 5) + 1u], bits >> (32u - (bp & 31u)));
        }
        wv::sync();
        const uint32_t t = carry + total, ndw = t >> 5;  // ndw <= 62
        if (l < ndw) out32[outdw + l] = s.buf[l];
        const uint32_t cw = s.buf[ndw];
        if (chained) exit_at = s.misc[2];
        if (exit_at < w + wv::kLanes) exit_at = w + wv::kLanes;  // (never: the chain's last lane leaves the window; the loop advances regardless)
        wv::sync();
        s.buf[l] = l == 0u ? cw : 0u;
        if (l < kBufWords - wv::kLanes) s.buf[wv::kLanes + l] = 0u;
        outdw += ndw;
        carry = t & 31u;
        w = exit_at;
        if (outdw * 4u > len + 8u) {
            given_up = true;
            break;
        }
    }
    wv::sync();
    *crc = s.misc[3];
    if (given_up) return (len + 5u) | kStored;
    // the end-of-block code (seven zero bits); then to a byte boundary, through an empty stored block unless the stream ends here
    uint32_t t = carry + 7u;
    if (!last) {
        t = ((t + 3u + 7u) & ~7u) + 16u;
        if (l == 0u) {
            s.buf[t >> 5] |= 0xFFFFu << (t & 31u);
            if ((t & 31u) > 16u) s.buf[(t >> 5) + 1u] |= 0xFFFFu >> (32u - (t & 31u));
        }
        t += 16u;
    } else {
        t = (t + 7u) & ~7u;
    }
    wv::sync();
    if (l < (t + 31u) >> 5) out32[outdw + l] = s.buf[l];
    wv::sync();
    const uint32_t size = outdw * 4u + (t >> 3);
    return size < len + 5u ? size : (len + 5u) | kStored;
}

// ---- per member, by one lane: where its blocks go, its CRC, its size.  first / end = the member's global block range, len its bytes;
// blk_size / blk_crc as compress_block left them; blk_rel[g] = block g's offset from the member's start.  Returns the member's bytes.
FG_WVH uint32_t finish_member(uint64_t first, uint64_t end, uint64_t len, const uint32_t* blk_size, const uint32_t* blk_crc, uint32_t* blk_rel,
                              uint32_t* crc_out) {
    if (end == first) {
        *crc_out = 0u;
        return 0u;
    }
    const uint32_t x_full = x_pow8(kBlock);
    uint32_t rel = kHeader, crc = 0u;
    for (uint64_t g = first; g < end; ++g) {
        blk_rel[g] = rel;
        rel += blk_size[g] & ~kStored;
        const bool tail = g + 1u == end;
        crc = gf_mul(tail ? x_pow8(len - (end - 1u - first) * kBlock) : x_full, crc) ^ blk_crc[g];
    }
    *crc_out = crc;
    return rel + kTrailer;
}

// dst[0 .. n) = src[0 .. n) by the wave: sixteen bytes a lane where dst is aligned, single bytes around that
struct alignas(16) Quad {
    uint32_t q[4];
};
FG_WV void wave_copy(uint8_t* dst, const uint8_t* src, uint32_t n) {
    const uint32_t l = wv::lane();
    uint32_t head = (16u - (uint32_t)((uintptr_t)dst & 15u)) & 15u;
    if (head > n) head = n;
    if (l < head) dst[l] = src[l];
    const uint32_t body = (n - head) & ~15u;
    for (uint32_t i = head + l * 16u; i < head + body; i += wv::kLanes * 16u) {
        Quad q;
        __builtin_memcpy(&q, src + i, 16);
        *(Quad*)(dst + i) = q;
    }
    const uint32_t i = head + body + l;
    if (i < n) dst[i] = src[i];
}

// the member of global block g: the last m with blk_first[m] <= g (blk_first[n_members] = the block count, g below it)
FG_WVH uint64_t member_of(const uint64_t* blk_first, uint64_t n_members, uint64_t g) {
    uint64_t lo = 0, hi = n_members;  // blk_first[lo] <= g < blk_first[hi]
    while (hi - lo > 1u) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (blk_first[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// One block into its place by one wave (the member's frame with its first and last block).  Writes only inside
// z[z_off[m] .. z_off[m + 1]) and only when that lies inside z_cap.
FG_WV void pack_block(const uint8_t* bytes, const uint64_t* cuts, const uint64_t* blk_first, uint64_t n_members, uint64_t g, const uint8_t* slots,
                      const uint32_t* blk_size, const uint32_t* blk_rel, const uint32_t* member_crc, const uint64_t* z_off, uint8_t* z,
                      uint64_t z_cap) {
    const uint32_t l = wv::lane();
    const uint64_t m = member_of(blk_first, n_members, g), j = g - blk_first[m], nblk = blk_first[m + 1] - blk_first[m];
    const uint64_t start = cuts[m] + j * kBlock, mlen = cuts[m + 1] - cuts[m];
    const uint32_t len = (uint32_t)(cuts[m + 1] - start < kBlock ? cuts[m + 1] - start : kBlock);
    const bool last = j + 1u == nblk;
    const uint32_t size = blk_size[g] & ~kStored, rel = blk_rel[g];
    const uint64_t z0 = z_off[m], z1 = z_off[m + 1];
    if (z1 > z_cap || z1 < z0 || (uint64_t)rel + size + (last ? kTrailer : 0u) > z1 - z0 || rel < kHeader) return;  // (never: the sizes are the scan's)
    uint8_t* dst = z + z0 + rel;
    if (j == 0u && l < kHeader) z[z0 + l] = l == 0u ? 0x1fu : l == 1u ? 0x8bu : l == 2u ? 8u : l == 9u ? 0xffu : 0u;
    if (blk_size[g] & kStored) {
        if (l < 5u) dst[l] = (uint8_t)(l == 0u ? (last ? 1u : 0u) : l == 1u ? len : l == 2u ? len >> 8 : l == 3u ? ~len : ~len >> 8);
        wave_copy(dst + 5u, bytes + start, len);
    } else {
        wave_copy(dst, slots + slot_offset(start, g), size);
    }
    if (last && l < kTrailer) {
        const uint32_t v = l < 4u ? member_crc[m] : (uint32_t)mlen;
        z[z1 - kTrailer + l] = (uint8_t)(v >> (8u * (l & 3u)));
    }
}

// ---- the two member policies over an encoder's out_offsets[n + 1] (fg_hip.h: fg_compress_cfg)
// coalesce = C >= 1: ceil(n / C) members by message index.  Entry k of member_first / cuts, k in 0 .. n_members.
FG_WVH uint64_t coalesce_members(uint64_t n, uint64_t c) { return (n + c - 1u) / c; }
FG_WVH void coalesce_cut(const uint64_t* off, uint64_t n, uint64_t c, uint64_t k, uint64_t* member_first, uint64_t* cuts) {
    const uint64_t i = k * c < n ? k * c : n;
    member_first[k] = i;
    cuts[k] = off[i];
}
// member_bytes = B: whether message i starts a member
FG_WVH bool bytes_starts(const uint64_t* off, uint64_t i, uint64_t b) { return i == 0u || off[i] / b > off[i - 1u] / b; }

}  // namespace deflate
}  // namespace fg
