// fg_deflate.hpp -- the output side's compressor: gzip members (RFC 1952) around raw deflate (RFC 1951: fixed-Huffman blocks from a
// greedy LZ77 parse, or stored blocks) over a resident byte buffer cut into members.  No HIP beyond fg_wave.hpp's vocabulary: hipcc
// compiles it into the kernels of fg_deflate.hip and g++ into tests/native/deflate_host.cpp, where a wave is 64 fibers, so the CPU
// suite runs what the GPU runs and both produce the same bytes.  That is FG_DEFLATE_FIXED, compress_block(); FG_DEFLATE_DYNAMIC
// (fg_set_deflate_mode) is compress_block_dyn() further down: dynamic-Huffman blocks where they are the smallest form.
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

// ---- FG_DEFLATE_DYNAMIC: every block as the cheapest of stored, fixed Huffman and dynamic Huffman (BTYPE 10), by two passes over the same
// greedy parse.  compress_block() above is the fixed mode and stays as it is; what follows shares its token rules and nothing else.
//   pass 1    parse_step() per window, nothing emitted: the tokens are counted into an LDS histogram (286 literal/length and 30 distance
//             counters, end-of-block once) and their extra bits summed.  The parse is a pure function of the input.
//   build     build_lengths() per alphabet: leaves ranked by (frequency, symbol), the two-queue Huffman merge (ties take the leaf, which
//             gives the shallowest of the optimal trees), depths clamped to the limit and the Kraft sum repaired as zlib's gen_bitlen
//             does; lengths go to the leaves in rank order.  Then the lengths of both codes run-length coded with 16 / 17 / 18 and the
//             code-length code built the same way (limit 7).  All of it a function of the histogram alone.
//   choice    both costs are exact before a bit is written: dynamic iff dyn_bits < fixed_bits, then the stored rule on the chosen form.
//   pass 2    the header, then the same parse again with the chosen table (code and length per symbol in LDS, the fixed codes when the
//             block chose them: such a block has the bytes compress_block() gives it), tokens of up to 48 bits.
// The hash table is dead between the passes: the build's workspace lies in it, the header goes out before pass 2 clears it.
// Slot room: the block's size is known before pass 2 and pass 2 runs only when size < len + 5, so the dwords stored end below
// size + 4 <= len + 8 bytes -- inside the len + kSlotPad of every slot, whatever a step carries.  emit_step() checks each store against the
// slot's end all the same.
constexpr uint32_t kLitSyms = 286u, kDistSyms = 30u, kClSyms = 19u;
constexpr uint32_t kSymWords = kLitSyms + kDistSyms;  // the histogram, then the lengths, then code | length << 16 per symbol
constexpr uint32_t kDynBufWords = 100u;               // the bit buffer: < 32 carried bits + 64 tokens of <= 48 bits = 97 whole dwords and a part, and the epilogue
constexpr uint32_t kDynLdsWords = kHashSize + kDynBufWords + kMiscWords + kSymWords;
constexpr uint32_t kLimLit = 1u, kLimDist = 2u, kLimCl = 4u;  // *info of compress_block_dyn: which codes the limiter shortened; the block's BTYPE << 4
// the workspace inside the hash table (words)
constexpr uint32_t kWsOrder = 0u, kWsNode = 288u, kWsPar = 576u, kWsKids = 864u, kWsFreq = 1152u, kWsBl = 1440u;  // build_lengths: 288 words each, then 17
constexpr uint32_t kWsBuild = 1460u;                                                                            // ... what build_lengths takes in all
constexpr uint32_t kWsCl = 1460u, kWsClCode = 1480u, kWsRle = 1500u, kWsScal = 1816u, kWsWords = 1824u;
static_assert(kWsWords <= kHashSize, "the workspace lies inside the hash table");

struct DynLds {
    uint32_t* table;  // kHashSize
    uint32_t* buf;    // kDynBufWords
    uint32_t* misc;   // kMiscWords
    uint32_t* sym;    // kSymWords
};
FG_WV DynLds dyn_lds_of(uint32_t* base) {
    return DynLds{base, base + kHashSize, base + kHashSize + kDynBufWords, base + kHashSize + kDynBufWords + kMiscWords};
}
FG_WV uint32_t wave_sum(uint32_t v) {
    uint32_t t;
    wv::excl_sum(v, &t);
    return t;
}
// the symbol of a match length 4 .. 258 / a distance 1 .. 32768, the count and the value of its extra bits (match_token's rules)
FG_WV uint32_t len_symbol(uint32_t len, uint32_t* eb, uint32_t* ex) {
    const uint32_t l = len - 3u;
    *eb = *ex = 0u;
    if (len == kMaxMatch) return 285u;
    if (l < 8u) return 257u + l;
    const uint32_t b = log2u(l) - 2u;
    *eb = b;
    *ex = l & ((1u << b) - 1u);
    return 257u + 4u * b + (l >> b);
}
FG_WV uint32_t dist_symbol(uint32_t dist, uint32_t* eb, uint32_t* ex) {
    const uint32_t d = dist - 1u;
    *eb = *ex = 0u;
    if (d < 4u) return d;
    const uint32_t b = log2u(d) - 1u;
    *eb = b;
    *ex = d & ((1u << b) - 1u);
    return 2u * b + (d >> b);
}
FG_WV uint32_t fixed_len(uint32_t k) { return k < 144u ? 8u : k < 256u ? 9u : k < 280u ? 7u : k < kLitSyms ? 8u : 5u; }  // k over both alphabets
// RFC 1951 3.2.7: the order the code-length code's lengths are sent in (five bits an entry)
FG_WV uint32_t clen_order(uint32_t k) {
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 |
                        11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((k < 12u ? lo >> (5u * k) : hi >> (5u * (k - 12u))) & 31u);
}

// One window of the greedy parse, exactly compress_block()'s: what this lane's position holds and whether it is a token.
struct Step {
    uint32_t mlen, mdist, lit, next;  // a match (mlen != 0) or the literal; next = where the following window starts (wave-uniform)
    bool tok;
};
FG_WV Step parse_step(const uint8_t* src, uint32_t len, uint32_t w, uint32_t hbits, uint32_t* table, uint32_t* misc) {
    const uint32_t l = wv::lane();
    const uint32_t p = w + l;
    const bool valid = p < len, hashed = p + kMinMatch <= len;
    uint32_t v = 0, h = 0, cand = 0;
    if (hashed) {
        v = ld32(src + p);
        h = (v * 2654435761u) >> (32u - hbits);
        cand = table[h];
    }
    wv::sync();
    if (hashed) wv::lds_max(&table[h], p + 1u);
    uint32_t mlen = 0, mdist = 0;
    if (hashed) {
        const uint32_t maxl = len - p < kMaxMatch ? len - p : kMaxMatch;
        if (cand != 0u && ld32(src + cand - 1u) == v) {
            mlen = match_len(src + cand - 1u, src + p, maxl);
            mdist = p - (cand - 1u);
        }
        if (p >= 1u && v == (uint32_t)src[p - 1u] * 0x01010101u) {
            const uint32_t rl = match_len(src + p - 1u, src + p, maxl);
            if (rl >= mlen) {
                mlen = rl;
                mdist = 1u;
            }
        }
        if (mlen < kMinMatch) mlen = 0u;
    }
    const uint32_t nxt = valid ? l + (mlen ? mlen : 1u) : wv::kLanes;
    bool on = true;
    uint32_t exit_at = w + wv::kLanes;
    const bool chained = wv::any(mlen != 0u);
    if (chained) {
        if (l < 2u) misc[l] = l == 0u ? 1u : 0u;
        wv::sync();
        uint32_t jmp = nxt < wv::kLanes ? nxt : wv::kLanes;
        uint64_t have = 1ull;
        on = l == 0u;
        for (uint32_t r = 0; r < 6u; ++r) {
            if (on && jmp < wv::kLanes) wv::lds_or(&misc[jmp >> 5], 1u << (jmp & 31u));
            wv::sync();
            const uint64_t m = (uint64_t)misc[0] | (uint64_t)misc[1] << 32;
            on = ((m >> l) & 1ull) != 0ull;
            if (m == have) break;
            have = m;
            const uint32_t j2 = wv::shfl(jmp, jmp & 63u);
            if (jmp < wv::kLanes) jmp = j2;
        }
        if (on && nxt >= wv::kLanes) misc[2] = w + nxt;
    }
    wv::sync();  // (the table and the exit are every lane's from here)
    if (chained) exit_at = misc[2];
    if (exit_at < w + wv::kLanes) exit_at = w + wv::kLanes;  // (never; the loop advances regardless)
    return Step{mlen, mdist, hashed ? v & 0xFFu : valid ? (uint32_t)src[p] : 0u, exit_at, on && valid};
}

// the lesser head of the two queues (the leaves' frequencies in rank order; the internal nodes in the order they were made); a tie takes the leaf
FG_WV uint32_t take_least(const uint32_t* sf, uint32_t used, uint32_t* li, const uint32_t* nf, uint32_t* par, uint32_t* ni, uint32_t nn, uint32_t* kids) {
    const uint32_t lf = sf[*li < used ? *li : 0u], hf = nf[*ni];  // (two independent reads; either may be unused)
    if (*li < used && (*ni >= nn || lf <= hf)) {
        ++*kids;
        ++*li;
        return lf;
    }
    par[(*ni)++] = nn;
    return hf;
}
// Length-limited prefix code by the wave: f[0 .. n) holds frequencies and comes back as code lengths: 0 iff the frequency is 0; one used
// symbol gets length 1; else the Kraft sum is exactly 1 and no length exceeds limit.  n <= 286, n <= 2^limit, limit <= 15, the frequencies'
// sum below 2^24.  ws: kWsBuild words.  Returns the sum of frequency * length; *limited = the limiter changed the Huffman lengths.
FG_WV uint32_t build_lengths(uint32_t* f, uint32_t n, uint32_t limit, uint32_t* ws, bool* limited) {
    const uint32_t l = wv::lane();
    uint32_t *order = ws + kWsOrder, *nf = ws + kWsNode, *par = ws + kWsPar, *kid = ws + kWsKids, *sf = ws + kWsFreq, *bl = ws + kWsBl;
    uint32_t *cs = par, *cf = kid;  // the used symbols in symbol order and their frequencies (dead once they are ranked)
    uint32_t used = 0;
    for (uint32_t base = 0; base < n; base += wv::kLanes) {
        const uint32_t s = base + l, fs = s < n ? f[s] : 0u;
        const uint64_t m = wv::ballot(fs != 0u);
        if (fs != 0u) {
            const uint32_t j = used + wv::mbcnt(m);
            cs[j] = s;
            cf[j] = fs;
        }
        used += wv::popc64(m);
    }
    if (l <= 16u) bl[l] = 0u;  // bl[1 .. 15]: leaves per length; bl[16]: limited
    wv::sync();
    for (uint32_t j = l; j < used; j += wv::kLanes) {  // rank by (frequency, symbol); every lane reads the same word at a time, a broadcast
        const uint32_t fs = cf[j];
        uint32_t r = 0;
        for (uint32_t t = 0; t < used; ++t) {
            const uint32_t ft = cf[t];
            r += (ft < fs || (ft == fs && t < j)) ? 1u : 0u;
        }
        order[r] = cs[j];
        sf[r] = fs;
    }
    wv::sync();
    if (l == 0u && used == 1u) bl[1] = 1u;
    if (l == 0u && used >= 2u) {
        // the two-queue merge: nn internal nodes so far, and used - nn >= 2 items left in the queues in front of every merge
        uint32_t li = 0, ni = 0;
        for (uint32_t nn = 0; nn + 1u < used; ++nn) {
            uint32_t kids = 0;
            const uint32_t a = take_least(sf, used, &li, nf, par, &ni, nn, &kids);
            const uint32_t b = take_least(sf, used, &li, nf, par, &ni, nn, &kids);
            nf[nn] = a + b;
            kid[nn] = kids;
        }
        // depths from the root down (a parent was made after its children: it has the higher index); nf becomes the node's depth.  A
        // leaf below the limit is counted at the limit.
        const uint32_t root = used - 2u;
        nf[root] = 0u;
        bl[1] = kid[root];
        for (uint32_t i = root; i-- > 0u;) {
            const uint32_t d = nf[par[i]] + 1u;
            nf[i] = d;
            bl[d + 1u < limit ? d + 1u : limit] += kid[i];
        }
        // The Kraft sum in units of 2^-limit.  Every node at depth limit with m >= 2 leaves below it weighed one unit and weighs m now, so
        // over = the sum of (m - 1), bl[limit] >= over + 1, and some leaf lies above the limit (n <= 2^limit leaves all at the limit would
        // not exceed 1).  zlib's repair, one unit a round: a leaf at the deepest level above the limit moves one down and takes a leaf
        // from the limit as its sibling.  bl[limit] - over never falls, so the limit's level never runs empty.
        uint32_t k = 0;
        for (uint32_t d = 1; d <= limit; ++d) k += bl[d] << (limit - d);
        uint32_t over = k - (1u << limit);
        bl[16] = over != 0u ? 1u : 0u;
        for (; over > 0u; --over) {
            uint32_t bits = limit - 1u;
            while (bits > 1u && bl[bits] == 0u) --bits;
            --bl[bits];
            bl[bits + 1u] += 2u;
            --bl[limit];
        }
    }
    wv::sync();
    // the longest lengths to the rarest symbols: rank j gets the length whose share of the ranks, counted from the limit down, holds j
    uint32_t cost = 0;
    for (uint32_t j = l; j < used; j += wv::kLanes) {
        uint32_t c = 0, d = limit;
        while (d > 1u && c + bl[d] <= j) c += bl[d--];
        cost += sf[j] * d;
        f[order[j]] = d;
    }
    *limited = bl[16] != 0u;
    cost = wave_sum(cost);
    wv::sync();
    return cost;
}
// canonical codes (RFC 1951 3.2.2) for lens[0 .. n): tab[s] = the code, bit-reversed | length << 16 (0 for an unused symbol).  tab may be lens.
FG_WV void assign_codes(const uint32_t* lens, uint32_t n, uint32_t* tab) {
    const uint32_t l = wv::lane();
    uint32_t cnt[16], next[16];  // (indexed by unrolled loops only: registers, wave-uniform)
#pragma unroll
    for (uint32_t d = 0; d < 16u; ++d) cnt[d] = 0u;
    for (uint32_t base = 0; base < n; base += wv::kLanes) {
        const uint32_t len = base + l < n ? lens[base + l] : 0u;
#pragma unroll
        for (uint32_t d = 1; d < 16u; ++d) cnt[d] += wv::popc64(wv::ballot(len == d));
    }
    next[0] = 0u;
#pragma unroll
    for (uint32_t d = 1; d < 16u; ++d) next[d] = (next[d - 1u] + cnt[d - 1u]) << 1;
    wv::sync();  // (tab may be lens: every length is read before a code is written)
    for (uint32_t base = 0; base < n; base += wv::kLanes) {
        const uint32_t len = base + l < n ? lens[base + l] : 0u;
        uint32_t code = 0;
#pragma unroll
        for (uint32_t d = 1; d < 16u; ++d) {
            const uint64_t m = wv::ballot(len == d);
            if (len == d) code = next[d] + wv::mbcnt(m);
            next[d] += wv::popc64(m);
        }
        if (base + l < n) tab[base + l] = len ? rev_bits(code, len) | len << 16 : 0u;
    }
    wv::sync();
}

// where the bits go: the slot, its end in dwords, the bits carried in buf[0] and the dwords stored so far
struct BitOut {
    uint32_t* out32;
    uint32_t lim, carry, outdw;
};
// One step of output by the wave: every lane's nbits <= 48 bits (0: none) in lane order behind what is carried; the whole dwords go to the slot.
FG_WV void emit_step(uint64_t bits, uint32_t nbits, uint32_t* buf, BitOut* o) {
    const uint32_t l = wv::lane();
    uint32_t total;
    const uint32_t bp = o->carry + wv::excl_sum(nbits, &total);
    if (nbits) {
        const uint32_t sh = bp & 31u, at = bp >> 5;
        const uint64_t lo = bits << sh;
        wv::lds_or(&buf[at], (uint32_t)lo);
        if (sh + nbits > 32u) wv::lds_or(&buf[at + 1u], (uint32_t)(lo >> 32));
        if (sh + nbits > 64u) wv::lds_or(&buf[at + 2u], (uint32_t)(bits >> (64u - sh)));  // (sh > 16 here)
    }
    wv::sync();
    const uint32_t t = o->carry + total, ndw = t >> 5;  // ndw <= 96
    if (l < ndw && o->outdw + l < o->lim) o->out32[o->outdw + l] = buf[l];
    if (wv::kLanes + l < ndw && o->outdw + wv::kLanes + l < o->lim) o->out32[o->outdw + wv::kLanes + l] = buf[wv::kLanes + l];
    const uint32_t cw = buf[ndw];
    wv::sync();
    buf[l] = l == 0u ? cw : 0u;
    if (wv::kLanes + l < kDynBufWords) buf[wv::kLanes + l] = 0u;
    wv::sync();
    o->outdw += ndw;
    o->carry = t & 31u;
}

// compress_block() for FG_DEFLATE_DYNAMIC, with its contract: one block by one wave into its slot, the size (| kStored) to every lane, *crc.
// *info = kLim* of the codes the limiter shortened | the block's BTYPE << 4 (tests; the kernel drops it).
FG_WV uint32_t compress_block_dyn(const uint8_t* src, uint32_t len, bool last, uint32_t* out32, const DynLds& s, uint32_t* crc, uint32_t* info) {
    const uint32_t l = wv::lane();
    const uint32_t hbits = len > kSmallLen ? kHashBits : kSmallBits;
    uint32_t* ws = s.table;
    for (uint32_t k = l; k < (1u << hbits); k += wv::kLanes) s.table[k] = 0u;
    for (uint32_t k = l; k < kDynBufWords; k += wv::kLanes) s.buf[k] = 0u;
    for (uint32_t k = l; k < kSymWords; k += wv::kLanes) s.sym[k] = 0u;
    if (l == 0u) s.misc[3] = 0u;
    wv::sync();
    {  // the CRC: 64 chunks, each shifted to its place
        const uint32_t c = (len + wv::kLanes - 1u) / wv::kLanes;
        const uint32_t a = l * c < len ? l * c : len, b = a + c < len ? a + c : len;
        if (b > a) wv::lds_xor(&s.misc[3], gf_mul(x_pow8(len - b), crc_bytes(src + a, b - a)));
    }
    // pass 1: the histogram and the extra bits
    uint32_t extra = 0;
    for (uint32_t w = 0; w < len;) {  // (wave-uniform; parse_step moves w on by at least a window)
        const Step t = parse_step(src, len, w, hbits, s.table, s.misc);
        uint32_t xb = 0;
        if (t.tok && t.mlen) {
            uint32_t leb, lex, deb, dex;
            wv::lds_add(&s.sym[len_symbol(t.mlen, &leb, &lex)], 1u);
            wv::lds_add(&s.sym[kLitSyms + dist_symbol(t.mdist, &deb, &dex)], 1u);
            xb = leb + deb;
        } else if (t.tok) {
            wv::lds_add(&s.sym[t.lit], 1u);
        }
        extra += wave_sum(xb);
        w = t.next;
    }
    wv::sync();
    if (l == 0u) s.sym[256] = 1u;  // end of block
    *crc = s.misc[3];
    wv::sync();
    // both costs, the codes
    uint32_t fx = 0;
    for (uint32_t k = l; k < kSymWords; k += wv::kLanes) fx += s.sym[k] * fixed_len(k);
    const uint32_t fixed_bits = 3u + wave_sum(fx) + extra;
    bool lim_lit, lim_dist, lim_cl;
    const uint32_t lit_cost = build_lengths(s.sym, kLitSyms, 15u, ws, &lim_lit);
    const uint32_t dist_cost = build_lengths(s.sym + kLitSyms, kDistSyms, 15u, ws, &lim_dist);
    // the two codes' lengths as one sequence, run-length coded (one lane: at most 316 steps): the entries (symbol | extra bits' value << 8),
    // their count, HLIT, HDIST, the repeat symbols' extra bits
    uint32_t *cl = ws + kWsCl, *clcode = ws + kWsClCode, *rle = ws + kWsRle, *scal = ws + kWsScal;
    if (l < kClSyms) cl[l] = 0u;
    wv::sync();
    if (l == 0u) {
        uint32_t hlit = kLitSyms, hdist = kDistSyms;
        while (hlit > 257u && s.sym[hlit - 1u] == 0u) --hlit;
        while (hdist > 1u && s.sym[kLitSyms + hdist - 1u] == 0u) --hdist;
        const uint32_t n = hlit + hdist;
        uint32_t cnt = 0, xbits = 0;
        for (uint32_t i = 0; i < n;) {  // (a run is at least one entry long: i moves on)
            const uint32_t v = s.sym[i < hlit ? i : kLitSyms + i - hlit];
            uint32_t run = 1;
            while (i + run < n && s.sym[i + run < hlit ? i + run : kLitSyms + i + run - hlit] == v) ++run;
            i += run;
            if (v != 0u) {  // the length itself, then repeats of three to six
                rle[cnt++] = v;
                ++cl[v];
                --run;
            }
            while (run >= 3u) {
                const uint32_t k = v != 0u ? (run < 6u ? run : 6u) : run < 138u ? run : 138u;
                const uint32_t sy = v != 0u ? 16u : k <= 10u ? 17u : 18u;
                rle[cnt++] = sy | (k - (sy == 18u ? 11u : 3u)) << 8;
                ++cl[sy];
                xbits += sy == 16u ? 2u : sy == 17u ? 3u : 7u;
                run -= k;
            }
            for (; run > 0u; --run) {
                rle[cnt++] = v;
                ++cl[v];
            }
        }
        scal[0] = cnt;
        scal[1] = hlit;
        scal[2] = hdist;
        scal[3] = xbits;
    }
    wv::sync();
    const uint32_t n_rle = scal[0], hlit = scal[1], hdist = scal[2], rle_extra = scal[3];
    const uint32_t cl_cost = build_lengths(cl, kClSyms, 7u, ws, &lim_cl);
    uint32_t hclen = kClSyms;
    while (hclen > 4u && cl[clen_order(hclen - 1u)] == 0u) --hclen;
    const uint32_t dyn_bits = 3u + 14u + 3u * hclen + cl_cost + rle_extra + lit_cost + dist_cost + extra;
    const bool dyn = dyn_bits < fixed_bits;
    const uint32_t bits = dyn ? dyn_bits : fixed_bits;
    const uint32_t size = last ? (bits + 7u) >> 3 : ((bits + 3u + 7u) >> 3) + 4u;  // (behind a non-last block: 000, to the byte, 00 00 ff ff)
    *info = (lim_lit ? kLimLit : 0u) | (lim_dist ? kLimDist : 0u) | (lim_cl ? kLimCl : 0u) | (size < len + 5u ? (dyn ? 2u : 1u) : 0u) << 4;
    if (size >= len + 5u) return (len + 5u) | kStored;
    // the header (it reads the workspace), then the table of the chosen codes
    BitOut o{out32, (len + kSlotPad) >> 2, 0u, 0u};
    if (dyn) {
        assign_codes(cl, kClSyms, clcode);
        uint32_t hb = 0, hn = 0;
        if (l == 0u) {
            hb = (last ? 1u : 0u) | 4u | (hlit - 257u) << 3 | (hdist - 1u) << 8 | (hclen - 4u) << 13;
            hn = 17u;
        } else if (l <= hclen) {
            hb = cl[clen_order(l - 1u)];
            hn = 3u;
        }
        emit_step(hb, hn, s.buf, &o);
        for (uint32_t base = 0; base < n_rle; base += wv::kLanes) {
            uint32_t eb = 0, en = 0;
            if (base + l < n_rle) {
                const uint32_t e = rle[base + l], sy = e & 0xFFu, c = clcode[sy];
                en = c >> 16;
                eb = (c & 0xFFFFu) | (e >> 8) << en;
                en += sy == 16u ? 2u : sy == 17u ? 3u : sy == 18u ? 7u : 0u;
            }
            emit_step(eb, en, s.buf, &o);
        }
        assign_codes(s.sym, kLitSyms, s.sym);
        assign_codes(s.sym + kLitSyms, kDistSyms, s.sym + kLitSyms);
    } else {
        emit_step((last ? 1u : 0u) | 2u, l == 0u ? 3u : 0u, s.buf, &o);
        for (uint32_t k = l; k < kSymWords; k += wv::kLanes) {
            const uint32_t code = k < 144u ? 0x30u + k : k < 256u ? 0x190u + (k - 144u) : k < 280u ? k - 256u : k < kLitSyms ? 0xC0u + (k - 280u) : k - kLitSyms;
            s.sym[k] = rev_bits(code, fixed_len(k)) | fixed_len(k) << 16;
        }
    }
    // pass 2: the same parse, the tokens from the table
    for (uint32_t k = l; k < (1u << hbits); k += wv::kLanes) s.table[k] = 0u;
    wv::sync();
    for (uint32_t w = 0; w < len;) {
        const Step t = parse_step(src, len, w, hbits, s.table, s.misc);
        uint64_t tb = 0;
        uint32_t tn = 0;
        if (t.tok && t.mlen) {
            uint32_t leb, lex, deb, dex;
            const uint32_t a = s.sym[len_symbol(t.mlen, &leb, &lex)], b = s.sym[kLitSyms + dist_symbol(t.mdist, &deb, &dex)];
            const uint32_t an = (a >> 16) + leb, bn = b >> 16;  // <= 20 and, with the extra bits, <= 28 bits
            tb = (uint64_t)((a & 0xFFFFu) | lex << (a >> 16)) | (uint64_t)((b & 0xFFFFu) | dex << bn) << an;
            tn = an + bn + deb;
        } else if (t.tok) {
            const uint32_t a = s.sym[t.lit];
            tb = a & 0xFFFFu;
            tn = a >> 16;
        }
        emit_step(tb, tn, s.buf, &o);
        w = t.next;
    }
    // end of block; then to a byte boundary, through an empty stored block unless the stream ends here
    emit_step(s.sym[256] & 0xFFFFu, l == 0u ? s.sym[256] >> 16 : 0u, s.buf, &o);
    uint32_t t = o.carry;
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
    if (l < (t + 31u) >> 5 && o.outdw + l < o.lim) out32[o.outdw + l] = s.buf[l];
    wv::sync();
    const uint32_t wrote = o.outdw * 4u + (t >> 3);  // (= size)
    return wrote < len + 5u ? wrote : (len + 5u) | kStored;
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
