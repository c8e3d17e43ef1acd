// fg_syslen.hpp -- framing an octet-counted stream (input.framing = "syslen", RFC 6587) without walking it front to back.  HIP-free:
// compiled by hipcc into fg_syslen.hip (launch code and nothing else lives there) and by g++ over the fiber emulation of a wave
// (tests/native/syslen_host.cpp), so the CPU suite runs what the kernels run.
//
// Reference: SyslenSplitter::run / read_msglen (src/flowgger/splitter/syslen_splitter.rs:17-57): "<len> " then exactly len bytes; the
// next frame starts behind them.  next(p) depends on the bytes at p, so the chain is serial -- it is broken by SPECULATION and
// stays exact:
//   1 resolve  one wave per kTile bytes, staged in LDS with a look-ahead of the prefix bound: every position of the tile where a
//              well-formed prefix starts is a CANDIDATE with a `next`.  Only the candidates whose next lies behind the tile (the EXITS)
//              matter to anybody else: the distinct exits (at most kExits) that land on a candidate are appended to the INBOX of the
//              tile they land in (at most kInbox entries); position 0 is the inbox of tile 0.  (Chains INSIDE a tile are not resolved
//              here: which of them matter is known only once the inboxes are, and stage 2 follows those few.)
//   2 walk     one lane per inbox entry walks its chain through its tile in global memory: where it leaves (or why it stops), the
//              frames it crosses and their payload bytes.  That is one NODE per reachable (tile, entry); its successor is the
//              inbox entry of the tile its exit lands in.
//   3 rank     the nodes form a forest; the chain from node 0 is the stream's.  ceil(log2(tiles)) rounds of pointer jumping give
//              every node ON that chain the frames and payload bytes before it (a marked node hands its sums to its 2^k-th successor
//              in round k, so every node of the chain is marked exactly once).
//   4 emit     the tile of a marked node walks from its true entry, writes frame starts and packed offsets at the ranked positions,
//              copies the payloads and sets the UTF-8 flags; the node that ends the chain writes n_frames / consumed / stop reason.
// A launch DECLINES (nothing is valid; the caller frames on the host) when a tile has more than kExits distinct exits or an inbox
// more than kInbox entries: payload text that looks like prefixes.  There is no spin and no wait on another wave anywhere.
#pragma once
#include "fg_syslen_parse.hpp"
#include "fg_wave.hpp"

namespace fg {
namespace syslen {

constexpr uint32_t kTile = 4096;      // bytes per wave of the resolve and emit stages
constexpr uint32_t kLook = 32;        // bytes staged behind the tile (>= kMaxPrefix, a multiple of 16)
constexpr uint32_t kRawExits = 256;   // exits of a tile before they are deduplicated
constexpr uint32_t kExits = 64;       // distinct exits of a tile
constexpr uint32_t kInbox = 16;       // entries of a tile anyone can reach
constexpr uint32_t kNil = 0xFFFFFFFFu;
constexpr uint64_t kMaxBytes = 0xFFFF0000ull;  // positions and sums are 32-bit words in the scratch
// (the result words of a launch, H_*: fg_syslen_parse.hpp)

// ---- device scratch: 32-bit words -------------------------------------------------------------------------------------------
struct Scratch {
    uint32_t* hdr;        // H_WORDS
    uint32_t* inbox_cnt;  // [tiles]
    uint32_t* mk_stamp;   // [nodes] 0 = not on the chain, else the round after which the node is known to be
    uint32_t* mk_f;       // [nodes] frames before the node
    uint32_t* mk_b;       // [nodes] payload bytes before the node
    uint32_t* inbox_pos;  // [nodes] node = tile * kInbox + slot
    uint32_t* nd_exit;    // [nodes] where the node's walk left its tile, or stopped
    uint32_t* nd_term;    // [nodes] kNil, or why it stopped (ST_*)
    uint32_t* jn[2];      // [nodes] 2^k-th successor (kNil: the chain ends before), double-buffered over the rounds
    uint32_t* jf[2];      // [nodes] frames up to it
    uint32_t* jb[2];      // [nodes] payload bytes up to it
    uint32_t tiles, rounds;
};
FG_WVH uint32_t tiles_of(uint64_t nbytes) { return (uint32_t)(nbytes / kTile) + 1u; }  // (position nbytes itself has a tile)
FG_WVH uint64_t scratch_words(uint64_t nbytes) { return H_WORDS + (uint64_t)tiles_of(nbytes) * (1u + 12u * kInbox); }
FG_WVH uint64_t scratch_zero_words(uint64_t nbytes) { return H_WORDS + (uint64_t)tiles_of(nbytes) * (1u + kInbox); }  // hdr, inbox_cnt, mk_stamp
FG_WVH Scratch carve(uint32_t* base, uint64_t nbytes) {
    Scratch s;
    s.tiles = tiles_of(nbytes);
    s.rounds = 0;
    while ((1ull << s.rounds) < s.tiles) ++s.rounds;
    const uint64_t n = (uint64_t)s.tiles * kInbox;
    uint32_t* p = base;
    s.hdr = p; p += H_WORDS;
    s.inbox_cnt = p; p += s.tiles;
    s.mk_stamp = p; p += n;
    s.mk_f = p; p += n;
    s.mk_b = p; p += n;
    s.inbox_pos = p; p += n;
    s.nd_exit = p; p += n;
    s.nd_term = p; p += n;
    for (int k = 0; k < 2; ++k) { s.jn[k] = p; p += n; s.jf[k] = p; p += n; s.jb[k] = p; p += n; }
    return s;
}

#if defined(__HIPCC__)
FG_WV uint32_t g_add32(uint32_t* p, uint32_t v) { return atomicAdd(p, v); }
FG_WV void g_or32(uint32_t* p, uint32_t v) { atomicOr(p, v); }
FG_WV void load16(const uint8_t* p, uint32_t q[4]) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
}
FG_WV void store16(uint8_t* p, const uint32_t q[4]) { *reinterpret_cast<uint4*>(p) = make_uint4(q[0], q[1], q[2], q[3]); }
#else
FG_WV uint32_t g_add32(uint32_t* p, uint32_t v) { const uint32_t o = *p; *p = o + v; return o; }
FG_WV void g_or32(uint32_t* p, uint32_t v) { *p |= v; }
FG_WV void load16(const uint8_t* p, uint32_t q[4]) { memcpy(q, p, 16); }
FG_WV void store16(uint8_t* p, const uint32_t q[4]) { memcpy(p, q, 16); }
#endif
// 16 bytes from any address (the payloads start anywhere)
FG_WV void load16u(const uint8_t* p, uint32_t q[4]) { __builtin_memcpy(q, p, 16); }

// LDS of the resolve kernel, in dwords
constexpr uint32_t kLdsBytes = (kTile + kLook) / 4u + 8u;  // the tile, its look-ahead, padding for Bytes::byte
constexpr uint32_t kLdsWords = kLdsBytes + kRawExits + 4u;

// How far the frame that starts at a position may reach.  One stream: the chunk's end, wherever the position is.  (The segmented
// framer, fg_syslen_multi.hpp, instantiates the stages below with the end of the SEGMENT that holds the position, and gives the
// segments' starts nodes of their own instead of the inbox entry of position 0.)
struct Whole {
    static constexpr bool kSegmented = false;
    uint64_t nbytes;
    struct Tile {
        uint64_t lim;
        FG_WV uint64_t limit(uint64_t) const { return lim; }
    };
    FG_WV Tile tile(uint64_t) const { return Tile{nbytes}; }
    FG_WV uint64_t limit(uint64_t) const { return nbytes; }
};

// ---- 1: resolve + route.  All 64 lanes; `lds` = kLdsWords dwords. ------------------------------------------------------------
template <class Span>
FG_WV void resolve_route(const uint8_t* bytes, uint64_t nbytes, uint32_t tile, const Scratch& sc, uint32_t* lds, const Span& span) {
    uint32_t* w = lds;
    uint32_t* raw = lds + kLdsBytes;
    uint32_t* ctr = raw + kRawExits;
    const uint32_t l = wv::lane();
    const uint64_t base = (uint64_t)tile * kTile;
    const uint64_t lim = (nbytes + 15ull) & ~15ull;
    for (uint32_t k = l; k < (kTile + kLook) / 16u; k += wv::kLanes) {
        uint32_t q[4] = {0u, 0u, 0u, 0u};
        if (base + (uint64_t)k * 16u < lim) load16(bytes + base + (uint64_t)k * 16u, q);
        w[4 * k] = q[0]; w[4 * k + 1] = q[1]; w[4 * k + 2] = q[2]; w[4 * k + 3] = q[3];
    }
    if (l == 0) { ctr[0] = 0u; ctr[1] = 0u; }
    wv::sync();
    const wv::Bytes tb{w};
    auto get = [&](uint64_t p) { return tb.byte((uint32_t)(p - base)); };
    const typename Span::Tile here = span.tile(base);
    // the candidates that leave the tile.  Positions are dealt out INTERLEAVED (lane l looks at 64 j + l): the 64 lanes of a step read
    // 16 consecutive dwords of the tile, four lanes each -- no LDS bank is asked twice
    for (uint32_t j = 0; j < kTile / wv::kLanes; ++j) {
        const uint32_t i = j * wv::kLanes + l;
        const uint32_t c = tb.byte(i);
        if (base + i >= nbytes || !(c == '+' || (c >= '0' && c <= '9'))) continue;
        const uint64_t lim = here.limit(base + i);
        const Prefix pr = parse_prefix(get, base + i, lim);
        if (pr.st != ST_VALID || (uint64_t)i + pr.plen + pr.len < kTile) continue;
        if (Span::kSegmented && base + i + pr.plen + pr.len == lim) continue;  // (ends on its segment's end: the end of a chain, no exit)
        const uint32_t k = wv::lds_add(&ctr[0], 1u);
        if (k < kRawExits) raw[k] = (uint32_t)(base + i + pr.plen + pr.len);
    }
    if (!Span::kSegmented && tile == 0 && l == 0) {  // the stream's own start
        sc.inbox_pos[0] = 0u;
        g_add32(&sc.inbox_cnt[0], 1u);
    }
    wv::sync();
    const uint32_t nraw = ctr[0];
    if (nraw > kRawExits) {
        if (l == 0) g_or32(&sc.hdr[H_DECLINE], 1u);
        return;
    }
    auto gget = [&](uint64_t p) { return (uint32_t)bytes[p]; };
    for (uint32_t e = l; e < nraw; e += wv::kLanes) {
        const uint32_t x = raw[e];
        bool uniq = true;
        for (uint32_t k = 0; k < e && uniq; ++k) uniq = raw[k] != x;
        if (!uniq) continue;
        if (wv::lds_add(&ctr[1], 1u) >= kExits) continue;
        // (one global read: an exit that does not land on a candidate ends there -- the node that takes it finds out by itself)
        if (x >= nbytes || parse_prefix(gget, x, span.limit(x)).st != ST_VALID) continue;
        const uint32_t t2 = x / kTile;
        const uint32_t slot = g_add32(&sc.inbox_cnt[t2], 1u);
        if (slot < kInbox) sc.inbox_pos[(uint64_t)t2 * kInbox + slot] = x;
        else g_or32(&sc.hdr[H_DECLINE], 2u);
    }
    wv::sync();
    if (l == 0 && ctr[1] > kExits) g_or32(&sc.hdr[H_DECLINE], 1u);
}
FG_WV void resolve_route(const uint8_t* bytes, uint64_t nbytes, uint32_t tile, const Scratch& sc, uint32_t* lds) {
    resolve_route(bytes, nbytes, tile, sc, lds, Whole{nbytes});
}

// the lowest slot of tile t2's inbox that holds position x (duplicates -- two tiles with the same exit -- collapse onto it)
FG_WV uint32_t inbox_find(const Scratch& sc, uint32_t t2, uint32_t x) {
    uint32_t n = sc.inbox_cnt[t2];
    if (n > kInbox) n = kInbox;
    for (uint32_t k = 0; k < n; ++k)
        if (sc.inbox_pos[(uint64_t)t2 * kInbox + k] == x) return t2 * kInbox + k;
    return kNil;
}

// ---- 2: one lane per node (no cross-lane primitive) ----------------------------------------------------------------------------
// the chain from x through its tile, `lim` = where the bytes x may use end; the node u it makes.  root: u starts a true chain.
FG_WV void walk_chain(const uint8_t* bytes, uint64_t lim, uint32_t tile, uint32_t u, uint32_t x, bool live, bool root, const Scratch& sc) {
    uint32_t next = kNil, term = kNil, frames = 0, pbytes = 0;
    uint64_t pos = x;
    if (live) {
        const uint64_t end = (uint64_t)(tile + 1u) * kTile;
        auto gget = [&](uint64_t p) { return (uint32_t)bytes[p]; };
        for (uint32_t hop = 0; hop <= kTile / 2u && pos < end; ++hop) {  // (a frame is two bytes at least)
            const Prefix pr = parse_prefix(gget, pos, lim);
            if (pr.st != ST_VALID) { term = pr.st; break; }
            ++frames;
            pbytes += (uint32_t)pr.len;
            pos += pr.plen + pr.len;
        }
        if (term == kNil) {
            if (pos >= lim) term = ST_CLEAN;
            else {
                next = inbox_find(sc, (uint32_t)(pos / kTile), (uint32_t)pos);
                if (next == kNil) term = parse_prefix(gget, pos, lim).st;  // (never ST_VALID unless an inbox ran over: declined then)
            }
        }
        if (root) { sc.mk_stamp[u] = 1u; sc.mk_f[u] = 0u; sc.mk_b[u] = 0u; }
    }
    sc.nd_exit[u] = (uint32_t)pos;
    sc.nd_term[u] = term;
    sc.jn[0][u] = next;
    sc.jf[0][u] = frames;
    sc.jb[0][u] = pbytes;
}
// one lane per inbox entry (slot = lane < kInbox)
FG_WV void walk_node(const uint8_t* bytes, uint64_t nbytes, uint32_t tile, uint32_t slot, const Scratch& sc) {
    uint32_t n = sc.inbox_cnt[tile];
    if (n > kInbox) n = kInbox;
    if (slot >= n) return;
    const uint32_t u = tile * kInbox + slot;
    const uint32_t x = sc.inbox_pos[u];
    // (a duplicate is nobody's successor: it stays an empty node)
    walk_chain(bytes, nbytes, tile, u, x, inbox_find(sc, tile, x) == u, u == 0, sc);
}

// ---- 3: round r = 1 .. rounds of the ranking, one thread per node -------------------------------------------------------------
FG_WV void jump_node(uint32_t u, uint32_t r, const Scratch& sc) {
    const uint32_t a = (r - 1u) & 1u, b = r & 1u;
    const uint32_t nx = sc.jn[a][u], f = sc.jf[a][u], pb = sc.jb[a][u];
    const uint32_t stamp = sc.mk_stamp[u];
    if (nx == kNil) {
        sc.jn[b][u] = kNil; sc.jf[b][u] = f; sc.jb[b][u] = pb;
        return;
    }
    if (stamp != 0u && stamp <= r) {  // on the chain since an earlier round: so is its 2^(r-1)-th successor (marked here and only here)
        sc.mk_f[nx] = sc.mk_f[u] + f;
        sc.mk_b[nx] = sc.mk_b[u] + pb;
        sc.mk_stamp[nx] = r + 1u;
    }
    sc.jn[b][u] = sc.jn[a][nx];
    sc.jf[b][u] = f + sc.jf[a][nx];
    sc.jb[b][u] = pb + sc.jb[a][nx];
}
FG_WV void jump_round(uint32_t tile, uint32_t slot, uint32_t r, const Scratch& sc) {
    uint32_t n = sc.inbox_cnt[tile];
    if (n > kInbox) n = kInbox;
    if (slot < n) jump_node(tile * kInbox + slot, r, sc);
}

// ---- 4: emit + pack.  All 64 lanes; `lds` = 4 * 64 + 4 dwords. ------------------------------------------------------------------
constexpr uint32_t kEmitLdsWords = 4u * 64u + 4u;
// the payload src[0 .. len) -> dst, by the whole wave; returns (to every lane that saw one) whether it is valid UTF-8
FG_WV bool copy_check(const uint8_t* src, uint8_t* dst, uint32_t len) {
    const uint32_t l = wv::lane();
    bool bad = false;
    const uint32_t head = (uint32_t)((16u - ((uintptr_t)dst & 15u)) & 15u);  // bytes before dst is 16-byte aligned
    const uint32_t h = head < len ? head : len;
    for (uint32_t i = l; i < h + 1u; i += wv::kLanes) {  // (position h: a sequence cut off at the end of a payload shorter than the head)
        if (i > len || (i == h && h != len)) continue;
        const uint32_t b = i < len ? src[i] : 0u;
        if (i < len) dst[i] = (uint8_t)b;
        const uint32_t p1 = i >= 1u ? src[i - 1u] : 0u;
        if ((b | p1) & 0x80u) bad |= utf8::err_at(b, p1, i >= 2u ? src[i - 2u] : 0u, i >= 3u ? src[i - 3u] : 0u);
    }
    for (uint32_t i = h + l * 16u; i < len; i += wv::kLanes * 16u) {
        const uint32_t nb = len - i >= 16u ? 16u : len - i;
        uint32_t q[4] = {0u, 0u, 0u, 0u};
        if (nb == 16u) {
            load16u(src + i, q);
            store16(dst + i, q);
        } else {
            for (uint32_t k = 0; k < nb; ++k) {
                const uint32_t b = src[i + k];
                dst[i + k] = (uint8_t)b;
                q[k >> 2] |= b << (8u * (k & 3u));
            }
        }
        const uint32_t before = i >= 1u ? src[i - 1u] : 0u;
        if (((q[0] | q[1] | q[2] | q[3]) & 0x80808080u) | (before & 0x80u)) {
            uint32_t p1 = before, p2 = i >= 2u ? src[i - 2u] : 0u, p3 = i >= 3u ? src[i - 3u] : 0u;
            const uint32_t upto = i + nb == len ? nb + 1u : nb;  // the lane of the payload's last bytes also looks at position len
            for (uint32_t k = 0; k < upto; ++k) {
                const uint32_t b = k < nb ? (q[k >> 2] >> (8u * (k & 3u))) & 0xFFu : 0u;
                bad |= utf8::err_at(b, p1, p2, p3);
                p3 = p2; p2 = p1; p1 = b;
            }
        }
    }
    return bad;
}

// the frames of one chain from `pos` to the end of its tile (`end`) or of the chain: starts, offsets, payloads, flags from frame index
// `frame` and packed offset `pb` on.  lim as walk_chain.  Wave-uniform arguments.
FG_WV void emit_chain(const uint8_t* bytes, uint64_t lim, uint64_t end, uint64_t pos, uint32_t frame, uint32_t pb, uint8_t* packed,
                      uint64_t* offsets, uint64_t* starts, uint8_t* bad, uint64_t cap, uint32_t* lds) {
    uint32_t* f_pos = lds;  // a strip of up to 64 frames: start, prefix length, payload length, packed offset
    uint32_t* f_plen = lds + 64;
    uint32_t* f_len = lds + 128;
    uint32_t* f_dst = lds + 192;
    uint32_t* st = lds + 256;  // [0] frames in the strip, [1] where the walk stands, [2] ST_* that ended it or kNil
    const uint32_t l = wv::lane();
    auto gget = [&](uint64_t p) { return (uint32_t)bytes[p]; };
    for (uint32_t strip = 0; strip <= kTile / 128u; ++strip) {
        if (l == 0) {
            uint32_t k = 0, term = kNil;
            uint64_t p = pos;
            uint32_t d = pb;
            while (k < 64u && p < end) {
                const Prefix pr = parse_prefix(gget, p, lim);
                if (pr.st != ST_VALID) { term = pr.st; break; }
                f_pos[k] = (uint32_t)p; f_plen[k] = pr.plen; f_len[k] = (uint32_t)pr.len; f_dst[k] = d;
                d += (uint32_t)pr.len;
                p += pr.plen + pr.len;
                ++k;
            }
            st[0] = k; st[1] = (uint32_t)p; st[2] = term;
        }
        wv::sync();
        const uint32_t k = st[0];
        const uint32_t term = st[2];
        pos = st[1];
        if (l < k && (uint64_t)frame + l < cap) {
            starts[frame + l] = f_pos[l];
            offsets[frame + l] = f_dst[l];
        }
        for (uint32_t j = 0; j < k; ++j) {
            if ((uint64_t)frame + j >= cap) break;
            if (copy_check(bytes + f_pos[j] + f_plen[j], packed + f_dst[j], f_len[j])) bad[frame + j] = 1;
        }
        if (k) pb = f_dst[k - 1u] + f_len[k - 1u];
        frame += k;
        wv::sync();
        if (term != kNil || pos >= end || k < 64u) break;
    }
}
// the marked entry of a tile's inbox (the one place where a true chain enters it), or kNil
FG_WV uint32_t marked_entry(uint32_t tile, const Scratch& sc) {
    const uint32_t l = wv::lane();
    uint32_t n = sc.inbox_cnt[tile];
    if (n > kInbox) n = kInbox;
    const uint64_t mine = wv::ballot(l < n && sc.mk_stamp[(uint64_t)tile * kInbox + (l < n ? l : 0u)] != 0u);
    return mine == 0ull ? kNil : tile * kInbox + wv::ctz64(mine);
}

FG_WV void emit_tile(const uint8_t* bytes, uint64_t nbytes, uint32_t tile, const Scratch& sc, uint8_t* packed, uint64_t* offsets,
                     uint64_t* starts, uint8_t* bad, uint64_t cap, uint32_t* lds) {
    const uint32_t l = wv::lane();
    if (sc.hdr[H_DECLINE] != 0u) return;  // (nothing is valid: write nothing)
    const uint32_t u = marked_entry(tile, sc);
    if (u == kNil) return;  // the chain does not enter this tile
    emit_chain(bytes, nbytes, (uint64_t)(tile + 1u) * kTile, sc.inbox_pos[u], sc.mk_f[u], sc.mk_b[u], packed, offsets, starts, bad, cap, lds);
    // the node that ends the chain reports for the stream
    if (l == 0 && sc.nd_term[u] != kNil) {
        const uint32_t total_f = sc.mk_f[u] + sc.jf[0][u], total_b = sc.mk_b[u] + sc.jb[0][u];
        sc.hdr[H_STOP] = sc.nd_term[u];
        sc.hdr[H_NFRAMES] = total_f;
        sc.hdr[H_CONSUMED] = sc.nd_exit[u];
        sc.hdr[H_TOTAL] = total_b;
        sc.hdr[H_DONE] = 1u;
        if (total_f <= cap) {
            starts[total_f] = sc.nd_exit[u];
            offsets[total_f] = total_b;
        }
    }
}

}  // namespace syslen
}  // namespace fg
