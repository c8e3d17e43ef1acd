// fg_capnp_frame.hpp -- framing a Cap'n Proto stream (input.format = "capnp") without walking it front to back.  HIP-free: compiled by
// hipcc into fg_capnp_frame.hip (launch code and nothing else lives there) and by g++ over the fiber emulation of a wave
// (tests/native/capnp_frame_host.cpp), so the CPU suite runs what the kernels run.
//
// Reference: CapnpSplitter::run (src/flowgger/splitter/capnp_splitter.rs:24-46) calls capnp::serialize::read_message per message:
// a segment table (count - 1, the segments' sizes in words, padded to a word), then that many words; the next message starts
// behind them (fg_capnp_next.hpp restates the rule).  next(w) depends on the words at w, so the chain is serial -- it is broken by
// SPECULATION and stays exact.  EVERY 8-byte word is a candidate here, and false candidates are common (struct and list pointers
// read as small segment counts, zero words as empty messages), so nothing is capped per tile; the one bound is the node store:
//   1 mark     one wave per tile of kTileWords words, staged in LDS: every word resolves to the word its message ends at or to a
//              terminal (TAIL, TOO_MANY_SEGMENTS, TOO_LARGE, the end of the chunk).  A table that runs past the tile is read from
//              global memory.  The landing word of every hop that LEAVES the tile is marked in a bitmap, one bit per word of the
//              chunk; word 0 is marked by the launcher.
//   2 nodes    a tile with marked words resolves itself again, follows the chains inside the tile by pointer doubling in LDS
//              (9 rounds: a chain strictly advances, so it has at most 511 hops) and turns each marked word into a NODE: where its
//              chain leaves the tile or stops, why, and the messages it crosses.  A tile takes its nodes' slots, consecutive and in
//              word order, from a per-launch counter.
//   3 link     one thread per node: the node of the word its exit lands on (the tile's first slot + the rank of the bit).
//   4 rank     the nodes form a forest; the chain from word 0 is the stream's and visits a tile at most once.
//              ceil(log2(tiles)) rounds of pointer jumping give every node ON that chain the messages before it.
//   5 emit     the tile of a node on the chain resolves itself once more, one lane follows the chain through the tile in LDS and
//              the wave writes the offsets at the ranked positions; the node that ends the chain writes n / consumed / stop.
// A launch DECLINES (nothing is valid; the caller walks on the host) when the chunk has more nodes than words / kNodeDiv + kNodeMin.
// There is no spin and no wait on another wave anywhere; every loop is bounded by the tile's words, 511 sizes, or the round count.
#pragma once
#include "fg_capnp_next.hpp"
#include "fg_wave.hpp"

namespace fg {
namespace capnpf {

constexpr uint32_t kTileWords = 512;             // words per wave of the mark, nodes and emit stages
constexpr uint32_t kTileBytes = kTileWords * 8u;
constexpr uint32_t kBmWords = kTileWords / 32u;  // dwords of the bitmap per tile
constexpr uint32_t kDoubling = 9;                // 2^9 >= kTileWords
constexpr uint32_t kNodeDiv = 6;                 // the node store: one node per kNodeDiv words (4x the most measured), plus
constexpr uint32_t kNodeMin = 64;
constexpr uint32_t kNil = 0xFFFFFFFFu;
constexpr uint64_t kMaxBytes = 0xFFFF0000ull;    // word indices and a 3-bit kind share a 32-bit word of the scratch
constexpr uint32_t kKindShift = 29, kPosMask = (1u << kKindShift) - 1u;
enum { K_EXIT = 4, K_HOP = 5, K_END = 6 };       // kinds of a word beyond the four stop reasons: its message leaves / stays in the tile /
                                                 // ends exactly on its SEGMENT's end (fg_capnp_frame_multi.hpp only): counted, no exit, no hop
// (the result words of a launch, H_*: fg_capnp_next.hpp)

// ---- device scratch: 32-bit words -------------------------------------------------------------------------------------------
struct Scratch {
    uint32_t* hdr;         // H_WORDS
    uint32_t* bitmap;      // [tiles * kBmWords] bit w: some tile's exit lands on word w
    uint32_t* mk_stamp;    // [node_cap] 0 = not on the chain, else the round after which the node is known to be
    uint32_t* tile_first;  // [tiles] the tile's first node
    uint32_t* tile_cnt;    // [tiles] its nodes
    uint32_t* mk_f;        // [node_cap] messages before the node
    uint32_t* nd_pos;      // [node_cap] the marked word
    uint32_t* nd_fin;      // [node_cap] kind << 29 | the word its chain leaves the tile for (K_EXIT) or stops at (a stop reason)
    uint32_t* nd_cnt;      // [node_cap] messages its chain crosses
    uint32_t *jn0, *jn1;   // [node_cap] 2^k-th successor (kNil: the chain ends before), double-buffered over the rounds
    uint32_t *jf0, *jf1;   // [node_cap] messages up to it
    uint32_t tiles, rounds, node_cap;
};
FG_WVH uint32_t words_of(uint64_t nbytes) { return (uint32_t)(nbytes / 8u); }  // whole words; word words_of() is the chunk's end
FG_WVH uint32_t tiles_of(uint64_t nbytes) { return words_of(nbytes) / kTileWords + 1u; }
FG_WVH uint32_t node_cap_of(uint64_t nbytes) { return words_of(nbytes) / kNodeDiv + kNodeMin; }
FG_WVH uint64_t scratch_zero_words(uint64_t nbytes) { return H_WORDS + (uint64_t)tiles_of(nbytes) * kBmWords + node_cap_of(nbytes); }
FG_WVH uint64_t scratch_words(uint64_t nbytes) { return scratch_zero_words(nbytes) + 2ull * tiles_of(nbytes) + 8ull * node_cap_of(nbytes); }
FG_WVH Scratch carve(uint32_t* base, uint64_t nbytes) {
    Scratch s;
    s.tiles = tiles_of(nbytes);
    s.node_cap = node_cap_of(nbytes);
    s.rounds = 0;
    while ((1ull << s.rounds) < s.tiles) ++s.rounds;
    const uint64_t n = s.node_cap;
    uint32_t* p = base;
    s.hdr = p; p += H_WORDS;
    s.bitmap = p; p += (uint64_t)s.tiles * kBmWords;
    s.mk_stamp = p; p += n;
    s.tile_first = p; p += s.tiles;
    s.tile_cnt = p; p += s.tiles;
    s.mk_f = p; p += n;
    s.nd_pos = p; p += n;
    s.nd_fin = p; p += n;
    s.nd_cnt = p; p += n;
    s.jn0 = p; p += n;
    s.jn1 = p; p += n;
    s.jf0 = p; p += n;
    s.jf1 = p; p += n;
    return s;
}

#if defined(__HIPCC__)
FG_WV uint32_t g_add32(uint32_t* p, uint32_t v) { return atomicAdd(p, v); }
FG_WV void g_or32(uint32_t* p, uint32_t v) { atomicOr(p, v); }
FG_WV void load16(const uint8_t* p, uint32_t q[4]) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
}
FG_WV uint32_t load4(const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); }
#else
FG_WV uint32_t g_add32(uint32_t* p, uint32_t v) { const uint32_t o = *p; *p = o + v; return o; }
FG_WV void g_or32(uint32_t* p, uint32_t v) { *p |= v; }
FG_WV void load16(const uint8_t* p, uint32_t q[4]) { memcpy(q, p, 16); }
FG_WV uint32_t load4(const uint8_t* p) { uint32_t v; memcpy(&v, p, 4); return v; }
#endif

// What a word may reach to and which words start a stream: the whole chunk and word 0 here.  The segmented framer
// (fg_capnp_frame_multi.hpp) instantiates the stages below with the end of the SEGMENT that holds the word and every segment's start.
struct Whole {
    static constexpr bool kSegmented = false;
    uint64_t nbytes;
    struct Tile {
        uint64_t lim;
        FG_WV uint64_t limit(uint64_t) const { return lim; }
    };
    FG_WV Tile tile(uint64_t) const { return Tile{nbytes}; }
    FG_WV bool root(uint32_t w) const { return w == 0u; }
};

// LDS of the three tile stages, in dwords: the tile | nx | c | fin | the tile's bitmap slice, its prefix popcounts, four state words
constexpr uint32_t kLdsTile = kTileBytes / 4u;
constexpr uint32_t kLdsWords = kLdsTile + 3u * kTileWords + 2u * kBmWords + 4u;
struct Lds {
    uint32_t *tw, *nx, *c, *fin, *sb, *pre, *st;
};
FG_WV Lds lds_of(uint32_t* lds) {
    Lds r;
    r.tw = lds;
    r.nx = lds + kLdsTile;
    r.c = r.nx + kTileWords;
    r.fin = r.c + kTileWords;
    r.sb = r.fin + kTileWords;
    r.pre = r.sb + kBmWords;
    r.st = r.pre + kBmWords;
    return r;
}

// Every word i of the tile: nx[i] = the word of the tile its message ends at and c[i] = 1 (K_HOP), or nx[i] = i and c[i] = 0 (the
// message leaves the tile, K_EXIT, or none starts here: a stop reason); fin[i] = kind << 29 | that word (the word itself for a stop).
// All 64 lanes; ends with a barrier.
template <class Span>
FG_WV void resolve_tile(const uint8_t* bytes, uint64_t nbytes, uint32_t tile, const Lds& m, const Span& span) {
    const uint32_t l = wv::lane();
    const uint64_t base_w = (uint64_t)tile * kTileWords, base_b = base_w * 8ull, end_b = base_b + kTileBytes;
    const uint64_t lim = (nbytes + 15ull) & ~15ull;
    for (uint32_t k = l; k < kTileBytes / 16u; k += wv::kLanes) {
        uint32_t q[4] = {0u, 0u, 0u, 0u};
        if (base_b + (uint64_t)k * 16u < lim) load16(bytes + base_b + (uint64_t)k * 16u, q);
        m.tw[4 * k] = q[0]; m.tw[4 * k + 1] = q[1]; m.tw[4 * k + 2] = q[2]; m.tw[4 * k + 3] = q[3];
    }
    wv::sync();
    // (a table that runs past the tile: its sizes lie inside the chunk -- next_at checks that before it asks for them)
    auto get32 = [&](uint64_t p) { return p < end_b ? m.tw[(uint32_t)(p - base_b) >> 2] : load4(bytes + p); };
    const typename Span::Tile here = span.tile(base_b);
    for (uint32_t j = 0; j < kTileWords / wv::kLanes; ++j) {
        const uint32_t i = j * wv::kLanes + l;
        const uint64_t w = base_w + i;
        const uint64_t reach = here.limit(w * 8ull);  // the end of the chunk, or of the segment that holds w
        const Next r = next_at(get32, w, reach);
        uint32_t nx = i, c = 0u, fin = (r.st << kKindShift) | (uint32_t)w;
        if (r.st == ST_VALID) {
            const uint64_t x = w + r.words;
            if (Span::kSegmented && x * 8ull == reach) fin = ((uint32_t)K_END << kKindShift) | (uint32_t)x;
            else if (x < base_w + kTileWords) { nx = (uint32_t)(x - base_w); c = 1u; fin = ((uint32_t)K_HOP << kKindShift) | (uint32_t)x; }
            else fin = ((uint32_t)K_EXIT << kKindShift) | (uint32_t)x;
        }
        m.nx[i] = nx; m.c[i] = c; m.fin[i] = fin;
    }
    wv::sync();
}
FG_WV void resolve_tile(const uint8_t* bytes, uint64_t nbytes, uint32_t tile, const Lds& m) { resolve_tile(bytes, nbytes, tile, m, Whole{nbytes}); }

// ---- 1: mark.  All 64 lanes; `lds` = kLdsWords dwords. -------------------------------------------------------------------------
template <class Span>
FG_WV void mark_tile(const uint8_t* bytes, uint64_t nbytes, uint32_t tile, const Scratch& sc, uint32_t* lds, const Span& span) {
    const Lds m = lds_of(lds);
    resolve_tile(bytes, nbytes, tile, m, span);
    const uint32_t l = wv::lane();
    for (uint32_t j = 0; j < kTileWords / wv::kLanes; ++j) {
        const uint32_t f = m.fin[j * wv::kLanes + l];
        if ((f >> kKindShift) != (uint32_t)K_EXIT) continue;
        const uint32_t x = f & kPosMask;  // (<= words_of(nbytes): the message fits the chunk)
        g_or32(&sc.bitmap[x >> 5], 1u << (x & 31u));
    }
}
FG_WV void mark_tile(const uint8_t* bytes, uint64_t nbytes, uint32_t tile, const Scratch& sc, uint32_t* lds) {
    mark_tile(bytes, nbytes, tile, sc, lds, Whole{nbytes});
}

// how many marked words of a tile lie before its word i (bm = the tile's kBmWords dwords of the bitmap)
FG_WV uint32_t rank_in_tile(const uint32_t* bm, uint32_t i) {
    uint32_t r = 0;
    for (uint32_t k = 0; k < (i >> 5); ++k) r += wv::popc32(bm[k]);
    return r + wv::popc32(bm[i >> 5] & ((1u << (i & 31u)) - 1u));
}

// ---- 2: nodes.  All 64 lanes; `lds` = kLdsWords dwords. ------------------------------------------------------------------------
template <class Span>
FG_WV void nodes_tile(const uint8_t* bytes, uint64_t nbytes, uint32_t tile, const Scratch& sc, uint32_t* lds, const Span& span) {
    const Lds m = lds_of(lds);
    const uint32_t l = wv::lane();
    if (l < kBmWords) m.sb[l] = sc.bitmap[(uint64_t)tile * kBmWords + l];
    wv::sync();
    if (l == 0) {
        uint32_t total = 0;
        for (uint32_t k = 0; k < kBmWords; ++k) { m.pre[k] = total; total += wv::popc32(m.sb[k]); }
        uint32_t first = 0, ok = 1u;
        if (total) {
            first = g_add32(&sc.hdr[H_NODES], total);
            if ((uint64_t)first + total > sc.node_cap) {  // the node store is used up: the launch declines
                g_or32(&sc.hdr[H_DECLINE], 1u);
                ok = 0u; first = 0u; total = 0u;
            }
        }
        sc.tile_first[tile] = first;
        sc.tile_cnt[tile] = total;
        m.st[0] = first; m.st[1] = total; m.st[2] = ok;
    }
    wv::sync();
    const uint32_t first = m.st[0], total = m.st[1];
    if (total == 0u) return;  // (wave-uniform)
    resolve_tile(bytes, nbytes, tile, m, span);
    for (uint32_t r = 0; r < kDoubling; ++r) {
        uint32_t n2[kTileWords / wv::kLanes], c2[kTileWords / wv::kLanes];
#pragma unroll
        for (uint32_t j = 0; j < kTileWords / wv::kLanes; ++j) {
            const uint32_t i = j * wv::kLanes + l, a = m.nx[i];
            n2[j] = m.nx[a];
            c2[j] = m.c[i] + m.c[a];
        }
        wv::sync();
#pragma unroll
        for (uint32_t j = 0; j < kTileWords / wv::kLanes; ++j) {
            const uint32_t i = j * wv::kLanes + l;
            m.nx[i] = n2[j];
            m.c[i] = c2[j];
        }
        wv::sync();
    }
    for (uint32_t j = 0; j < kTileWords / wv::kLanes; ++j) {
        const uint32_t i = j * wv::kLanes + l;
        if (!((m.sb[i >> 5] >> (i & 31u)) & 1u)) continue;
        const uint32_t u = first + m.pre[i >> 5] + wv::popc32(m.sb[i >> 5] & ((1u << (i & 31u)) - 1u));
        const uint32_t f = m.fin[m.nx[i]];
        const uint32_t kind = f >> kKindShift;
        const uint32_t cnt = m.c[i] + (kind == (uint32_t)K_EXIT || (Span::kSegmented && kind == (uint32_t)K_END) ? 1u : 0u);
        sc.nd_pos[u] = tile * kTileWords + i;
        sc.nd_fin[u] = f;
        sc.nd_cnt[u] = cnt;
        sc.jf0[u] = cnt;
    }
}
FG_WV void nodes_tile(const uint8_t* bytes, uint64_t nbytes, uint32_t tile, const Scratch& sc, uint32_t* lds) {
    nodes_tile(bytes, nbytes, tile, sc, lds, Whole{nbytes});
}

// ---- 3: one thread per node slot ---------------------------------------------------------------------------------------------------
template <class Span>
FG_WV void link_node(uint32_t u, const Scratch& sc, const Span& span) {
    if (sc.hdr[H_DECLINE] != 0u || u >= sc.hdr[H_NODES]) return;
    const uint32_t f = sc.nd_fin[u];
    uint32_t next = kNil;
    if ((f >> kKindShift) == (uint32_t)K_EXIT) {
        const uint32_t x = f & kPosMask, t2 = x / kTileWords;
        const uint32_t k = rank_in_tile(sc.bitmap + (uint64_t)t2 * kBmWords, x % kTileWords);
        if (k < sc.tile_cnt[t2]) next = sc.tile_first[t2] + k;
        else g_or32(&sc.hdr[H_DECLINE], 2u);  // (never: the mark stage set the bit of every exit)
    }
    sc.jn0[u] = next;
    if (span.root(sc.nd_pos[u])) { sc.mk_stamp[u] = 1u; sc.mk_f[u] = 0u; }  // the start of a stream of its own
}
FG_WV void link_node(uint32_t u, const Scratch& sc) { link_node(u, sc, Whole{0}); }

// ---- 4: round r = 1 .. rounds of the ranking, one thread per node slot -------------------------------------------------------------
FG_WV void jump_round(uint32_t u, uint32_t r, const Scratch& sc) {
    if (sc.hdr[H_DECLINE] != 0u || u >= sc.hdr[H_NODES]) return;
    const uint32_t* jna = (r & 1u) ? sc.jn0 : sc.jn1;
    const uint32_t* jfa = (r & 1u) ? sc.jf0 : sc.jf1;
    uint32_t* jnb = (r & 1u) ? sc.jn1 : sc.jn0;
    uint32_t* jfb = (r & 1u) ? sc.jf1 : sc.jf0;
    const uint32_t nx = jna[u], f = jfa[u];
    const uint32_t stamp = sc.mk_stamp[u];
    if (nx == kNil) {
        jnb[u] = kNil; jfb[u] = f;
        return;
    }
    if (stamp != 0u && stamp <= r) {  // on the chain since an earlier round: so is its 2^(r-1)-th successor (marked here and only here)
        sc.mk_f[nx] = sc.mk_f[u] + f;
        sc.mk_stamp[nx] = r + 1u;
    }
    jnb[u] = jna[nx];
    jfb[u] = f + jfa[nx];
}

// ---- 5: emit.  All 64 lanes; `lds` = kLdsWords dwords. -----------------------------------------------------------------------------
FG_WV void emit_tile(const uint8_t* bytes, uint64_t nbytes, uint32_t tile, const Scratch& sc, uint64_t* offsets, uint64_t cap, uint32_t* lds) {
    const Lds m = lds_of(lds);
    const uint32_t l = wv::lane();
    if (sc.hdr[H_DECLINE] != 0u) return;  // (nothing is valid: write nothing)
    const uint32_t first = sc.tile_first[tile], cnt = sc.tile_cnt[tile];
    uint32_t u = kNil;
    for (uint32_t k0 = 0; k0 < cnt && u == kNil; k0 += wv::kLanes) {  // (at most kTileWords / 64 steps; the chain enters a tile once)
        const uint32_t k = k0 + l;
        const uint64_t mine = wv::ballot(k < cnt && sc.mk_stamp[first + (k < cnt ? k : 0u)] != 0u);
        if (mine != 0ull) u = first + k0 + wv::ctz64(mine);
    }
    if (u == kNil) return;  // the chain does not enter this tile
    resolve_tile(bytes, nbytes, tile, m);
    uint32_t* list = m.c;  // (the hop counts are not needed here: the words of the tile where the chain's messages start)
    if (l == 0) {
        uint32_t p = sc.nd_pos[u] - tile * kTileWords, k = 0;
        for (uint32_t hop = 0; hop < kTileWords; ++hop) {
            const uint32_t kind = m.fin[p] >> kKindShift;
            if (kind < (uint32_t)K_EXIT) break;
            list[k++] = p;
            if (kind == (uint32_t)K_EXIT) break;
            p = m.nx[p];
        }
        m.st[0] = k;
    }
    wv::sync();
    const uint32_t k = m.st[0], frame = sc.mk_f[u];
    for (uint32_t j = l; j < k; j += wv::kLanes)
        if ((uint64_t)frame + j < cap) offsets[frame + j] = ((uint64_t)tile * kTileWords + list[j]) * 8ull;
    // the node that ends the chain reports for the stream
    const uint32_t f = sc.nd_fin[u];
    if (l == 0 && (f >> kKindShift) < (uint32_t)K_EXIT) {
        const uint32_t total = frame + sc.nd_cnt[u];
        sc.hdr[H_STOP] = f >> kKindShift;
        sc.hdr[H_NFRAMES] = total;
        sc.hdr[H_CONSUMED] = f & kPosMask;
        sc.hdr[H_DONE] = 1u;
        if (total <= cap) offsets[total] = (uint64_t)(f & kPosMask) * 8ull;
    }
}

}  // namespace capnpf
}  // namespace fg
