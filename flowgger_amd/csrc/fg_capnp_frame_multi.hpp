// fg_capnp_frame_multi.hpp -- framing the Cap'n Proto chunks of MANY connections in one launch: the buffer holds K segments back to back
// and every segment is walked as if it were the whole chunk (host_walk of fg_capnp_next.hpp over bytes[c[k] .. c[k + 1])).  HIP-free:
// compiled by hipcc into fg_capnp_frame_multi.hip (launch code and nothing else lives there) and by g++ over the fiber emulation of a
// wave (tests/native/capnp_frame_multi_host.cpp).
//
// Reference: every connection has a CapnpSplitter of its own (input/tcp/tcp_input.rs:39-47, splitter/capnp_splitter.rs:24-46).
//
// ALIGNMENT.  The framer works on 8-byte words counted from the buffer's start, so every segment starts on a word: the starts are clamped
// as fmulti::clamp_start does and then rounded DOWN to a multiple of 8 (c[n_segs] = nbytes stays as it is: only the last segment may end
// off a word).  A message is whole words, so the last len % 8 bytes of a connection's pending bytes never complete one: the caller
// keeps them back.  Memory safety never depends on the list.
//
// Many connections are many roots of the forest that fg_capnp_frame.hpp ranks; its stages are instantiated here with one change each:
//   1 resolve  a message at word w may reach to the end of the SEGMENT that holds w (Segs::limit), not to nbytes: a table or a body
//              that would cross that end is TAIL, whatever bytes the buffer holds there.  A tile finds the boundaries inside it by one
//              binary search over c (none is the common case: one limit for the tile).  A message that ends exactly on its segment's end
//              is K_END: it counts, and its chain ends CLEAN there -- no exit, no hop, because the word it ends on is another
//              connection's root or the buffer's end.  So no chain, true or speculative, ever crosses a boundary.
//   2 mark     seg_root (one lane per segment) writes the rounded starts and sets the bitmap bit of every NON-EMPTY segment's first
//     nodes    word: the roots are nodes like the landing words, through the same bitmap.  The node store grows by n_segs.
//   3 link     a node whose word is a non-empty segment's start is a root: stamp 1, zero messages before it.
//   4 rank     unchanged: the chains are disjoint and each enters a tile at most once.
//   + collect  one lane per node: the stamped node whose chain stops (anything but K_EXIT) writes its segment's messages, consumed, stop.
//     scan     ONE wave: slots per segment = its messages + one CARRY slot when consumed < length; the exclusive sums are seg_first;
//              when the total fits the capacity, the per-segment outputs, the CARRY slots and offsets[n_slots] = nbytes.  An empty
//              segment is CLEAN with nothing and has no node.
//   5 emit     a tile emits from EVERY stamped node in it (the chain that enters and every root inside): the lanes share the nodes out,
//              each follows its chain through the tile in LDS and leaves slot + 1 at every message's word; then all lanes sweep the
//              tile's words and write the offsets.  True chains are disjoint, so all walks of a tile together make at most kTileWords
//              hops, however many segments the tile holds.
// Declines as fg_capnp_frame.hpp does (the node store), and when a non-empty segment was left without an end (never).  No spin and no
// wait on another wave anywhere; every loop is bounded by the tile's words, 511 sizes, the segment count or the round count.
#pragma once
#include "fg_capnp_frame.hpp"
#include "fg_frame_multi.hpp"

namespace fg {
namespace capnpf {

constexpr uint64_t kMaxSegs = 1ull << 24;  // (the node store and the per-segment words are 32-bit counts)

// the rounded starts as the stages ask for them
struct Segs : fmulti::Segs<kTileBytes> {  // (c[k < n_segs] a multiple of 8)
    // word w is the first word of a non-empty segment
    FG_WV bool root(uint32_t w) const {
        const uint64_t p = (uint64_t)w * 8ull;
        return p < c[n_segs] && c[behind(p) - 1u] == p;  // (c[0] = 0 <= p: behind(p) >= 1)
    }
};

// ---- device scratch: fg_capnp_frame.hpp's with n_segs more nodes, three words per segment and the starts ------------------------------
struct MScratch : Scratch {
    uint64_t* c;        // [n_segs + 1] the clamped starts, rounded down to a word
    uint64_t* raw;      // [n_segs + 1] the clamped starts
    uint32_t* sg_f;     // [n_segs] messages of the segment; after the scan: slots before it
    uint32_t* sg_cons;  // [n_segs] bytes its messages cover
    uint32_t* sg_stop;  // [n_segs] ST_*, kNil until its chain's last node reports
    uint32_t n_segs;
    FG_WV Segs segs() const { return Segs{{c, n_segs}}; }
};
FG_WVH uint32_t m_node_cap(uint64_t nbytes, uint64_t n_segs) { return node_cap_of(nbytes) + (uint32_t)n_segs; }
// hdr, bitmap, mk_stamp are cleared; sg_stop is filled with kNil
FG_WVH uint64_t m_zero_words(uint64_t nbytes, uint64_t n_segs) { return H_WORDS + (uint64_t)tiles_of(nbytes) * kBmWords + m_node_cap(nbytes, n_segs); }
FG_WVH uint64_t m_scratch_words(uint64_t nbytes, uint64_t n_segs) {
    return m_zero_words(nbytes, n_segs) + 3u * n_segs + 2ull * tiles_of(nbytes) + 8ull * m_node_cap(nbytes, n_segs) + 4u * (n_segs + 1u) + 2u;
}
FG_WVH MScratch m_carve(uint32_t* base, uint64_t nbytes, uint64_t n_segs) {
    MScratch s;
    s.tiles = tiles_of(nbytes);
    s.node_cap = m_node_cap(nbytes, n_segs);
    s.rounds = 0;
    while ((1ull << s.rounds) < s.tiles) ++s.rounds;  // (a chain has one node per tile at most, its root included)
    s.n_segs = (uint32_t)n_segs;
    const uint64_t n = s.node_cap;
    uint32_t* p = base;
    s.hdr = p; p += H_WORDS;
    s.bitmap = p; p += (uint64_t)s.tiles * kBmWords;
    s.mk_stamp = p; p += n;
    s.sg_stop = p; p += n_segs;
    s.sg_f = p; p += n_segs;
    s.sg_cons = p; p += n_segs;
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
    if ((p - base) & 1) ++p;  // (base is 8-byte aligned)
    s.c = reinterpret_cast<uint64_t*>(p);
    s.raw = s.c + n_segs + 1u;
    return s;
}

// ---- the starts and the roots: one lane per k <= n_segs (sc.raw holds the clamped starts) -------------------------------------------
FG_WV void seg_root(uint64_t k, const MScratch& sc) {
    const uint64_t s = k < sc.n_segs ? sc.raw[k] & ~7ull : sc.raw[k];
    sc.c[k] = s;
    if (k >= sc.n_segs) return;
    const uint64_t e = k + 1u < sc.n_segs ? sc.raw[k + 1u] & ~7ull : sc.raw[k + 1u];
    if (e > s) g_or32(&sc.bitmap[s >> 8], 1u << ((uint32_t)(s >> 3) & 31u));  // (word s / 8 < tiles * kTileWords)
}

// ---- 1 .. 4: mark_tile / nodes_tile / link_node with sc.segs(), jump_round as it is ------------------------------------------------------

// ---- collect: one lane per node slot; the last node of a true chain speaks for its segment ------------------------------------------
FG_WV void m_collect(uint32_t u, const MScratch& sc) {
    if (sc.hdr[H_DECLINE] != 0u || u >= sc.hdr[H_NODES] || sc.mk_stamp[u] == 0u) return;
    const uint32_t f = sc.nd_fin[u], kind = f >> kKindShift;
    if (kind == (uint32_t)K_EXIT) return;
    const uint64_t k = sc.segs().behind((uint64_t)sc.nd_pos[u] * 8ull) - 1u;
    sc.sg_f[k] = sc.mk_f[u] + sc.nd_cnt[u];
    sc.sg_cons[k] = (uint32_t)((uint64_t)(f & kPosMask) * 8ull - sc.c[k]);
    sc.sg_stop[k] = kind == (uint32_t)K_END ? (uint32_t)ST_CLEAN : kind;
}

// ---- scan: ONE wave, all 64 lanes.  H_NFRAMES = the slots of the buffer. ---------------------------------------------------------------
FG_WV void m_scan(const MScratch& sc, uint64_t cap, uint64_t* offsets, uint8_t* kind, uint64_t* seg_first, uint64_t* seg_consumed, uint8_t* seg_stop) {
    const uint32_t l = wv::lane();
    uint32_t base = 0;
    bool missing = false;
    for (uint32_t k0 = 0; k0 < sc.n_segs; k0 += wv::kLanes) {
        const uint32_t k = k0 + l;
        const bool in = k < sc.n_segs;
        const uint64_t len = in ? sc.c[k + 1u] - sc.c[k] : 0ull;
        uint32_t slots = 0;
        if (in && len == 0ull) {  // an empty segment: CLEAN with nothing
            sc.sg_cons[k] = 0u;
            sc.sg_stop[k] = (uint32_t)ST_CLEAN;
        } else if (in) {
            if (sc.sg_stop[k] == kNil) missing = true;
            else slots = sc.sg_f[k] + (sc.sg_cons[k] < len ? 1u : 0u);
        }
        uint32_t t = 0;
        const uint32_t e = wv::excl_sum(slots, &t);
        if (in) sc.sg_f[k] = base + e;
        base += t;
    }
    const bool declined = wv::any(missing) || sc.hdr[H_DECLINE] != 0u;
    wv::sync();  // (everybody has read the decline word; every sg_f is the segment's first slot)
    if (l == 0) {
        if (declined) sc.hdr[H_DECLINE] |= 4u;
        sc.hdr[H_NFRAMES] = base;
        sc.hdr[H_DONE] = 1u;
    }
    if (declined || base > cap) return;  // (nothing is valid / the caller learns the need: no output)
    for (uint32_t k = l; k < sc.n_segs; k += wv::kLanes) {
        const uint64_t len = sc.c[k + 1u] - sc.c[k];
        seg_first[k] = sc.sg_f[k];
        seg_consumed[k] = sc.sg_cons[k];
        seg_stop[k] = (uint8_t)sc.sg_stop[k];
        if (sc.sg_cons[k] < len) {  // the CARRY tail: the segment's last slot
            const uint32_t slot = (k + 1u < sc.n_segs ? sc.sg_f[k + 1u] : base) - 1u;
            offsets[slot] = sc.c[k] + sc.sg_cons[k];
            kind[slot] = fmulti::kSlotCarry;
        }
    }
    if (l == 0) {
        seg_first[sc.n_segs] = base;
        offsets[base] = sc.c[sc.n_segs];
    }
}

// ---- 5: emit.  All 64 lanes; `lds` = kLdsWords dwords. -----------------------------------------------------------------------------
FG_WV void m_emit_tile(const uint8_t* bytes, uint64_t nbytes, uint32_t tile, const MScratch& sc, uint64_t* offsets, uint8_t* kind, uint64_t cap,
                       uint32_t* lds) {
    const Lds m = lds_of(lds);
    const uint32_t l = wv::lane();
    if (sc.hdr[H_DECLINE] != 0u || sc.hdr[H_NFRAMES] > cap) return;  // (nothing is valid / nothing fits: write nothing)
    const uint32_t first = sc.tile_first[tile], cnt = sc.tile_cnt[tile];
    bool mine = false;
    for (uint32_t k = l; k < cnt; k += wv::kLanes) mine |= sc.mk_stamp[first + k] != 0u;  // (at most kTileWords / 64 steps)
    if (!wv::any(mine)) return;  // no true chain enters or starts in this tile
    const Segs sg = sc.segs();
    resolve_tile(bytes, nbytes, tile, m, sg);
    uint32_t* slot_of = m.c;  // (the hop counts are not needed here: slot + 1 of the message that starts at the word, 0 = none)
    for (uint32_t j = 0; j < kTileWords / wv::kLanes; ++j) slot_of[j * wv::kLanes + l] = 0u;
    wv::sync();
    for (uint32_t k = l; k < cnt; k += wv::kLanes) {
        const uint32_t u = first + k;
        if (sc.mk_stamp[u] == 0u) continue;
        const uint32_t pos = sc.nd_pos[u];
        uint32_t p = pos - tile * kTileWords;
        uint32_t slot = sc.sg_f[sg.behind((uint64_t)pos * 8ull) - 1u] + sc.mk_f[u];
        for (uint32_t hop = 0; hop < kTileWords; ++hop) {  // (true chains are disjoint: all lanes together make at most kTileWords hops)
            const uint32_t kd = m.fin[p] >> kKindShift;
            if (kd < (uint32_t)K_EXIT) break;
            slot_of[p] = ++slot;
            if (kd != (uint32_t)K_HOP) break;
            p = m.nx[p];
        }
    }
    wv::sync();
    for (uint32_t j = 0; j < kTileWords / wv::kLanes; ++j) {
        const uint32_t i = j * wv::kLanes + l, s = slot_of[i];
        if (s == 0u || (uint64_t)s > cap) continue;
        offsets[s - 1u] = ((uint64_t)tile * kTileWords + i) * 8ull;
        kind[s - 1u] = fmulti::kSlotFrame;
    }
}

}  // namespace capnpf
}  // namespace fg
