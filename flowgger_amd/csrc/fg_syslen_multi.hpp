// fg_syslen_multi.hpp -- framing the octet-counted chunks of MANY connections in one launch: the buffer holds K segments back to back
// (clamped starts c[0 .. K], as fg_frame_multi.hpp), and every segment is walked as if it were the whole chunk (host_walk of
// fg_syslen_parse.hpp over bytes[c[k] .. c[k + 1])).  HIP-free: compiled by hipcc into fg_syslen_multi.hip (launch code and nothing else
// lives there) and by g++ over the fiber emulation of a wave (tests/native/syslen_multi_host.cpp).
//
// Reference: every connection has a SyslenSplitter of its own (input/tcp/tcp_input.rs:39-47, splitter/syslen_splitter.rs:10-57).
//
// Many connections are many roots of the forest that fg_syslen.hpp ranks; its stages are instantiated here with one change each:
//   1 resolve  a candidate at p may reach to the end of the SEGMENT that holds p (Segs::limit), not to nbytes: a prefix that meets that
//              end without a ' ' is TAIL, so is a payload that would cross it, whatever bytes the buffer holds there.  A tile finds
//              the boundaries inside it by a binary search over c (none is the common case: one limit for the tile).  A candidate
//              whose frame ends exactly on its segment's end ends a chain and is no exit.  Only the segment that spans a tile's end
//              can leave the tile, so the exit and inbox bounds see less speculation than one stream gives them, not more.
//   2 walk     the roots do NOT go through the inboxes (forty connections of 100 bytes put forty roots into one tile, kInbox is 16):
//              node tiles * kInbox + k is segment k's start, walked like an inbox entry and marked with zero sums.  An empty
//              segment's root is a chain of its own that ends CLEAN at once.
//   3 rank     unchanged: the chains are disjoint, pointer jumping marks every node of every true chain once, with the frames and
//              payload bytes before it IN ITS SEGMENT.
//   + collect  one lane per node: the node that ends a true chain writes its segment's frames, payload bytes, consumed and stop;
//     scan     one wave: the exclusive sums over the segments -- seg_first and each segment's base in d_packed -- the totals, and, when
//              the frames fit the capacity, the per-segment outputs.
//   4 emit     a tile emits from its at most one marked inbox entry, then from every root that starts inside it, in order, each from
//              its segment's bases.
// Declines as fg_syslen.hpp does, and when a segment was left without an end (never, unless an inbox ran over).  No spin, no wait on
// another wave anywhere.
#pragma once
#include "fg_frame_multi.hpp"
#include "fg_syslen.hpp"

namespace fg {
namespace syslen {

constexpr uint64_t kMaxSegs = 1ull << 24;  // node numbers are 32-bit words

using Segs = fmulti::Segs<kTile>;  // the clamped starts as the stages ask for them

// ---- device scratch: fg_syslen.hpp's, with n_segs root nodes behind the inbox nodes, and four words per segment ---------------------
struct MScratch : Scratch {
    uint64_t* c;        // [n_segs + 1] the clamped starts
    uint32_t* sg_f;     // [n_segs] frames of the segment; after the scan: frames before it
    uint32_t* sg_b;     // [n_segs] payload bytes likewise
    uint32_t* sg_cons;  // [n_segs] bytes its frames cover
    uint32_t* sg_stop;  // [n_segs] ST_*, kNil until its chain's last node reports
    uint32_t n_segs, root0, nodes;
    FG_WV Segs segs() const { return Segs{c, n_segs}; }
};
FG_WVH uint64_t m_nodes(uint64_t nbytes, uint64_t n_segs) { return (uint64_t)tiles_of(nbytes) * kInbox + n_segs; }
// hdr, inbox_cnt, mk_stamp are cleared; sg_stop is filled with kNil
FG_WVH uint64_t m_zero_words(uint64_t nbytes, uint64_t n_segs) { return H_WORDS + tiles_of(nbytes) + m_nodes(nbytes, n_segs); }
FG_WVH uint64_t m_scratch_words(uint64_t nbytes, uint64_t n_segs) {
    return m_zero_words(nbytes, n_segs) + 4u * n_segs + 10u * m_nodes(nbytes, n_segs) + (uint64_t)tiles_of(nbytes) * kInbox + 2u * (n_segs + 1u) + 2u;
}
FG_WVH MScratch m_carve(uint32_t* base, uint64_t nbytes, uint64_t n_segs) {
    MScratch s;
    s.tiles = tiles_of(nbytes);
    s.rounds = 0;
    while ((1ull << s.rounds) < s.tiles) ++s.rounds;  // (a chain has one node per tile at most, its root included)
    s.n_segs = (uint32_t)n_segs;
    s.root0 = s.tiles * kInbox;
    s.nodes = s.root0 + s.n_segs;
    const uint64_t n = s.nodes;
    uint32_t* p = base;
    s.hdr = p; p += H_WORDS;
    s.inbox_cnt = p; p += s.tiles;
    s.mk_stamp = p; p += n;
    s.sg_stop = p; p += n_segs;
    s.sg_f = p; p += n_segs;
    s.sg_b = p; p += n_segs;
    s.sg_cons = p; p += n_segs;
    s.mk_f = p; p += n;
    s.mk_b = p; p += n;
    s.inbox_pos = p; p += s.root0;
    s.nd_exit = p; p += n;
    s.nd_term = p; p += n;
    for (int k = 0; k < 2; ++k) { s.jn[k] = p; p += n; s.jf[k] = p; p += n; s.jb[k] = p; p += n; }
    if ((p - base) & 1) ++p;  // (base is 8-byte aligned)
    s.c = reinterpret_cast<uint64_t*>(p);
    return s;
}

// ---- 1: resolve_route(bytes, nbytes, tile, sc, lds, sc.segs()) ---------------------------------------------------------------------

// ---- 2: one lane per node u < sc.nodes --------------------------------------------------------------------------------------------
FG_WV void m_walk(const uint8_t* bytes, uint32_t u, const MScratch& sc) {
    if (u < sc.root0) {
        const uint32_t tile = u / kInbox;
        uint32_t n = sc.inbox_cnt[tile];
        if (n > kInbox) n = kInbox;
        if (u % kInbox >= n) return;
        const uint32_t x = sc.inbox_pos[u];
        walk_chain(bytes, sc.segs().limit(x), tile, u, x, inbox_find(sc, tile, x) == u, false, sc);
    } else {
        const uint64_t s = sc.c[u - sc.root0], e = sc.c[u - sc.root0 + 1u];
        walk_chain(bytes, e, (uint32_t)(s / kTile), u, (uint32_t)s, true, true, sc);  // (s == e: CLEAN at once)
    }
}

// ---- 3: round r, one lane per node ------------------------------------------------------------------------------------------------
FG_WV void m_jump(uint32_t u, uint32_t r, const MScratch& sc) {
    if (u < sc.root0) jump_round(u / kInbox, u % kInbox, r, sc);
    else jump_node(u, r, sc);
}

// ---- collect: one lane per node; the last node of a true chain speaks for its segment ------------------------------------------------
FG_WV void m_collect(uint32_t u, const MScratch& sc) {
    uint64_t k = u - sc.root0;
    if (u < sc.root0) {
        uint32_t n = sc.inbox_cnt[u / kInbox];
        if (n > kInbox) n = kInbox;
        if (u % kInbox >= n) return;
    }
    if (sc.mk_stamp[u] == 0u || sc.nd_term[u] == kNil) return;
    if (u < sc.root0) k = sc.segs().behind(sc.inbox_pos[u]) - 1u;
    sc.sg_f[k] = sc.mk_f[u] + sc.jf[0][u];
    sc.sg_b[k] = sc.mk_b[u] + sc.jb[0][u];
    sc.sg_cons[k] = sc.nd_exit[u] - (uint32_t)sc.c[k];
    sc.sg_stop[k] = sc.nd_term[u];
}

// ---- scan: ONE wave, all 64 lanes ----------------------------------------------------------------------------------------------------
FG_WV void m_scan(const MScratch& sc, uint64_t cap, uint64_t* offsets, uint64_t* seg_first, uint64_t* seg_consumed, uint8_t* seg_stop) {
    const uint32_t l = wv::lane();
    uint32_t base_f = 0, base_b = 0;
    bool missing = false;
    for (uint32_t k0 = 0; k0 < sc.n_segs; k0 += wv::kLanes) {
        const uint32_t k = k0 + l;
        const bool in = k < sc.n_segs && sc.sg_stop[k] != kNil;
        missing |= k < sc.n_segs && !in;
        const uint32_t f = in ? sc.sg_f[k] : 0u, b = in ? sc.sg_b[k] : 0u;
        uint32_t tf = 0, tb = 0;
        const uint32_t ef = wv::excl_sum(f, &tf), eb = wv::excl_sum(b, &tb);
        if (k < sc.n_segs) {
            sc.sg_f[k] = base_f + ef;
            sc.sg_b[k] = base_b + eb;
        }
        base_f += tf;
        base_b += tb;
    }
    const bool declined = wv::any(missing) || sc.hdr[H_DECLINE] != 0u;
    wv::sync();  // (everybody has read the decline word)
    if (l == 0) {
        if (declined) sc.hdr[H_DECLINE] |= 4u;
        sc.hdr[H_NFRAMES] = base_f;
        sc.hdr[H_TOTAL] = base_b;
        sc.hdr[H_DONE] = 1u;
    }
    if (declined || base_f > cap) return;  // (nothing is valid / the caller learns the need: no per-segment output)
    for (uint32_t k = l; k < sc.n_segs; k += wv::kLanes) {
        seg_first[k] = sc.sg_f[k];
        seg_consumed[k] = sc.sg_cons[k];
        seg_stop[k] = (uint8_t)sc.sg_stop[k];
    }
    if (l == 0) {
        seg_first[sc.n_segs] = base_f;
        offsets[base_f] = base_b;
    }
}

// ---- 4: emit + pack.  All 64 lanes; `lds` = kEmitLdsWords dwords. -----------------------------------------------------------------
FG_WV void m_emit(const uint8_t* bytes, uint32_t tile, const MScratch& sc, uint8_t* packed, uint64_t* offsets, uint64_t* starts, uint8_t* bad,
                  uint64_t cap, uint32_t* lds) {
    if (sc.hdr[H_DECLINE] != 0u || sc.hdr[H_NFRAMES] > cap) return;  // (nothing is valid / nothing fits: write nothing)
    const Segs sg = sc.segs();
    const uint64_t base = (uint64_t)tile * kTile, end = base + kTile;
    const uint32_t u = marked_entry(tile, sc);
    if (u != kNil) {  // the segment that spans the tile's start enters here
        const uint64_t j = sg.behind(sc.inbox_pos[u]);
        emit_chain(bytes, sg.c[j], end, sc.inbox_pos[u], sc.sg_f[j - 1u] + sc.mk_f[u], sc.sg_b[j - 1u] + sc.mk_b[u], packed, offsets, starts, bad, cap, lds);
    }
    for (uint64_t k = fmulti::lower_bound_u64(sg.c, 0, sg.n_segs, base); k < sg.n_segs && sg.c[k] < end; ++k)
        if (sg.c[k + 1u] > sg.c[k]) emit_chain(bytes, sg.c[k + 1u], end, sg.c[k], sc.sg_f[k], sc.sg_b[k], packed, offsets, starts, bad, cap, lds);
}

// ---- the per-segment CUT (fg_transcode_multi_batch) ---------------------------------------------------------------------------------
// SyslenSplitter::run unwraps String::from_utf8 (syslen_splitter.rs:33): the first payload of a connection that is not valid UTF-8 ends
// its thread, and no frame behind it is ever decoded.  bad[n] holds 0 / 1 per frame, seg_first[n_segs + 1] the first frame of every
// segment (non-decreasing, seg_first[n_segs] = n); with c_k the first flagged frame of segment k, every frame of k behind c_k becomes
// kCutMark.  Two passes, one lane per frame each, over cut[n_segs + 1] words that start as kCutNone: cut[k] = c_k, cut[n_segs] = the
// first flagged frame of the whole batch.  A batch without a flagged payload -- the everyday case -- costs the first pass its read of
// `bad` and the second one word per wave: no search runs.
constexpr uint32_t kCutNone = 0xFFFFFFFFu;  // (also what bounds n: frame numbers are 32-bit words here)
constexpr uint8_t kCutMark = 3u;            // FG_SLOT_UNREACHED (include/fg_hip.h; fg_syslen_multi.hip asserts it)
FG_WVH uint64_t cut_words(uint64_t n_segs) { return n_segs + 1u; }
#if defined(__HIPCC__)
FG_WV void g_min32(uint32_t* p, uint32_t v) { atomicMin(p, v); }
#else
FG_WV void g_min32(uint32_t* p, uint32_t v) { if (v < *p) *p = v; }
#endif
// the segment that holds frame i < n: the last k with seg_first[k] <= i (empty segments are runs of equal values: the upper bound
// steps over them)
FG_WV uint64_t cut_segment(const uint64_t* seg_first, uint64_t n_segs, uint64_t i) {
    return fmulti::upper_bound_u64(seg_first, 0, n_segs + 1u, i) - 1u;
}
// pass 1, frame i < n: the rare flagged lane finds its segment and reports its number
FG_WV void cut_find(const uint8_t* bad, uint64_t i, const uint64_t* seg_first, uint64_t n_segs, uint32_t* cut) {
    if (bad[i] == 0u) return;
    g_min32(cut + cut_segment(seg_first, n_segs, i), (uint32_t)i);
    g_min32(cut + n_segs, (uint32_t)i);
}
// pass 2 (a launch of its own: pass 1 has ended), frame i < n
FG_WV void cut_mark(uint8_t* bad, uint64_t i, const uint64_t* seg_first, uint64_t n_segs, const uint32_t* cut) {
    if (i <= cut[n_segs]) return;  // (nothing flagged: every lane of every wave leaves here; else the frames in front of the first one)
    if (i > cut[cut_segment(seg_first, n_segs, i)]) bad[i] = kCutMark;
}

}  // namespace syslen
}  // namespace fg
