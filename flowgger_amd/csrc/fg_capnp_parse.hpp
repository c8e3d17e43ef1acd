// fg_capnp_parse.hpp -- CapnpSplitter's handle_message for ONE Cap'n Proto message (input.format = "capnp"), host + device.
// reference: src/flowgger/splitter/capnp_splitter.rs:65-167 (get_pairs, get_sd, handle_message) over the readers that
// record.capnp generates (Record: 2 data words, 9 pointers; Pair: 2 data words, 2 pointers) and capnp 0.14's
// private/layout.rs (read_struct_pointer, read_list_pointer, read_text_pointer, follow_fars, bounds_check).
//
// A message is an array of 8-byte words: the segment table (segments - 1, their sizes in words, padded to a word), then the
// segments back to back.  Every access below is ONE aligned word through the reader R (`uint64_t word(uint32_t w)`, w counted
// from the message's first byte, w < Msg::words): a reader never sees an index outside the message.  Nothing is copied or
// unescaped: the spans of the row and of the entries point into the message.
//
// The rules a getter follows (DESIGN section 6 lists them as UNPINNED: the capnp crate cannot be built here, the reference
// pins one vector):
//   * a NULL pointer word reads as the default ("" / an empty list) and is Ok;
//   * a near pointer's target (its own word + 1 + the signed 30-bit offset) must lie inside ITS segment, end inclusive; the
//     object must then fit the segment.  A segment is what the table says, cut at the end of the message;
//   * a far pointer names a segment and a landing pad in it (one word; two words for a double-far): the pad must lie inside
//     that segment; a single pad is read as a near pointer at its own place (a pad that is itself far fails the kind check of
//     the getter), a double pad's first word gives segment + position of the object, its second word is the tag the object
//     is read by;
//   * struct pointer: kind 0; sizes smaller or larger than the schema's are honoured (a missing data field reads as 0, a
//     missing pointer as NULL);
//   * Text: a list pointer (kind 1) of element size BYTE, at least one element, the last byte NUL, the bytes before it
//     well-formed UTF-8 (Unicode 15 table 3-7); padding behind the NUL is not looked at;
//   * List(Pair): a list pointer of any element size but BIT.  INLINE_COMPOSITE: the tag must be a struct tag, elements x
//     words per element must not exceed the pointer's word count, the stride is the TAG's.  Other sizes are read as structs
//     of that one field (capnp upgrades them): VOID nothing, BYTE .. EIGHT_BYTES that many data bits, POINTER one pointer;
//   * of the traversal limit only this: a list of ZERO-sized elements counts one word per element against the reader's
//     8 Mi words, so such a list with more elements than that fails.  The nesting limit cannot be reached (depth 3).
#pragma once
#include <stdint.h>

#include "../../include/fg_hip.h"

#if defined(__HIPCC__)
#define FGC_HD __host__ __device__ __forceinline__
#else
#define FGC_HD inline
#endif

namespace fg {
namespace capnp {

enum : uint32_t {
    ST_OK = 0,
    ST_NO_TS = 1,    // "Missing timestamp"  capnp_splitter.rs:135
    ST_NO_HOST = 2,  // "Missing host name"  :140
    ST_NO_ROOT = 3   // get_root() fails: the reference unwrap()s (:47) and the connection thread is gone
};
constexpr uint32_t kMaxSegments = 512;            // capnp 0.14 serialize::read_segment_table: "Too many segments"
constexpr uint64_t kTraversalWords = 8u << 20;    // ReaderOptions::new().traversal_limit_in_words
constexpr uint32_t kFacilityMax = 0xFFu >> 3, kSeverityMax = 7u;  // record.rs:85,89

struct Seg {
    uint32_t start, len;  // words, from the message's first byte; already cut at the message's end
};
struct Msg {
    uint32_t words = 0;  // whole words of the message
    uint32_t nseg = 0;
    Seg seg0{0, 0};
};
// where a pointer leads: the object's first word, the pointer word that describes it, the segment it must fit
struct Target {
    uint32_t at;
    uint32_t lo, hi;
    Seg seg;
};
// a struct as the generated readers see it
struct StructView {
    uint32_t data_byte = 0;  // first byte of the data section
    uint32_t data_bits = 0;
    uint32_t ptr_at = 0;     // first pointer word
    uint32_t nptr = 0;
    Seg seg{0, 0};
};
struct ListView {
    bool ok = false;         // the getter returned Ok (an empty list for a NULL pointer)
    uint32_t count = 0;
    uint32_t at = 0;         // first element's word
    uint32_t step_bits = 0;  // element stride
    uint32_t data_bits = 0, nptr = 0;  // of one element
    Seg seg{0, 0};
};
struct Row {
    uint32_t status = ST_OK;
    uint32_t fac = 0xFFu, sev = 0xFFu;  // 0xFF = None
    uint64_t ts_bits = 0;
    fg_span sp[6];                      // hostname, appname, procid, msgid, msg, full_msg
    bool sd = false;                    // Record.sd is Some([one element])
    fg_span sd_id{0u, FG_NONE};
    ListView pairs, extra;
    uint32_t n_ent = 0;                 // 1 (the element) + the kept pairs + the kept extras; 0 when sd is None
};

template <class R>
FGC_HD bool open_message(R& rd, uint64_t len_bytes, Msg* m) {
    if (len_bytes < 8u || len_bytes > 0xFFFFFFFFull) return false;  // (spans are 32-bit: a longer message has no row)
    m->words = (uint32_t)(len_bytes >> 3);
    const uint64_t w0 = rd.word(0);
    const uint64_t nseg = (w0 & 0xFFFFFFFFull) + 1u;
    if (nseg >= kMaxSegments) return false;
    m->nseg = (uint32_t)nseg;
    const uint32_t tab = (m->nseg + 2u) >> 1;
    if (tab > m->words) return false;
    const uint64_t s0 = w0 >> 32;
    const uint32_t left = m->words - tab;
    m->seg0 = Seg{tab, s0 < left ? (uint32_t)s0 : left};
    return true;
}
// segment `id` of the table (size k is the 32-bit half (k + 1) & 1 of word (k + 1) >> 1)
template <class R>
FGC_HD bool segment(R& rd, const Msg& m, uint64_t id, Seg* s) {
    if (id >= m.nseg) return false;
    if (id == 0u) {
        *s = m.seg0;
        return true;
    }
    uint64_t start = (m.nseg + 2u) >> 1, size = 0;
    for (uint32_t k = 0; k <= (uint32_t)id; ++k) {
        start += size;
        const uint64_t w = rd.word((k + 1u) >> 1);
        size = ((k + 1u) & 1u) ? (w >> 32) : (w & 0xFFFFFFFFull);
    }
    if (start > m.words) start = m.words;
    const uint64_t left = m.words - start;
    *s = Seg{(uint32_t)start, (uint32_t)(size < left ? size : left)};
    return true;
}
FGC_HD int64_t near_offset(uint32_t lo) { return (int64_t)((int32_t)lo >> 2); }  // signed 30 bits
FGC_HD bool fits(const Target& t, uint64_t words) { return (uint64_t)t.at + words <= (uint64_t)t.seg.start + t.seg.len; }

// layout.rs follow_fars: the non-NULL pointer p at word pw of segment seg
template <class R>
FGC_HD bool follow(R& rd, const Msg& m, const Seg& seg, uint32_t pw, uint64_t p, Target* t) {
    const uint32_t lo = (uint32_t)p, hi = (uint32_t)(p >> 32);
    if ((lo & 3u) != 2u) {
        const int64_t rel = (int64_t)(pw - seg.start) + 1 + near_offset(lo);
        if (rel < 0 || rel > (int64_t)seg.len) return false;
        *t = Target{seg.start + (uint32_t)rel, lo, hi, seg};
        return true;
    }
    Seg ps;
    if (!segment(rd, m, hi, &ps)) return false;
    const uint32_t pos = lo >> 3;
    const bool dbl = (lo & 4u) != 0u;
    if ((uint64_t)pos + (dbl ? 2u : 1u) > ps.len) return false;
    const uint64_t pad = rd.word(ps.start + pos);
    if (!dbl) {
        const int64_t rel = (int64_t)pos + 1 + near_offset((uint32_t)pad);
        if (rel < 0 || rel > (int64_t)ps.len) return false;
        *t = Target{ps.start + (uint32_t)rel, (uint32_t)pad, (uint32_t)(pad >> 32), ps};
        return true;
    }
    Seg os;
    if (!segment(rd, m, pad >> 32, &os)) return false;
    const uint32_t opos = (uint32_t)pad >> 3;
    if (opos > os.len) return false;
    const uint64_t tag = rd.word(ps.start + pos + 1u);
    *t = Target{os.start + opos, (uint32_t)tag, (uint32_t)(tag >> 32), os};
    return true;
}

// One step of the UTF-8 automaton.  st: 0 = between characters, else  need | lo << 8 | hi << 16  (continuation bytes still
// owed, the range the next one must lie in).
FGC_HD bool utf8_step(uint32_t b, uint32_t& st) {
    if (st) {
        if (b < ((st >> 8) & 0xFFu) || b > (st >> 16)) return false;
        const uint32_t need = (st & 0xFFu) - 1u;
        st = need ? need | 0x80u << 8 | 0xBFu << 16 : 0u;
        return true;
    }
    if (b < 0x80u) return true;
    if (b < 0xC2u || b > 0xF4u) return false;
    if (b < 0xE0u) st = 1u | 0x80u << 8 | 0xBFu << 16;
    else if (b < 0xF0u) st = 2u | (b == 0xE0u ? 0xA0u : 0x80u) << 8 | (b == 0xEDu ? 0x9Fu : 0xBFu) << 16;
    else st = 3u | (b == 0xF0u ? 0x90u : 0x80u) << 8 | (b == 0xF4u ? 0x8Fu : 0xBFu) << 16;
    return true;
}
// str::from_utf8 over the n bytes that start at word `at` (a text always starts on a word)
template <class R>
FGC_HD bool utf8_ok(R& rd, uint32_t at, uint32_t n) {
    uint32_t st = 0;
    for (uint32_t i = 0; i < n; i += 8u) {
        uint64_t w = rd.word(at + (i >> 3));
        const uint32_t have = n - i < 8u ? n - i : 8u;
        if (have < 8u) w &= (1ull << (8u * have)) - 1ull;  // (what lies behind the text reads as NUL)
        if (st == 0u && (w & 0x8080808080808080ull) == 0ull) continue;
        for (uint32_t k = 0; k < have; ++k)
            if (!utf8_step((uint32_t)(w >> (8u * k)) & 0xFFu, st)) return false;
    }
    return st == 0u;
}

// layout.rs read_text_pointer for the pointer at word pw: false = the getter's Err; a NULL pointer is Ok("")
template <class R>
FGC_HD bool get_text(R& rd, const Msg& m, const Seg& seg, uint32_t pw, fg_span* out) {
    const uint64_t p = rd.word(pw);
    *out = fg_span{0u, 0u};
    if (p == 0ull) return true;
    Target t;
    if (!follow(rd, m, seg, pw, p, &t)) return false;
    if ((t.lo & 3u) != 1u || (t.hi & 7u) != 2u) return false;
    const uint32_t n = t.hi >> 3;
    if (!fits(t, ((uint64_t)n + 7u) >> 3) || n == 0u) return false;
    const uint32_t last = n - 1u;
    if (((rd.word(t.at + (last >> 3)) >> (8u * (last & 7u))) & 0xFFull) != 0ull) return false;
    if (!utf8_ok(rd, t.at, last)) return false;
    *out = fg_span{t.at << 3, last};
    return true;
}
// pointer field k of a struct (NULL when the struct has fewer pointers)
template <class R>
FGC_HD bool text_field(R& rd, const Msg& m, const StructView& s, uint32_t k, fg_span* out) {
    if (k >= s.nptr) {
        *out = fg_span{0u, 0u};
        return true;
    }
    return get_text(rd, m, s.seg, s.ptr_at + k, out);
}
// layout.rs read_list_pointer(expected = INLINE_COMPOSITE) for pointer field k
template <class R>
FGC_HD ListView list_field(R& rd, const Msg& m, const StructView& s, uint32_t k) {
    ListView l;
    const uint64_t p = k < s.nptr ? rd.word(s.ptr_at + k) : 0ull;
    if (p == 0ull) {
        l.ok = true;
        return l;
    }
    Target t;
    if (!follow(rd, m, s.seg, s.ptr_at + k, p, &t)) return l;
    if ((t.lo & 3u) != 1u) return l;
    const uint32_t es = t.hi & 7u, cnt = t.hi >> 3;
    l.seg = t.seg;
    if (es == 7u) {
        if (!fits(t, (uint64_t)cnt + 1u)) return l;
        const uint64_t tag = rd.word(t.at);
        if ((tag & 3ull) != 0ull) return l;
        const uint32_t n = (uint32_t)tag >> 2, dw = (uint32_t)(tag >> 32) & 0xFFFFu, pc = (uint32_t)(tag >> 48);
        const uint32_t wpe = dw + pc;
        if ((uint64_t)n * wpe > (uint64_t)cnt) return l;
        if (wpe == 0u && n > kTraversalWords) return l;
        l.count = n;
        l.at = t.at + 1u;
        l.step_bits = wpe * 64u;
        l.data_bits = dw * 64u;
        l.nptr = pc;
    } else {
        if (es == 1u) return l;  // a bit list is not upgraded
        const uint32_t bits = es == 0u ? 0u : es == 6u ? 64u : 4u << (es - 1u);  // 2: 8, 3: 16, 4: 32, 5: 64
        if (!fits(t, ((uint64_t)cnt * bits + 63u) >> 6)) return l;
        if (bits == 0u && cnt > kTraversalWords) return l;
        l.count = cnt;
        l.at = t.at;
        l.step_bits = bits;
        l.data_bits = es == 6u ? 0u : bits;
        l.nptr = es == 6u ? 1u : 0u;
    }
    l.ok = true;
    return l;
}
FGC_HD StructView element(const ListView& l, uint32_t e) {
    StructView s;
    const uint64_t bit = (uint64_t)e * l.step_bits;
    s.data_byte = (l.at << 3) + (uint32_t)(bit >> 3);
    s.data_bits = l.data_bits;
    s.ptr_at = l.at + (uint32_t)((bit + l.data_bits) >> 6);
    s.nptr = l.nptr;
    s.seg = l.seg;
    return s;
}
// data fields (a field beyond the struct's data section reads as 0)
template <class R>
FGC_HD uint32_t data_u16_0(R& rd, const StructView& s) {
    return s.data_bits >= 16u ? (uint32_t)(rd.word(s.data_byte >> 3) >> (8u * (s.data_byte & 7u))) & 0xFFFFu : 0u;
}
template <class R>
FGC_HD uint32_t data_byte_at(R& rd, const StructView& s, uint32_t i) {  // (word-aligned structs only)
    return s.data_bits >= 8u * (i + 1u) ? (uint32_t)(rd.word((s.data_byte + i) >> 3) >> (8u * (i & 7u))) & 0xFFu : 0u;
}
template <class R>
FGC_HD uint64_t data_u64(R& rd, const StructView& s, uint32_t i) {  // (word-aligned structs only)
    return s.data_bits >= 64u * (i + 1u) ? rd.word((s.data_byte >> 3) + i) : 0ull;
}

struct NoSink {
    FGC_HD void put(uint32_t, fg_span, uint64_t, uint32_t, uint32_t) {}
};
// get_pairs (:65-113) over one list: the kept elements go to sink.put(k0 + kept so far, name, value, FG_T_*, FG_EF_*).
// Returns how many were kept.
template <class R, class Sink>
FGC_HD uint32_t walk_list(R& rd, const Msg& m, const ListView& l, bool extras, uint32_t k0, Sink& sink) {
    uint32_t kept = 0;
    if (!l.ok) return 0u;
    for (uint32_t e = 0; e < l.count; ++e) {
        const StructView s = element(l, e);
        fg_span key;
        if (!text_field(rd, m, s, 0u, &key)) continue;
        const uint32_t which = data_u16_0(rd, s);
        uint64_t val = 0;
        if (which == 0u) {
            fg_span v;
            if (!text_field(rd, m, s, 1u, &v)) continue;
            val = (uint64_t)v.off | ((uint64_t)v.len << 32);
        } else if (extras || which > 5u) {
            continue;  // extras keep strings only (:104-108); an unknown discriminant is NotInSchema (:97)
        } else if (which == 1u) {
            val = s.data_bits > 16u ? (rd.word((s.data_byte + 2u) >> 3) >> (8u * ((s.data_byte + 2u) & 7u))) & 1ull : 0ull;
        } else if (which != 5u) {
            val = data_u64(rd, s, 1u);
        }
        sink.put(k0 + kept, key, val, which, extras ? (uint32_t)FG_EF_NAME_VERBATIM : 0u);
        ++kept;
    }
    return kept;
}

// handle_message (:132-167): the row, the two lists resolved, the entries COUNTED (emit_entries writes them once they have slots)
template <class R>
FGC_HD void parse_message(R& rd, uint64_t len_bytes, Row& r, Msg& m) {
    const fg_span none{0u, FG_NONE};
    for (int k = 0; k < 6; ++k) r.sp[k] = none;
    if (!open_message(rd, len_bytes, &m) || m.seg0.len == 0u) {
        r.status = ST_NO_ROOT;
        return;
    }
    StructView root;  // a NULL root: every field its default
    root.seg = m.seg0;
    const uint64_t p = rd.word(m.seg0.start);
    if (p != 0ull) {
        Target t;
        if (!follow(rd, m, m.seg0, m.seg0.start, p, &t) || (t.lo & 3u) != 0u || !fits(t, (uint64_t)(t.hi & 0xFFFFu) + (t.hi >> 16))) {
            r.status = ST_NO_ROOT;
            return;
        }
        root.data_byte = t.at << 3;
        root.data_bits = (t.hi & 0xFFFFu) * 64u;
        root.ptr_at = t.at + (t.hi & 0xFFFFu);
        root.nptr = t.hi >> 16;
        root.seg = t.seg;
    }
    r.ts_bits = data_u64(rd, root, 0u);
    {   // ts.is_nan() || ts <= 0.0, on the bits: NaN, any negative (the sign bit), +0.0
        const uint64_t mag = r.ts_bits & 0x7FFFFFFFFFFFFFFFull;
        if (mag > 0x7FF0000000000000ull || (r.ts_bits >> 63) != 0ull || mag == 0ull) {
            r.status = ST_NO_TS;
            return;
        }
    }
    if (!text_field(rd, m, root, 0u, &r.sp[0])) {
        r.sp[0] = none;
        r.status = ST_NO_HOST;
        return;
    }
    const uint32_t fac = data_byte_at(rd, root, 8u), sev = data_byte_at(rd, root, 9u);
    r.fac = fac <= kFacilityMax ? fac : 0xFFu;
    r.sev = sev <= kSeverityMax ? sev : 0xFFu;
    for (uint32_t k = 1; k < 6u; ++k)
        if (!text_field(rd, m, root, k, &r.sp[k])) r.sp[k] = none;
    const bool id_ok = text_field(rd, m, root, 6u, &r.sd_id);
    if (!id_ok) r.sd_id = none;
    r.pairs = list_field(rd, m, root, 7u);
    r.extra = list_field(rd, m, root, 8u);
    r.sd = id_ok || r.pairs.ok || r.extra.ok;  // get_sd :115-130
    if (!r.sd) return;
    NoSink ns;
    r.n_ent = 1u + walk_list(rd, m, r.pairs, false, 0u, ns);
    r.n_ent += walk_list(rd, m, r.extra, true, 0u, ns);
}
// the row's entries: the element (FG_T_SDID; name = sd_id, len FG_NONE = None), the kept pairs, the kept extras
template <class R, class Sink>
FGC_HD void emit_entries(R& rd, const Msg& m, const Row& r, Sink& sink) {
    sink.put(0u, r.sd_id, 0ull, (uint32_t)FG_T_SDID, 0u);
    const uint32_t kp = walk_list(rd, m, r.pairs, false, 1u, sink);
    (void)walk_list(rd, m, r.extra, true, 1u + kp, sink);
}

}  // namespace capnp
}  // namespace fg
