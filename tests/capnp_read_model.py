"""Test helper: a Python model of flowgger's Cap'n Proto INPUT (splitter/capnp_splitter.rs:65-167) -- not product code.

`handle_message(msg)` restates the reference's `handle_message` / `get_sd` / `get_pairs` over a LENIENT reader of the wire
format: every getter returns its value or raises `GetterError`, by the rules capnp 0.14's `private/layout.rs` follows
(`read_struct_pointer`, `read_list_pointer`, `read_text_pointer`, `follow_fars`, `bounds_check`).  The crate cannot be
built here, so those rules are restated from knowledge of it and are UNPINNED beyond the reference's one vector (DESIGN
section 6 lists them).  Written over Python integers and byte slices, independently of flowgger_amd/csrc/fg_capnp_parse.hpp:
segments are separate byte strings here, absolute word indices there.

Result: `("err", text)` or `("ok", Record, skipped)` where `skipped` counts the pairs / extras the reference `continue`s over.
"""
from __future__ import annotations

import math
import struct
from typing import List, Optional, Tuple

from flowgger_amd.record import SD_BOOL, SD_F64, SD_I64, SD_NULL, SD_STRING, SD_U64, Record, SDValue, StructuredData

MAX_SEGMENTS = 512          # capnp 0.14 serialize.rs: "Too many segments"
TRAVERSAL_WORDS = 8 << 20   # ReaderOptions::new()
FACILITY_MAX, SEVERITY_MAX = 0xFF >> 3, 7
ERR_TS, ERR_HOST, ERR_ROOT = "Missing timestamp", "Missing host name", "Capnp decoding error: the root pointer cannot be read"


class GetterError(Exception):
    pass


class _Msg:
    """the segments of one message; a segment is what the table says, cut at the end of the message"""

    def __init__(self, msg: bytes):
        if len(msg) < 8 or len(msg) >= 1 << 32:
            raise GetterError("no segment table")
        msg = msg[:len(msg) & ~7]
        (n1,) = struct.unpack_from("<I", msg, 0)
        n = n1 + 1
        if n >= MAX_SEGMENTS:
            raise GetterError("too many segments")
        table = (4 + 4 * n + 7) // 8 * 8
        if table > len(msg):
            raise GetterError("truncated segment table")
        sizes = struct.unpack_from(f"<{n}I", msg, 4)
        self.segs: List[bytes] = []
        self.base: List[int] = []  # byte offset of each segment in the message (for the spans)
        p = table
        for sz in sizes:
            p = min(p, len(msg))
            self.base.append(p)
            self.segs.append(msg[p:p + 8 * sz])
            p += 8 * sz

    def words(self, seg: int) -> int:
        return len(self.segs[seg]) // 8

    def word(self, seg: int, w: int) -> int:
        assert 0 <= w < self.words(seg), "the model itself read outside a segment"
        return struct.unpack_from("<Q", self.segs[seg], 8 * w)[0]


def _signed30(lo: int) -> int:
    off = (lo & 0xFFFF_FFFF) >> 2
    return off - (1 << 30) if off >= 1 << 29 else off


def _follow(m: _Msg, seg: int, w: int, p: int) -> Tuple[int, int, int]:
    """follow_fars for the non-null pointer p at (seg, w): (segment, first word of the object, the pointer describing it)"""
    if p & 3 != 2:
        t = w + 1 + _signed30(p)
        if not 0 <= t <= m.words(seg):
            raise GetterError("out-of-bounds pointer")
        return seg, t, p
    fseg, pos, dbl = p >> 32, (p & 0xFFFF_FFFF) >> 3, bool(p & 4)
    if fseg >= len(m.segs):
        raise GetterError("far pointer to a segment that is not there")
    if pos + (2 if dbl else 1) > m.words(fseg):
        raise GetterError("landing pad out of bounds")
    pad = m.word(fseg, pos)
    if not dbl:
        t = pos + 1 + _signed30(pad)
        if not 0 <= t <= m.words(fseg):
            raise GetterError("out-of-bounds pointer in a landing pad")
        return fseg, t, pad
    oseg, opos = pad >> 32, (pad & 0xFFFF_FFFF) >> 3
    if oseg >= len(m.segs) or opos > m.words(oseg):
        raise GetterError("double-far pad leads nowhere")
    return oseg, opos, m.word(fseg, pos + 1)


def _utf8_ok(b: bytes) -> bool:
    try:
        b.decode("utf-8")  # Python's strict decoder applies Unicode table 3-7 (no surrogates, no overlongs, <= U+10FFFF)
        return True
    except UnicodeDecodeError:
        return False


class _Struct:
    def __init__(self, m: _Msg, seg: int = 0, data_byte: int = 0, data_bits: int = 0, ptr_word: int = 0, nptr: int = 0):
        self.m, self.seg, self.data_byte, self.data_bits, self.ptr_word, self.nptr = m, seg, data_byte, data_bits, ptr_word, nptr

    def uint(self, bit_offset: int, bits: int) -> int:
        """a data field; beyond the data section it reads as 0"""
        if bit_offset + bits > self.data_bits:
            return 0
        raw = self.m.segs[self.seg]
        v = int.from_bytes(raw[self.data_byte + bit_offset // 8:self.data_byte + (bit_offset + bits + 7) // 8], "little")
        return (v >> (bit_offset % 8)) & ((1 << bits) - 1)

    def text(self, k: int) -> Tuple[int, bytes]:
        """(byte offset in the message, content) of pointer field k; raises GetterError"""
        if k >= self.nptr:
            return 0, b""
        m, w = self.m, self.ptr_word + k
        p = m.word(self.seg, w)
        if p == 0:
            return 0, b""
        seg, at, q = _follow(m, self.seg, w, p)
        if q & 3 != 1:
            raise GetterError("non-list pointer where text was expected")
        if (q >> 32) & 7 != 2:
            raise GetterError("list of non-bytes where text was expected")
        n = q >> 35
        if at + (n + 7) // 8 > m.words(seg):
            raise GetterError("text out of bounds")
        if n == 0:
            raise GetterError("text without its NUL")
        raw = m.segs[seg][8 * at:8 * at + n]
        if raw[-1] != 0:
            raise GetterError("text not NUL-terminated")
        if not _utf8_ok(raw[:-1]):
            raise GetterError("text not UTF-8")
        return m.base[seg] + 8 * at, raw[:-1]

    def struct_list(self, k: int) -> List["_Struct"]:
        m = self.m
        p = m.word(self.seg, self.ptr_word + k) if k < self.nptr else 0
        if p == 0:
            return []
        seg, at, q = _follow(m, self.seg, self.ptr_word + k, p)
        if q & 3 != 1:
            raise GetterError("non-list pointer where a list was expected")
        es, cnt = (q >> 32) & 7, q >> 35
        if es == 7:
            if at + cnt + 1 > m.words(seg):
                raise GetterError("list out of bounds")
            tag = m.word(seg, at)
            if tag & 3 != 0:
                raise GetterError("inline-composite tag is not a struct")
            n, dw, pc = (tag & 0xFFFF_FFFF) >> 2, (tag >> 32) & 0xFFFF, tag >> 48
            if n * (dw + pc) > cnt:
                raise GetterError("elements overrun the word count")
            if dw + pc == 0 and n > TRAVERSAL_WORDS:
                raise GetterError("amplification")
            return _Lazy(n, lambda e: _Struct(m, seg, 8 * (at + 1 + e * (dw + pc)), 64 * dw, at + 1 + e * (dw + pc) + dw, pc))
        if es == 1:
            raise GetterError("bit list where a struct list was expected")
        bits = {0: 0, 2: 8, 3: 16, 4: 32, 5: 64, 6: 64}[es]
        if at + (cnt * bits + 63) // 64 > m.words(seg):
            raise GetterError("list out of bounds")
        if bits == 0 and cnt > TRAVERSAL_WORDS:
            raise GetterError("amplification")
        if es == 6:
            return _Lazy(cnt, lambda e: _Struct(m, seg, 8 * (at + e), 0, at + e, 1))
        return _Lazy(cnt, lambda e: _Struct(m, seg, 8 * at + e * bits // 8, bits, 0, 0))


class _Lazy:
    """a list of structs made on demand (a void list may claim millions of elements)"""

    def __init__(self, n, make):
        self.n, self.make = n, make

    def __len__(self):
        return self.n

    def __iter__(self):
        return (self.make(e) for e in range(self.n))


def _root(m: _Msg) -> _Struct:
    if m.words(0) == 0:
        raise GetterError("segment 0 is empty")
    p = m.word(0, 0)
    if p == 0:
        return _Struct(m)
    seg, at, q = _follow(m, 0, 0, p)
    if q & 3 != 0:
        raise GetterError("root is not a struct pointer")
    dw, pc = (q >> 32) & 0xFFFF, q >> 48
    if at + dw + pc > m.words(seg):
        raise GetterError("root struct out of bounds")
    return _Struct(m, seg, 8 * at, 64 * dw, at + dw, pc)


def _s(b: bytes) -> str:
    return b.decode("utf-8")


def _value(p: _Struct):
    """Pair.value.which() -> SDValue, or None for NotInSchema / a failed string getter"""
    which = p.uint(0, 16)
    if which == 0:
        return SDValue(SD_STRING, _s(p.text(1)[1]))  # (GetterError -> the caller skips)
    if which == 1:
        return SDValue(SD_BOOL, bool(p.uint(16, 1)))
    if which == 2:
        return SDValue(SD_F64, struct.unpack("<d", struct.pack("<Q", p.uint(64, 64)))[0])
    if which == 3:
        return SDValue(SD_I64, struct.unpack("<q", struct.pack("<Q", p.uint(64, 64)))[0])
    if which == 4:
        return SDValue(SD_U64, p.uint(64, 64))
    if which == 5:
        return SDValue(SD_NULL)
    return None


def handle_message(msg: bytes, max_pairs: Optional[int] = None):
    """-> ("err", text) | ("ok", Record, skipped).  max_pairs: give up (("big", n)) on a list with more elements than that."""
    try:
        m = _Msg(msg)
        root = _root(m)
    except GetterError:
        return ("err", ERR_ROOT)
    ts = struct.unpack("<d", struct.pack("<Q", root.uint(0, 64)))[0]
    if math.isnan(ts) or ts <= 0.0:
        return ("err", ERR_TS)
    try:
        hostname = _s(root.text(0)[1])
    except GetterError:
        return ("err", ERR_HOST)
    fac, sev = root.uint(64, 8), root.uint(72, 8)

    def opt(k):
        try:
            return _s(root.text(k)[1])
        except GetterError:
            return None
    appname, procid, msgid, text, full = (opt(k) for k in range(1, 6))
    sd_id = opt(6)
    lists = []
    for k in (7, 8):
        try:
            lists.append(root.struct_list(k))
        except GetterError:
            lists.append(None)
    pairs_l, extra_l = lists
    skipped = 0
    if pairs_l is None and extra_l is None:
        sd = None if sd_id is None else [StructuredData(None if sd_id is None else sd_id, [])]
    else:
        if max_pairs is not None and len(pairs_l or []) + len(extra_l or []) > max_pairs:
            return ("big", len(pairs_l or []) + len(extra_l or []))
        pairs: List[Tuple[str, SDValue]] = []
        for p in pairs_l or []:
            try:
                name = _s(p.text(0)[1])
                val = _value(p)
            except GetterError:
                skipped += 1
                continue
            if val is None:
                skipped += 1
                continue
            pairs.append((name if name.startswith("_") else "_" + name, val))
        for p in extra_l or []:
            try:
                name = _s(p.text(0)[1])
                val = _value(p)
            except GetterError:
                skipped += 1
                continue
            if val is None or val.kind != SD_STRING:
                skipped += 1
                continue
            pairs.append((name, val))
        sd = [StructuredData(sd_id, pairs)]
    rec = Record(ts=ts, hostname=hostname, facility=fac if fac <= FACILITY_MAX else None, severity=sev if sev <= SEVERITY_MAX else None,
                 appname=appname, procid=procid, msgid=msgid, msg=text, full_msg=full, sd=sd)
    return ("ok", rec, skipped)


def frame_stream(buf: bytes) -> Tuple[List[int], int, Optional[str]]:
    """capnp::serialize::read_message's framing over a byte stream: (offsets of the whole messages, bytes consumed, the
    error that ends the connection or None)"""
    offs, p = [0], 0
    while len(buf) - p >= 8:
        n = struct.unpack_from("<I", buf, p)[0] + 1
        if n >= MAX_SEGMENTS:
            return offs, p, "Too many segments"
        table = (4 + 4 * n + 7) // 8 * 8
        if len(buf) - p < table:
            break
        total = sum(struct.unpack_from(f"<{n}I", buf, p + 4))
        if total > TRAVERSAL_WORDS:
            return offs, p, "Message is too large"
        if len(buf) - p < table + 8 * total:
            break
        p += table + 8 * total
        offs.append(p)
    return offs, p, None
