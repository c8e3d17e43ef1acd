"""Test helper: a clean-room model of flowgger's Cap'n Proto output (encoder/capnp_encoder.rs, schema record.capnp) -- not product
code.

`serialize(record, extra)` builds the message the reference writes: `Builder::new_default()`, `build_record`, then
`capnp::serialize::write_message`, with capnp 0.14's allocator (first segment 1024 words; an object that does not fit the segment of
its pointer takes a landing pad + far pointer in the first segment with room, else in a new segment of max(size + 1, next_size),
next_size growing by each new segment's size).  `parse(message)` is an independent reader: segment table, near and far pointers,
landing pads, inline-composite lists -- back to a Record (only sd[0] exists on the wire) and the extra pairs.
"""
from __future__ import annotations

import struct
from typing import List, Optional, Tuple

from flowgger_amd.record import (SD_BOOL, SD_F64, SD_I64, SD_NULL, SD_STRING, SD_U64, Record, SDValue,
                                 StructuredData)

SEG0_WORDS = 1024
DISCRIMINANT = {SD_STRING: 0, SD_BOOL: 1, SD_F64: 2, SD_I64: 3, SD_U64: 4, SD_NULL: 5}
KIND_OF = {v: k for k, v in DISCRIMINANT.items()}
ROOT_PTR = 0x0009_0002_0000_0000  # struct pointer, offset 0, 2 data words, 9 pointers


def _b(s: str) -> bytes:
    return s.encode("utf-8", "surrogateescape")


def _s(b: bytes) -> str:
    return b.decode("utf-8", "surrogateescape")


def text_ptr_hi(n: int) -> int:
    return 2 | (n + 1) << 3


def list_ptr_hi(n: int) -> int:
    return 7 | (4 * n) << 3


class _Arena:
    def __init__(self):
        self.segs = [bytearray(8)]  # the root pointer's word
        self.cap = [SEG0_WORDS]
        self.next = 2 * SEG0_WORDS

    def used(self, s):
        return len(self.segs[s]) // 8

    def alloc(self, home: int, words: int) -> Tuple[int, int, bool]:
        """(segment, first word, far)"""
        if self.cap[home] - self.used(home) >= words:
            pos = self.used(home)
            self.segs[home] += bytes(8 * words)
            return home, pos, False
        for s in range(len(self.segs)):
            if self.cap[s] - self.used(s) >= words + 1:
                pos = self.used(s) + 1
                self.segs[s] += bytes(8 * (words + 1))
                return s, pos, True
        c = max(words + 1, self.next)
        self.next += c
        self.segs.append(bytearray(8 * (words + 1)))
        self.cap.append(c)
        return len(self.segs) - 1, 1, True

    def put(self, seg: int, word: int, value: int):
        struct.pack_into("<Q", self.segs[seg], 8 * word, value & 0xFFFF_FFFF_FFFF_FFFF)

    def point(self, pseg: int, pword: int, place, hi: int):
        """list pointer at (pseg, pword) to the object at `place` (hi: its upper 32 bits)"""
        seg, pos, far = place
        if far:
            self.put(pseg, pword, 2 | (pos - 1) << 3 | seg << 32)
            self.put(seg, pos - 1, 1 | hi << 32)  # the landing pad: the same pointer, offset 0
        else:
            self.put(pseg, pword, 1 | (pos - pword - 1) << 2 | hi << 32)

    def text(self, pseg: int, pword: int, data: bytes):
        place = self.alloc(pseg, (len(data) + 8) // 8)
        seg, pos, _ = place
        self.segs[seg][8 * pos:8 * pos + len(data)] = data
        self.point(pseg, pword, place, text_ptr_hi(len(data)))

    def pairs(self, pseg: int, pword: int, items: List[Tuple[bytes, SDValue]]):
        n = len(items)
        place = self.alloc(pseg, 1 + 4 * n)
        seg, pos, _ = place
        self.point(pseg, pword, place, list_ptr_hi(n))
        self.put(seg, pos, n << 2 | (2 | 2 << 16) << 32)  # tag: n elements, 2 data words, 2 pointers
        for i, (key, val) in enumerate(items):
            sw = pos + 1 + 4 * i
            d0 = DISCRIMINANT[val.kind]
            if val.kind == SD_BOOL and val.value:
                d0 |= 1 << 16
            self.put(seg, sw, d0)
            if val.kind == SD_F64:
                self.put(seg, sw + 1, struct.unpack("<Q", struct.pack("<d", val.value))[0])
            elif val.kind == SD_I64:
                self.put(seg, sw + 1, val.value)
            elif val.kind == SD_U64:
                self.put(seg, sw + 1, val.value)
            self.text(seg, sw + 2, key)
            if val.kind == SD_STRING:
                self.text(seg, sw + 3, _b(val.value))


def serialize(rec: Record, extra: Optional[List[Tuple[str, str]]] = None) -> bytes:
    """CapnpEncoder::encode(rec) with output.capnp_extra = `extra` (sorted by key, as the configuration table iterates)"""
    a = _Arena()
    a.alloc(0, 11)
    a.put(0, 0, ROOT_PTR)
    a.put(0, 1, struct.unpack("<Q", struct.pack("<d", rec.ts))[0])
    a.put(0, 2, (0xFF if rec.facility is None else rec.facility) | (0xFF if rec.severity is None else rec.severity) << 8)
    a.text(0, 3, _b(rec.hostname))
    for j, f in enumerate((rec.appname, rec.procid, rec.msgid, rec.msg, rec.full_msg)):
        if f is not None:
            a.text(0, 4 + j, _b(f))
    if rec.sd is not None:
        el = rec.sd[0]  # only the first StructuredData is encoded (capnp_encoder.rs:79-81)
        if el.sd_id is not None:
            a.text(0, 9, _b(el.sd_id))
        a.pairs(0, 10, [(_b(k), v) for k, v in el.pairs])
    if extra:
        a.pairs(0, 11, [(_b(k), SDValue(SD_STRING, v)) for k, v in extra])
    n = len(a.segs)
    table = [n - 1] + [a.used(s) for s in range(n)]
    if len(table) % 2:
        table.append(0)
    return struct.pack(f"<{len(table)}I", *table) + b"".join(bytes(s) for s in a.segs)


# ---- the reader ----------------------------------------------------------------------------------
class WireError(Exception):
    pass


def _word(segs, seg, w):
    if not 0 <= w < len(segs[seg]) // 8:
        raise WireError(f"word {w} outside segment {seg}")
    return struct.unpack_from("<Q", segs[seg], 8 * w)[0]


def _deref(segs, seg, w):
    """the pointer at (seg, w) -> (its non-far form, the segment and word its target starts at), or None when null"""
    p = _word(segs, seg, w)
    if p == 0:
        return None
    if p & 3 == 2:
        if p & 4:
            raise WireError("double-far pointer")
        tseg, pad = p >> 32, (p & 0xFFFF_FFFF) >> 3
        q = _word(segs, tseg, pad)
        if q & 3 == 2 or (q & 0xFFFF_FFFF) >> 2 != 0:
            raise WireError("landing pad is not a pointer with offset 0")
        return q, tseg, pad + 1
    off = (p & 0xFFFF_FFFF) >> 2
    if off >= 1 << 29:
        off -= 1 << 30
    return p, seg, w + 1 + off


def _text(segs, seg, w) -> Optional[bytes]:
    r = _deref(segs, seg, w)
    if r is None:
        return None
    p, tseg, tw = r
    if p & 3 != 1 or (p >> 32) & 7 != 2:
        raise WireError("not a byte list")
    n = p >> 35
    if n < 1:
        raise WireError("text without its NUL")
    raw = bytes(segs[tseg][8 * tw:8 * tw + n])
    if len(raw) != n or raw[-1] != 0:
        raise WireError("text not NUL-terminated")
    pad = bytes(segs[tseg][8 * tw + n:8 * tw + (n + 7) // 8 * 8])
    if any(pad):
        raise WireError("nonzero text padding")
    return raw[:-1]


def _pairs(segs, seg, w) -> Optional[List[Tuple[str, SDValue]]]:
    r = _deref(segs, seg, w)
    if r is None:
        return None
    p, tseg, tw = r
    if p & 3 != 1 or (p >> 32) & 7 != 7:
        raise WireError("not an inline-composite list")
    tag = _word(segs, tseg, tw)
    n, dw, pw = (tag & 0xFFFF_FFFF) >> 2, (tag >> 32) & 0xFFFF, tag >> 48
    if (dw, pw) != (2, 2) or p >> 35 != 4 * n:
        raise WireError("unexpected Pair layout")
    out = []
    for i in range(n):
        sw = tw + 1 + 4 * i
        d0, d1 = _word(segs, tseg, sw), _word(segs, tseg, sw + 1)
        kind = KIND_OF[d0 & 0xFFFF]
        key = _s(_text(segs, tseg, sw + 2))
        if kind == SD_STRING:
            val = SDValue(kind, _s(_text(segs, tseg, sw + 3)))
        elif kind == SD_BOOL:
            val = SDValue(kind, bool(d0 >> 16 & 1))
        elif kind == SD_F64:
            val = SDValue(kind, struct.unpack("<d", struct.pack("<Q", d1))[0])
        elif kind == SD_I64:
            val = SDValue(kind, struct.unpack("<q", struct.pack("<Q", d1))[0])
        elif kind == SD_U64:
            val = SDValue(kind, d1)
        else:
            val = SDValue(kind)
        out.append((key, val))
    return out


def parse(msg: bytes) -> Tuple[Record, List[Tuple[str, str]], int]:
    """one message -> (Record with at most sd[0], the extra pairs, bytes consumed)"""
    (n1,) = struct.unpack_from("<I", msg, 0)
    n = n1 + 1
    sizes = struct.unpack_from(f"<{n}I", msg, 4)
    p = (4 + 4 * n + 7) // 8 * 8
    segs = []
    for sz in sizes:
        segs.append(msg[p:p + 8 * sz])
        if len(segs[-1]) != 8 * sz:
            raise WireError("truncated segment")
        p += 8 * sz
    if _word(segs, 0, 0) & 0xFFFF_FFFF_0000_0003 != ROOT_PTR:
        raise WireError("unexpected root pointer")
    r = _deref(segs, 0, 0)
    _, rseg, rw = r
    ts = struct.unpack("<d", struct.pack("<Q", _word(segs, rseg, rw)))[0]
    d1 = _word(segs, rseg, rw + 1)
    fac, sev = d1 & 0xFF, d1 >> 8 & 0xFF
    t = [_text(segs, rseg, rw + 2 + j) for j in range(7)]
    host = t[0]
    if host is None:
        raise WireError("hostname is always set")
    pairs = _pairs(segs, rseg, rw + 9)
    extra = _pairs(segs, rseg, rw + 10)
    sd = None
    if pairs is not None:
        sd = [StructuredData(None if t[6] is None else _s(t[6]), pairs)]
    elif t[6] is not None:
        raise WireError("sd_id without pairs")
    rec = Record(ts=ts, hostname=_s(host), facility=None if fac == 0xFF else fac, severity=None if sev == 0xFF else sev,
                 appname=None if t[1] is None else _s(t[1]), procid=None if t[2] is None else _s(t[2]),
                 msgid=None if t[3] is None else _s(t[3]), msg=None if t[4] is None else _s(t[4]),
                 full_msg=None if t[5] is None else _s(t[5]), sd=sd)
    return rec, [(k, v.value) for k, v in (extra or [])], p


def first_sd_only(rec: Record) -> Record:
    """what the wire can hold of `rec`"""
    return Record(**{**rec.__dict__, "sd": None if rec.sd is None else rec.sd[:1]})


def record_key(rec: Record):
    """a comparable form: floats by their bits (NaN payloads, -0.0)"""
    bits = lambda x: struct.pack("<d", x)

    def val(v):
        return (v.kind, bits(v.value) if v.kind == SD_F64 else v.value)
    sd = None if rec.sd is None else [(e.sd_id, [(k, val(v)) for k, v in e.pairs]) for e in rec.sd]
    return (bits(rec.ts), rec.hostname, rec.facility, rec.severity, rec.appname, rec.procid, rec.msgid, rec.msg, rec.full_msg, sd)


def frame(msg: bytes, merger: int) -> bytes:
    """merger/{line,nul,syslen}_merger.rs around one message (0 none, 1 line, 2 nul, 3 syslen)"""
    if merger == 1:
        return msg + b"\n"
    if merger == 2:
        return msg + b"\0"
    if merger == 3:
        return str(len(msg) + 1).encode() + b" " + msg + b"\n"
    return msg


def unframe(data: bytes, merger: int) -> bytes:
    """the message inside one frame()"""
    if merger == 3:
        data = data[data.index(b" ") + 1:]
    return data[:-1] if merger in (1, 2, 3) else data
