"""Lines that aim a run of backslashes and the quote behind it at every boundary across which the two decode kernels carry escape
state: the GELF fast form (flowgger_amd/csrc/fg_gelf2.hpp: find_escaped per 64-byte word, the carry inside a lane's range and between
lanes, the string parity and its toggle pass, the 64-bit windows of a member) and the structured-data walk of RFC5424 (fg_sd2.hpp:
find_escaped16 per 16-byte chunk, the carry between lanes and between the 1 KiB trips of classify_tile, HEAD rows).  Pure Python, no
GPU (test infrastructure); what tests/utf8_hazards.py is for the UTF-8 verdicts of fused framing.

A hazard is `pad` text bytes, a run of r backslashes, a quote and a tail: an even run leaves the quote real, an odd one escapes it, and
every tail gives the oracle a definite Record or error both ways.

Position invariants (asserted on every built stream, check_invariants):
  * a tile starts at offsets[first line of the group] & ~15 (fg_pipeline.hpp, geometry), the fused kernels' at T * S - 16 with S a
    multiple of 16: absolute offset == tile offset mod 16 under every grouping.  That is all the 16-byte chunks of the SD walk need.
  * GELF `fine`, `coarse`, `toggle`: every frame (line + terminator) is a multiple of 64 bytes -- `toggle`: every PAIR of frames, the
    second of which is never the first of a group of an even number of lines cut by count -- so whichever line a group starts with, it
    starts at a multiple of 64 and the residue of a hazard mod 64 in the tile is its absolute one.  A fused tile is not tied to a line
    start: `fine` orders its lines so that every run still meets every residue of a fused tile's words (fused_residue).
  * `coarse`: every frame is 768 bytes (GELF: twelve words, a multiple of the wn = 1, 2, 3, 4, 6 words a lane owns, so the lane-range
    edges of the word pass fall on word boundaries of the lines, each of which holds a hazard) or 2048 bytes (SD: a line's offset 1024
    is a trip edge of classify_tile)."""
from __future__ import annotations

from collections import Counter
from typing import Dict, List, NamedTuple, Optional, Tuple

GELF, SD = "gelf", "sd"
NONE, LINE, NUL = 0, 1, 2  # (= FG_FRAME_NONE / _LINE / _NUL): bare lines, or a stream with "\n" / "\0" behind every line

RUNS = tuple(range(1, 9)) + (15, 16, 17, 31, 32, 33, 62, 63, 64, 65, 66, 127, 128, 129)
FAST_MAX = {GELF: 62, SD: 15}   # the longest even run the fast form must handle itself
LONG_FROM = {GELF: 64, SD: 16}  # a run this long can fill a 64-byte word / a 16-byte chunk: the tile bails -- streams of their own
WORD = {GELF: 64, SD: 16}       # the fine boundary
COARSE_LINE = {GELF: 768, SD: 2048}
HEAD_CAP = 1024

HDR = b"<13>1 2015-08-05T15:53:45.637824Z host app 1234 ID7 "
HEAD = {GELF: b'{"host":"h","s":"', SD: HDR + b'[a b="'}

# position classes -> the formats they apply to
CLASSES: Dict[str, Tuple[str, ...]] = {
    "fine": (GELF, SD),       # the escaped character at every residue of the 64-byte words / 16-byte chunks
    "coarse": (GELF, SD),     # around the lane-range edges of the word pass / the 1 KiB trip edge of classify_tile
    "member": (GELF,),        # the value's closing quote and its escapes relative to the member's 64-bit windows
    "odd-end": (GELF, SD),    # a line that ends in an odd run, the next one begins with a quote
    "round-up": (GELF, SD),   # the last line of a tile ends 0 .. 15 bytes before a 16-byte boundary: the next line's first bytes are staged
    "toggle": (GELF, SD),     # an odd-quote line immediately before a hazard line that starts at bit 0, 1, 63 of a word
    "head-cap": (SD,),        # the run straddles the cut end of a HEAD row
}


class Tail(NamedTuple):
    name: str
    head: bytes
    fill: bytes  # repeated to stretch the line to an exact length
    end: bytes

    def make(self, k: int = 0) -> bytes:
        return self.head + self.fill * k + self.end


TAILS = {
    GELF: [Tail("member", b',"t":"z', b"z", b'"}'), Tail("close", b"}", b" ", b""), Tail("number", b',"t":1}', b" ", b"")],
    SD: [Tail("pair", b' c="d"] m', b"m", b""), Tail("close", b"] m", b"m", b""), Tail("element", b'][e f="g"] m', b"m", b""),
         Tail("quoted", b'] "q" m', b"m", b"")],
}


class Hz(NamedTuple):
    line: bytes
    cls: str
    run: int = 0            # backslashes of the run (0: a helper -- an everyday, odd-quote or oversized line)
    q: int = -1             # line offset of the quote behind the run
    tail: str = ""
    at: Optional[Tuple[int, int]] = None  # (residue, modulus) the line's absolute start must have (a filler in front sees to it)
    msg_at: int = -1        # SD, even run: line offset of the ' ' that starts the message
    want: int = -1          # the residue / offset the class aims the quote at (checked by check_invariants)

    def must(self, fmt: str) -> bool:
        """the fast form must handle the line itself: an even run it can carry, a well-formed tail (every tail is)"""
        return self.run != 0 and self.run % 2 == 0 and self.run <= FAST_MAX[fmt]


class Stream(NamedTuple):
    name: str
    fmt: str
    cls: str
    framing: int
    bail: bool              # holds runs that take whole tiles off the fast form
    hz: List[Hz]            # one per frame
    raw: bytes
    offsets: List[int]      # frame i = raw[offsets[i]:offsets[i + 1]], its terminator included

    def lines(self) -> List[bytes]:
        return [h.line for h in self.hz]


def term_of(framing: int) -> bytes:
    return b"" if framing == NONE else b"\n" if framing == LINE else b"\0"


def hazard(fmt: str, cls: str, q: int, r: int, tail: Tail, length: Optional[int] = None, at=None, want: int = -1) -> Optional[Hz]:
    """HEAD, pad bytes, r backslashes, the quote at line offset q, the tail stretched to `length`; None when it does not fit"""
    pad = q - len(HEAD[fmt]) - r
    body_len = q + 1
    k = 0 if length is None else length - body_len - len(tail.make())
    if pad < 0 or k < 0:
        return None
    line = HEAD[fmt] + b"x" * pad + b"\\" * r + b'"' + tail.make(k)
    assert line[q:q + 1] == b'"' and line[q - r:q] == b"\\" * r and (length is None or len(line) == length)
    msg_at = -1
    if fmt == SD and r % 2 == 0:
        msg_at = q + line[q:].index(b"] ") + 1
    return Hz(line, cls, r, q, tail.name, at, msg_at, want)


def everyday(fmt: str, length: int, i: int = 0) -> bytes:
    a, z = (b'{"host":"h%d","short_message":"' % (i % 10), b'","_n":%d}' % (i % 10)) if fmt == GELF else \
        (HDR + b'[o p="q%d" r="s"] ' % (i % 10), b"")
    assert length >= len(a) + len(z) + 1, length
    return a + b"m" * (length - len(a) - len(z)) + z


MIN_EVERYDAY = {GELF: 48, SD: 80}


def up(v: int, m: int) -> int:
    return -(-v // m) * m


def assemble(name: str, fmt: str, cls: str, framing: int, hz: List[Hz], bail: bool = False) -> Stream:
    t = term_of(framing)
    out = bytearray()
    frames: List[Hz] = []
    offsets = [0]
    for i, h in enumerate(hz):
        if h.at is not None:
            res, m = h.at
            need = (res - len(out)) % m
            if need:
                while need < MIN_EVERYDAY[fmt] + len(t):
                    need += m
                out += everyday(fmt, need - len(t), i) + t
                frames.append(Hz(bytes(out[offsets[-1]:len(out) - len(t)]), cls))
                offsets.append(len(out))
            assert len(out) % m == res
        out += h.line + t
        frames.append(h)
        offsets.append(len(out))
    return Stream(name, fmt, cls, framing, bail, frames, bytes(out), offsets)


# ---- the classes ------------------------------------------------------------------------------------------------------------------
def short_runs(fmt: str) -> List[int]:
    return [r for r in RUNS if r < LONG_FROM[fmt]]


def long_runs(fmt: str) -> List[int]:
    return [r for r in RUNS if r >= LONG_FROM[fmt]]


def fine(fmt: str, framing: int, runs: List[int], cls: str = "fine", every: int = 0, reps: int = 1) -> List[Hz]:
    """every run with the quote at every residue of the word; frames are multiples of the word.  The residues come in quads 16 a + b,
    a = 0 .. 3, each quad `reps` times in a row (fused_residue has the reason).  every = k: an everyday line behind every k-th hazard"""
    W, tl, t = WORD[fmt], TAILS[fmt], len(term_of(framing))
    out: List[Hz] = []
    order = [16 * a + b for b in range(16) for _ in range(reps) for a in range(W // 16)]
    for r in runs:
        for res in order:
            lo = len(HEAD[fmt]) + r
            q = lo + (res - lo) % W
            tail = tl[(r + res) % len(tl)]
            h = hazard(fmt, cls, q, r, tail, up(q + 1 + len(tail.make()) + t, W) - t, want=res)
            out.append(h)
            if every and len(out) % every == 0:
                out.append(Hz(everyday(fmt, up(MIN_EVERYDAY[fmt] + 17 * (res % 5) + t, W) - t, res), cls))
    return out


def fused_residue(s: "Stream", i: int, S: int) -> int:
    """residue mod 64, in the tile of a FUSED launch, of hazard i's quote.  A fused tile is a byte tile of the raw stream -- tile T stages
    the stream from T * S - 16 on and decodes the lines that start in [T * S, T * S + S) (fg_fused.hpp) --, so it is not tied to a line
    start, and S is a multiple of 16 only: the words of tile T are shifted by (16 - T * S) mod 64 against the stream.  Four lines in a
    row whose absolute residues are 16 a + b, a = 0 .. 3, meet all four residues = b mod 16 of the tile's words when they start in one
    tile; `fine` has every quad twice in a row (eight frames, 1.5 KiB at most: one tile edge among them at most for S >= 1.5 KiB)."""
    a = s.offsets[i]
    return (a + s.hz[i].q + 16 - (a // S) * S) % 64


def coarse(fmt: str, framing: int) -> List[Hz]:
    tl, t, n = TAILS[fmt], len(term_of(framing)), COARSE_LINE[fmt]
    out: List[Hz] = []
    if fmt == GELF:
        edges, runs = [64 * k for k in range(1, 12)], (1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 62, 63)
    else:
        edges, runs = [1024], (1, 2, 3, 4, 5, 6, 7, 8, 15)
    i = 0
    for r in runs:
        for e in edges:
            for d in range(-3, 4):
                for tail in (tl if fmt == SD else tl[i % 3:i % 3 + 1]):
                    h = hazard(fmt, "coarse", e + d, r, tail, n - t, want=e + d)
                    i += 1
                    if h is not None:
                        out.append(h)
    return out


# the escapes of a GELF string value: valid ones, and the two serde_json refuses
ESCAPES = [b'\\"', b"\\\\", b"\\n", b"\\u00e9", b"\\ud83d\\ude00", b"\\q", b"\\ud83d"]
MEMBER_ITEM = 11  # line offset of the ',' that owns the member `"s":"..."` of member_line


def member_line(D: int, escapes: List[Tuple[int, bytes]]) -> Optional[bytes]:
    """the closing quote of "s"'s value D bytes behind the member's item (the ',' at line offset 11: bit i of the member's first
    window is byte 12 + i, the body starts at bit 5, the closing quote is bit D - 1); escapes = (window bit of the backslash, bytes)"""
    body = bytearray(b"x" * (D - 6))
    used = set()
    for bit, e in escapes:
        a = bit - 5
        span = set(range(a, a + len(e)))
        if a < 0 or a + len(e) > len(body) or used & span:
            return None
        used |= span
        body[a:a + len(e)] = e
    line = b'{"host":"h","s":"' + bytes(body) + b'","t":"z"}'
    assert line[MEMBER_ITEM:MEMBER_ITEM + 1] == b"," and line[MEMBER_ITEM + D:MEMBER_ITEM + D + 1] == b'"'
    return line


def member() -> List[Hz]:
    out: List[Hz] = []
    for D in list(range(58, 71)) + list(range(122, 135)):
        out.append(Hz(member_line(D, []), "member", 0, MEMBER_ITEM + D, "none", want=D))
        for e in ESCAPES:
            places = {5, D - 1 - len(e)} | {b for b in (62, 63, 64, 65, 126, 127, 128, 129)}
            for bit in sorted(places):
                ln = member_line(D, [(bit, e)])
                if ln is not None:
                    out.append(Hz(ln, "member", 1, MEMBER_ITEM + D, e.decode(), want=D))
        # the `simple` shortcut: exactly one two-byte escape is above; two escapes; one at bit 62 / 63 with a second one behind
        for a, b in ((5, D - 3), (62, D - 3), (63, D - 3), (5, 8), (D - 5, D - 3)):
            ln = member_line(D, [(a, b"\\n"), (b, b"\\t")])
            if ln is not None:
                out.append(Hz(ln, "member", 2, MEMBER_ITEM + D, "two", want=D))
    return out


def odd_end(fmt: str) -> List[Hz]:
    """a line that ends in an odd run (an unterminated value), then a line that begins with a quote: unframed the run and the quote are
    neighbours in the tile, framed a terminator stands between them.  Everyday lines around them must still decode."""
    out: List[Hz] = []
    nxt = [b'"', b'"{"host":"h"}', b'" {"host":"h","s":"v"}', b'"",{"host":"h"}'] if fmt == GELF else \
        [b'"', b'"' + HDR + b'[a b="c"] m', HDR + b'[a b="c"] m']
    i = 0
    for r in ((1, 3, 5, 7, 15, 17, 33, 63) if fmt == GELF else (1, 3, 5, 7, 9, 11, 13, 15)):  # (no run that makes a tile bail)
        for pad in range(16):
            ln = HEAD[fmt] + b"x" * pad + b"\\" * r
            out.append(Hz(ln, "odd-end", r, len(ln), "eol"))
            out.append(Hz(nxt[i % len(nxt)], "odd-end"))
            out.append(Hz(everyday(fmt, MIN_EVERYDAY[fmt] + i % 7, i), "odd-end"))
            i += 1
    return out


OVERSIZED = 66000  # longer than any tile: never staged with the lines before it, which makes the line before it its tile's last


def round_up(fmt: str, framing: int) -> List[Hz]:
    """hazard line (ends e = 0 .. 15 bytes before a 16-byte boundary), then a line longer than any tile, which starts with quotes and
    backslashes: the hazard line is the last of its tile and the span's round-up stages the first bytes of the long line"""
    tl, t = TAILS[fmt], len(term_of(framing))
    out: List[Hz] = []
    i = 0
    for r in (1, 2):
        for e in range(16):
            tail = tl[i % len(tl)]
            q = len(HEAD[fmt]) + r + 5 + i % 11
            n = q + 1 + len(tail.make()) + 3
            out.append(hazard(fmt, "round-up", q, r, tail, n, at=((-e - n - t) % 16, 16), want=e))
            if fmt == GELF:
                big = (b'"\\"\\\\",{"host":"h","x":"' if i % 2 else b'{"host":"h","x":"\\"') + b"y" * OVERSIZED + b'"}'
            else:
                big = (b'"\\"' if i % 2 else b"") + HDR + b'[a b="\\"' + b"y" * OVERSIZED + b'"] m'
            out.append(Hz(big, "round-up"))
            i += 1
    return out


def toggle(fmt: str, framing: int) -> List[Hz]:
    """an odd-quote line whose frame is s mod 64 bytes long, then a hazard line whose frame is -s mod 64: the hazard line starts at
    bit s of a word of the tile, s = 0, 1, 63"""
    tl, t = TAILS[fmt], len(term_of(framing))
    odd = [b'{"host":"h","s":"abc', b'x"y"z"', b'{"host":"h"}"'] if fmt == GELF else [HDR + b'[a b="c] m', HDR + b'[a b="c" d="] m']
    out: List[Hz] = []
    i = 0
    for s in (0, 1, 63):
        for r in ((1, 2, 3, 4, 8, 16, 32) if fmt == GELF else (1, 2, 3, 4, 6, 8, 14)):  # (no run that makes a tile bail)
            for tail in tl:
                o = odd[i % len(odd)]
                n_odd = up(len(o) + t - s, 64) + s - t
                out.append(Hz(o + b"x" * (n_odd - len(o)), "toggle", at=(0, 64)))
                q = len(HEAD[fmt]) + r + i % 13
                n = up(q + 1 + len(tail.make()) + t + s, 64) - s - t
                out.append(hazard(fmt, "toggle", q, r, tail, n, want=s))
                i += 1
    return out


def head_cap(framing: int) -> List[Hz]:
    """SD lines of 1300 bytes whose quote lies at offsets 1020 .. 1028 of the HEAD row (row = alignment slack o0 & 15, then the line's
    first bytes, 1024 in all): the run straddles the row's cut end; the structured data ends before the cut in some, behind it in others"""
    tl = TAILS[SD]
    out: List[Hz] = []
    i = 0
    for slack in (0, 1, 15):
        for row_off in range(1020, 1029):
            for r in (1, 2, 3, 4, 7, 8, 15):
                out.append(hazard(SD, "head-cap", row_off - slack, r, tl[i % len(tl)], 1300, at=(slack, 16), want=row_off))
                i += 1
    return out


# ---- the streams of the tests -----------------------------------------------------------------------------------------------------
_STREAMS: dict = {}


def streams(fmt: str, framing: int = NONE) -> List[Stream]:
    key = (fmt, framing)
    if key in _STREAMS:
        return _STREAMS[key]
    mk = lambda name, cls, hz, bail=False: assemble(f"{fmt}-{name}", fmt, cls, framing, hz, bail)  # noqa: E731
    out = [mk("fine", "fine", fine(fmt, framing, short_runs(fmt), reps=2 if fmt == GELF else 1)),
           mk("fine-bail", "fine", fine(fmt, framing, long_runs(fmt), every=4), True),
           mk("coarse", "coarse", coarse(fmt, framing)),
           mk("odd-end", "odd-end", odd_end(fmt)),
           mk("round-up", "round-up", round_up(fmt, framing)),
           mk("toggle", "toggle", toggle(fmt, framing))]
    if fmt == GELF:
        out.append(mk("member", "member", member()))
    else:
        out.append(mk("head-cap", "head-cap", head_cap(framing)))
    for s in out:
        check_invariants(s)
    _STREAMS[key] = out
    return out


def check_invariants(s: Stream) -> None:
    t = term_of(s.framing)
    assert len(s.offsets) == len(s.hz) + 1 and s.offsets[-1] == len(s.raw) < (4 << 20)
    for i, h in enumerate(s.hz):
        a, b = s.offsets[i], s.offsets[i + 1]
        assert s.raw[a:b] == h.line + t
        assert t == b"" or t not in h.line
        if h.run and h.q >= 0 and h.cls != "member" and h.tail != "eol":
            assert s.raw[a + h.q:a + h.q + 1] == b'"' and s.raw[a + h.q - h.run:a + h.q] == b"\\" * h.run
            assert s.raw[a + h.q - h.run - 1:a + h.q - h.run] != b"\\"
        if s.cls == "fine":
            assert (b - a) % WORD[s.fmt] == 0 and (not h.run or (a + h.q) % WORD[s.fmt] == h.want)
        elif s.cls == "coarse":
            assert b - a == COARSE_LINE[s.fmt] and a % COARSE_LINE[s.fmt] == 0 and h.q == h.want
        elif s.cls == "toggle":
            assert b % 64 == 0 if h.run else a % 64 == 0
            assert not h.run or (a % 64 == h.want and s.hz[i - 1].line.count(b'"') % 2 == 1)
        elif s.cls == "round-up" and h.run:
            assert (-b) % 16 == h.want and len(s.hz[i + 1].line) > OVERSIZED
        elif s.cls == "head-cap" and h.run:
            assert (a & 15) + h.q == h.want and len(h.line) > HEAD_CAP
        elif s.cls == "member":
            assert h.line[MEMBER_ITEM + h.want:MEMBER_ITEM + h.want + 1] == b'"'


def plan(framing: int = NONE) -> Counter:
    """hazard lines per (format, class) -- and per (format, class, 'bail') for the streams of long runs"""
    c: Counter = Counter()
    for fmt in (GELF, SD):
        for s in streams(fmt, framing):
            n = sum(1 for h in s.hz if h.run)
            c[(fmt, s.cls, "bail") if s.bail else (fmt, s.cls)] += n
    return c


def coverage(s: Stream) -> set:
    """what the stream's hazards cover: (run, wanted residue / offset) pairs"""
    return {(h.run, h.want) for h in s.hz if h.run}


# ---- byte-wise models of the two escape functions -----------------------------------------------------------------------------------
def escaped_model(bs: int, cin: int, width: int) -> Tuple[int, int]:
    """-> (mask of the characters escaped by a backslash, carry out): bit i of bs = byte i is a backslash; walked byte by byte"""
    esc, out = cin & 1, 0
    for i in range(width):
        if esc:
            out |= 1 << i
            esc = 0
        elif (bs >> i) & 1:
            esc = 1
    return out, esc
