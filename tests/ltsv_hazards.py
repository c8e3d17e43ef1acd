"""Lines that aim a byte at every boundary of the LTSV kernel (flowgger_amd/csrc/fg_ltsv.hip: LtsvFormatT::walk_tile, tab_behind_head,
decode): the 64-bit register window of the TAB bitmap (next_tab), the 16-byte window in which a part's first ':' and its key are
looked for, the key and suffix compares, the 16-byte records written over a line's own consumed bytes, the register windows that read
past a value's end, the end of the staged head of a long line and the 1 KiB rows scanned behind it.  Pure Python, no GPU (test
infrastructure); what tests/escape_hazards.py is for the escape carries.

Every line is put together part by part by `B`, which derives the Record (or the error) the reference must give FROM THE PARTS, not
from the bytes: the expectation is by construction (tests/test_ltsv_hazards_cpu.py pins the oracle to it).  Every aimed line carries
its intent -- class, aim, the line offset `pos` it aims at and `want`, the value that offset must have -- and check_invariants
recomputes each from the packed offsets:

  ("line", v)         pos == v, an offset in the line (a TAB, or the byte behind one: the start of a search)
  ("run", n)          n TABs in a row start at pos, none before, none behind
  ("part", c)         the part's first ':' at pos, c bytes behind the part's start
  ("next", n, g)      pos = the first ':' behind a colon-less part of n bytes, g bytes behind the part's end: the next part's or
                      the next LINE's
  ("abs", r, m)       (line start + pos) % m == r
  ("rec", o, m, d, w) line start & 3 == o; pair m's record ends d bytes behind its limit (d <= 0: it fits), every pair before it
                      fits; w = "part": the limit is the next part's first byte, "end": the line's end, a good line follows
  ("follows", nxt)    the line ends at pos and the bytes `nxt` follow it (behind the terminator, if any); "" = the batch ends
  ("head", d)         the head's end (HEAD - (line start & 15), the first byte that is NOT staged) lies d bytes behind pos
  ("rest", r)         pos = the head's end + r
  ("end", j)          pos = the line's end - j
  ("total", v)        len(line) + (line start & 15) == v

Every stream comes bare (lines packed back to back), "\\n"-framed and "\\0"-framed.  The classes whose point is adjacency -- `records`
(limit = the line's end), `value-end`, `colon` (bare-then-line) -- have the neighbour's bytes right behind the line when bare: that is
the hazard proper.  Framed, the terminator stands between the two (the invariants above count it in): the same lines then show that
a window which reads past the line's end does not take the terminator, or what follows it, for part of the value.

Absolute residues mod 16 are tile residues under every grouping: a tile starts at offsets[first line of the group] & ~15, a head row
at a multiple of 16 of the tile, a fused tile at T * S - 16 with S a multiple of 16 (fg_pipeline.hpp, fg_fused.hpp).  A filler line
in front fixes a line's start residue where `at` asks for it."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

from flowgger_amd.record import Record, SDValue, StructuredData

NONE, LINE, NUL = 0, 1, 2  # (= FG_FRAME_NONE / _LINE / _NUL): bare lines, or a stream with "\n" / "\0" behind every line

# ---- the kernel's geometry (test_ltsv_hazards_cpu.py compares these with the sources) ---------------------------------------------
HEAD = 512           # LtsvFormatT::kHeadBytes: bytes of a long line that are staged, alignment slack (line start & 15) included
CHUNK = 16           # the window of a part's name, its ':' and its key; a tile's alignment
TAB_WINDOW = 64      # bits of the TAB bitmap next_tab keeps in registers
ROW = 1024           # tab_behind_head: bytes per row behind the head
RECORD = 16          # bytes of a pair's in-tile record ...
RECORD_ALIGN = 4     # ... the first of which starts at the line's first multiple of this
NAME_LIMIT = 65536   # records keep 16-bit name offsets: decode's name_fits

TAB = b"\t"
KEYS = (b"time", b"host", b"level", b"message")
TYPES = ("string", "bool", "f64", "i64", "u64")
E_LEVEL, E_LEVEL7 = "Invalid severity level", "Severity level should be <= 7"
E_BOOL, E_F64, E_I64, E_U64 = ("Type error; boolean was expected", "Type error; f64 was expected", "Type error; i64 was expected",
                               "Type error; u64 was expected")
E_NOTS, E_NOHOST = "Missing timestamp", "Missing hostname"
E_TIME = "Unable to parse the English to Unix timestamp in LTSV decoder"

# ---- the configuration ------------------------------------------------------------------------------------------------------------
ALPHA = "abcdefghijklmnopqrst"
VAL = {"string": (b"v", "v"), "bool": (b"true", True), "f64": (b"2.5", 2.5), "i64": (b"-7", -7), "u64": (b"7", 7)}
KIND = {"string": "String", "bool": "Bool", "f64": "F64", "i64": "I64", "u64": "U64"}
SUFFIX = {"bool": "", "f64": "_", "i64": "_i64sfx", "u64": "_u64sufx"}   # lengths 0, 1, 7, 8
SUFFIX9 = dict(SUFFIX, u64="_u64suffx")                                  # ... and 9


def schema_name(t: str, n: int) -> str:
    """the schema's name of type t and length n, 1 .. 20"""
    return (t[0] + ALPHA)[:n]


def twin(k: int, c: str) -> str:
    """18-byte names that differ in byte k alone: c = 'A' is a u64, 'B' an i64, anything else is not in the schema"""
    return "q" * k + c + "q" * (17 - k)


def suffix_names(s: str) -> List[Tuple[str, str, bool]]:
    """(case, name, is the suffix appended?) for a configured suffix s"""
    if not s:
        return [("any", "b", False), ("any", "done", False)]
    out = [("equal", s, False), ("ends", "ab" + s, False), ("long-ends", "abcdefghijklmn" + s, False),
           ("all-but-last", "ab" + s[:-1], True), ("last-differs", "ab" + s[:-1] + "X", True)]
    if len(s) > 1:
        out.append(("shorter", s[1:], True))
    return out


def _schema() -> Dict[str, str]:
    s: Dict[str, str] = {}
    for k in (15, 16, 17):  # (first: the kernel mirrors the first 32 entries in LDS, the rest is matched from global memory)
        s[twin(k, "A")] = "u64"
        s[twin(k, "B")] = "i64"
    for n in (16, 17, 15, 18, 20, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 19):
        for t in TYPES:
            s[schema_name(t, n)] = t
    s.update({"counter": "u64", "score": "i64", "mean": "f64", "done": "bool", "zähler": "u64"})
    for sufs in (SUFFIX, SUFFIX9):
        for t in TYPES[1:]:
            for _, name, _ in suffix_names(sufs[t]):
                assert s.get(name, t) == t, name
                s[name] = t
    return s


SCHEMA = _schema()
SCHEMA_B = {k.encode(): v for k, v in SCHEMA.items()}
CONFIG = {"input": {"ltsv_schema": SCHEMA, "ltsv_suffixes": SUFFIX}}
CONFIG9 = {"input": {"ltsv_schema": SCHEMA, "ltsv_suffixes": SUFFIX9}}

# timestamps: the text and the value it has
TS = [(b"1", 1.0), (b"1.5", 1.5), (b"1438790025.5", 1438790025.5), (b"[2015-08-05T15:53:45Z]", 1438790025.0),
      (b"2015-08-05T15:53:45.5+00:00", 1438790025.5), (b"[10/Oct/2000:13:55:36 -0700]", 971211336.0)]

CLASSES = ("tab-window", "colon", "keys", "suffix", "records", "value-end", "head-end", "behind-head")


class Ln(NamedTuple):
    line: bytes
    cls: str
    exp: object             # the Record, or the error's text
    aim: str = ""           # what the line aims ("": a helper -- a filler, a neighbour)
    pos: int = -1
    want: tuple = ()
    at: Optional[Tuple[int, int]] = None  # (residue, modulus) the line's absolute start must have (a filler in front sees to it)


class Stream(NamedTuple):
    name: str
    cls: str
    framing: int
    config: dict
    ln: List[Ln]            # one per frame
    raw: bytes
    offsets: List[int]      # frame i = raw[offsets[i]:offsets[i + 1]], its terminator included

    def lines(self) -> List[bytes]:
        return [h.line for h in self.ln]


def term_of(framing: int) -> bytes:
    return b"" if framing == NONE else b"\n" if framing == LINE else b"\0"


def _s(b: bytes) -> str:
    return b.decode("utf-8", "surrogateescape")


class B:
    """a line, part by part, and what the reference makes of it (ltsv_decoder.rs:87-221)"""

    def __init__(self, suffixes: Dict[str, str] = SUFFIX):
        self.parts: List[bytes] = []
        self.suf = suffixes
        self.ts = self.hostname = self.message = self.sev = self.err = None
        self.pairs: List[Tuple[str, SDValue]] = []
        self.slot_at: Optional[int] = None
        self.slot_pair: Optional[int] = None
        self.last = 0  # line offset of the last part's first byte

    @property
    def n(self) -> int:
        return sum(len(p) for p in self.parts) + max(len(self.parts) - 1, 0)

    def _add(self, part: bytes) -> "B":
        assert b"\t" not in part and b"\n" not in part and b"\0" not in part
        self.last = self.n + (1 if self.parts else 0)
        self.parts.append(part)
        return self

    def time(self, text: bytes, ts: float) -> "B":
        if self.err is None:
            self.ts = ts
        return self._add(b"time:" + text)

    def host(self, v: bytes) -> "B":
        if self.err is None:
            self.hostname = _s(v)
        return self._add(b"host:" + v)

    def msg(self, v: bytes) -> "B":
        if self.err is None:
            self.message = _s(v)
        return self._add(b"message:" + v)

    def level(self, text: bytes, n: int) -> "B":
        assert 0 <= n <= 7
        if self.err is None:
            self.sev = n
        return self._add(b"level:" + text)

    def pair(self, name: bytes, t: str, text: bytes, value=None, appended: Optional[bool] = None) -> "B":
        assert name not in KEYS and b":" not in name and SCHEMA_B.get(name, "string") == t, name
        final = b"_" + name
        if t != "string" and t in self.suf and not name.endswith(self.suf[t].encode()):
            final += self.suf[t].encode()
            assert appended is not False
        else:
            assert appended is not True
        if self.err is None:
            self.pairs.append((_s(final), SDValue(KIND[t], _s(text) if t == "string" else value)))
        return self._add(name + b":" + text)

    def bare(self, text: bytes) -> "B":
        """a part without ':' ("Missing value for name ...": printed, no effect on the Record)"""
        assert b":" not in text
        return self._add(text)

    def fail(self, part: bytes, error: str) -> "B":
        """a part at which the reference gives up with `error`"""
        if self.err is None:
            self.err = error
        return self._add(part)

    def pad(self, k: int) -> "B":
        return self.pair(b"p", "string", b"x" * k)

    def slot(self) -> "B":
        """a part `p:xx..` whose length build() chooses (frame=)"""
        self.slot_pair = len(self.pairs) if self.err is None else None
        self.pair(b"p", "string", b"")
        self.slot_at = len(self.parts) - 1
        return self

    def fill(self, total: int, key: bytes = b"message") -> "B":
        """a last part `message:xx..` (or `p:xx..`) that makes the line `total` bytes long"""
        k = total - self.n - (1 if self.parts else 0) - len(key) - 1
        assert k >= 0, (total, self.n)
        return self.msg(b"x" * k) if key == b"message" else self.pad(k)

    def build(self, cls: str, aim: str = "", pos: int = -1, want: tuple = (), at=None, frame: Optional[Tuple[int, int, int]] = None) -> Ln:
        """frame = (r, m, t): the slot is stretched until len(line) + t == r mod m"""
        if frame is not None:
            r, m, t = frame
            k = (r - t - self.n) % m
            self.parts[self.slot_at] += b"x" * k
            if self.slot_pair is not None:
                self.pairs[self.slot_pair] = ("_p", SDValue("String", "x" * k))
        line = b"\t".join(self.parts)
        if self.err is not None:
            exp: object = self.err
        elif self.ts is None:
            exp = E_NOTS
        elif self.hostname is None:
            exp = E_NOHOST
        else:
            sd = [StructuredData(None, list(self.pairs))] if self.pairs else None
            exp = Record(ts=self.ts, hostname=self.hostname, severity=self.sev, msg=self.message, full_msg=_s(line), sd=sd)
        return Ln(line, cls, exp, aim, pos, want, at)


MIN_FILLER = 56  # (the longest timestamp of TS, a host and an empty message: 49 bytes)


def assemble(name: str, cls: str, framing: int, ln: List[Ln], config: dict = CONFIG) -> Stream:
    t = term_of(framing)
    out = bytearray()
    frames: List[Ln] = []
    offsets = [0]
    for i, h in enumerate(ln):
        if h.at is not None:
            res, m = h.at
            need = (res - len(out)) % m
            if need:
                while need < MIN_FILLER + len(t):
                    need += m
                f = B().time(*TS[i % len(TS)]).host(b"f").fill(need - len(t)).build(cls)
                out += f.line + t
                frames.append(f)
                offsets.append(len(out))
            assert len(out) % m == res
        out += h.line + t
        frames.append(h)
        offsets.append(len(out))
    return Stream(name, cls, framing, config, frames, bytes(out), offsets)


# ---- tab-window: next_tab's 64-bit window of the TAB bitmap ------------------------------------------------------------------------
def tab_index(t: int) -> List[Ln]:
    """the line's first TAB at every index 0 .. 200, for every start residue mod 16: every frame is 1 mod 16 bytes long, so sixteen
    lines in a row start at sixteen residues.  Searched from index 0, the TAB is bit i % 64 of the window after i // 64 refills."""
    out = []
    for i in range(201):
        for j in range(16):
            b = B()
            if i == 0:
                b.bare(b"")
            elif i == 1:
                b.bare(b"z")
            else:
                b.pair(b"z", "string", b"x" * (i - 2))
            b.time(*TS[j % len(TS)]).host(b"h%d" % j).slot()
            out.append(b.build("tab-window", "first-tab", i, ("line", i), frame=(1, 16, t)))
    return out


EMPTY_RUNS = (1, 2, 63, 64, 65)


def tab_parts(t: int) -> List[Ln]:
    out = []
    # a first part of 0 .. 130 bytes: the search for the SECOND TAB starts at offset p + 1 = 1 .. 131 of the first window
    for p in range(131):
        for j in range(4):
            b = B()
            if p == 0:
                b.bare(b"")
            elif p == 1:
                b.bare(b"z")
            else:
                b.pair(b"z", "string", b"x" * (p - 2))
            b.time(*TS[(p + j) % len(TS)]).host(b"h").pair(b"k", "string", b"v" * (j * 21)).slot()
            out.append(b.build("tab-window", "search-start", p + 1, ("line", p + 1), frame=(5, 16, t)))
    # runs of empty parts: n + 1 TABs between two parts, n in front of the first part, n behind the last
    for n in EMPTY_RUNS:
        for j in range(16):
            b = B().time(*TS[j % len(TS)]).host(b"h").slot()
            for _ in range(n):
                b.bare(b"")
            b.pair(b"k", "string", b"v")
            ln = b.build("tab-window", "empty-run", -1, ("run", n + 1), frame=(1, 16, t))
            out.append(ln._replace(pos=ln.line.index(b"\t\t")))
            b = B()
            for _ in range(n):
                b.bare(b"")
            b.time(*TS[j % len(TS)]).host(b"h").slot()
            out.append(b.build("tab-window", "empty-run", 0, ("run", n), frame=(1, 16, t)))
            b = B().time(*TS[j % len(TS)]).host(b"h").slot()
            for _ in range(n):
                b.bare(b"")
            ln = b.build("tab-window", "empty-run", -1, ("run", n), frame=(1, 16, t))
            out.append(ln._replace(pos=len(ln.line) - n))
    # a TAB as the first byte, as the last byte; no TAB at all (such a line cannot have both a time and a host)
    for j in range(16):
        out.append(B().bare(b"").time(*TS[j % len(TS)]).host(b"h").slot().build("tab-window", "tab-first", 0, ("line", 0), frame=(1, 16, t)))
    for j in range(16):
        ln = B().time(*TS[j % len(TS)]).host(b"h").slot().bare(b"").build("tab-window", "tab-last", -1, ("end", 1), frame=(1, 16, t))
        out.append(ln._replace(pos=len(ln.line) - 1))
    for j in range(16):
        out.append(B().host(b"h" * (j + 1)).build("tab-window", "no-tab", j + 6, ("end", 0)))
        out.append(B().time(*TS[j % len(TS)]).build("tab-window", "no-tab", len(TS[j % len(TS)][0]) + 5, ("end", 0)))
        out.append(B().bare(b"w" * (j + 1)).build("tab-window", "no-tab", j + 1, ("end", 0)))
    return out


# ---- colon: the part's first ':' in the 16-byte window, in_part, the byte-wise search from index 16 on ------------------------------
COLON_AT = tuple(range(18)) + (40,)
BARE_LEN = (1, 15, 16, 17, 40)
QUAD = (0, 5, 10, 15)  # start residues mod 16 that are all four residues mod 4


def colon(t: int) -> List[Ln]:
    out = []
    for c in COLON_AT:
        name = b"n" * c  # (c = 0: the empty name)
        for r in QUAD:
            b = B().pair(name, "string", b"v").time(*TS[c % len(TS)]).host(b"h")
            out.append(b.build("colon", "colon-first", c, ("part", c), at=(r, 16)))
            b = B().time(*TS[c % len(TS)]).host(b"h").pair(name, "string", b"v:w")
            ps = b.last
            out.append(b.pad(3).build("colon", "colon-middle", ps + c, ("part", c), at=(r, 16)))
            b = B().time(*TS[c % len(TS)]).host(b"h").pair(name, "string", b"")
            out.append(b.build("colon", "colon-last", b.last + c, ("part", c), at=(r, 16)))
    # a part without ':' whose neighbour's ':' is as near as can be: the next part is `:v` (the empty name), or the next LINE is
    for n in BARE_LEN:
        for r in QUAD:
            b = B().time(*TS[n % len(TS)]).host(b"h").bare(b"w" * n)
            ps = b.last
            out.append(b.pair(b"", "string", b"v").build("colon", "bare-then-part", ps + n + 1, ("next", n, 1), at=(r, 16)))
            if n < 12:  # ... and two bytes further on, still inside the bare part's window
                b = B().time(*TS[n % len(TS)]).host(b"h").bare(b"w" * n)
                out.append(b.pair(b"cd", "string", b"v").build("colon", "bare-then-part", ps + n + 3, ("next", n, 3), at=(r, 16)))
            b = B().time(*TS[n % len(TS)]).host(b"h").bare(b"w" * n)
            out.append(b.build("colon", "bare-then-line", b.last + n + t, ("next", n, t), at=(r, 16)))
            out.append(B().pair(b"", "string", b"v").time(b"2", 2.0).host(b"n").build("colon"))
    # the value holds colons
    for r in QUAD:
        b = B().pair(b"a", "string", b"b:c").time(b"[2015-08-05T15:53:45Z]", 1438790025.0).host(b"h:1:2").msg(b":a:b:").pair(b"", "string", b":")
        out.append(b.build("colon", "value-colons", 1, ("part", 1), at=(r, 16)))
    # the batch ends in a part without ':'
    b = B().time(b"1", 1.0).host(b"h").bare(b"w" * 15)
    out.append(b.build("colon", "bare-then-end", b.last + 15, ("end", 0)))
    return out


# ---- keys: the compares on k[0..3], the schema lookup ------------------------------------------------------------------------------
def near_misses(key: bytes) -> List[bytes]:
    return [key[:-1], key + b"s", key.upper(), key.capitalize(), key + b"x" * (16 - len(key)), key + b"x" * (17 - len(key))]


def keys(t: int) -> List[Ln]:
    """every frame is a multiple of 4 bytes: a part's offset in its line mod 4 is its absolute one"""
    out = []
    fr = (0, 4, t)
    for key in KEYS:
        for k in range(4):
            b = B().pad(k).host(b"h0").time(b"1", 1.0)
            if key == b"time":
                b.time(b"1.5", 1.5)
            elif key == b"host":
                b.host(b"h1")
            elif key == b"level":
                b.level(b"5", 5)
            else:
                b.msg(b"m m")
            ps = b.last
            out.append(b.slot().build("keys", "key " + key.decode(), ps, ("abs", ps % 4, 4), frame=fr))
            for miss in near_misses(key):
                b = B().pad(k).host(b"h0").time(b"1", 1.0).level(b"1", 1).msg(b"m").pair(miss, "string", b"9")
                ps = b.last
                out.append(b.slot().build("keys", "near " + key.decode(), ps, ("abs", ps % 4, 4), frame=fr))
    for ty in TYPES:
        for n in range(1, 21):
            for k in range(4):
                b = B().pad(k).time(*TS[n % len(TS)]).host(b"h").pair(schema_name(ty, n).encode(), ty, *VAL[ty])
                ps = b.last
                out.append(b.slot().build("keys", f"schema {ty} {n}", ps, ("abs", ps % 4, 4), frame=fr))
    for ty in TYPES:  # one byte longer than the schema's longest name of the type: not in the schema
        for k in range(4):
            b = B().pad(k).time(b"1", 1.0).host(b"h").pair(schema_name(ty, 20).encode() + b"x", "string", b"7")
            ps = b.last
            out.append(b.slot().build("keys", "schema long", ps, ("abs", ps % 4, 4), frame=fr))
    for at in (15, 16, 17):
        for k in range(4):
            b = B().pad(k).time(b"1", 1.0).host(b"h").pair(twin(at, "A").encode(), "u64", b"12", 12).pair(twin(at, "B").encode(), "i64", b"-12", -12)
            b.pair(twin(at, "C").encode(), "string", b"12")
            out.append(b.slot().build("keys", f"twins {at}", 4 + k, ("abs", k % 4, 4), frame=fr))
    for k in range(4):  # multi-byte UTF-8 in names and values: offsets count bytes
        b = B().pad(k).time(b"1", 1.0).host("hé".encode()).pair("näme".encode(), "string", "wért €".encode())
        b.pair("zähler".encode(), "u64", b"42", 42).msg("日本語 \U0001F600 x".encode()).pair(b"counter", "u64", b"3", 3)
        ps = b.last
        out.append(b.slot().build("keys", "utf-8", ps, ("abs", ps % 4, 4), frame=fr))
    return out


# ---- suffix: load8 of the name's tail, the byte-wise compare from nine bytes on ------------------------------------------------------
def suffix(t: int, sufs: Dict[str, str]) -> List[Ln]:
    out = []
    for ty in TYPES[1:]:
        s = sufs[ty]
        for case, name, appended in suffix_names(s):
            for k in range(4):
                b = B(sufs).pad(k).time(b"1", 1.0).host(b"h").pair(name.encode(), ty, *VAL[ty], appended=appended)
                pos = b.last + max(len(name) - len(s), 0)  # where the compare starts
                out.append(b.slot().build("suffix", f"{len(s)} {case}", pos, ("abs", pos % 4, 4), frame=(0, 4, t)))
    return out


# ---- records: wpos + 16 <= base + (more ? nps : len) --------------------------------------------------------------------------------
REC_M = (0, 1, 2, 5)
PAIR_COUNTS = (1, 3, 4, 5, 8, 9, 64, 300)


def record_fit(line: bytes, a: int, strict: bool = False) -> List[int]:
    """for the pairs of a line that starts at absolute offset a, in order, up to the first whose record does not fit: how far
    its record's end lies behind its limit (d = wpos + 16 - limit, it fits when d <= 0; strict: when d < 0)"""
    w = (-a) % RECORD_ALIGN
    parts = line.split(TAB)
    ps, out = 0, []
    for i, p in enumerate(parts):
        limit = ps + len(p) + 1 if i + 1 < len(parts) else len(line)
        if b":" in p and p.split(b":", 1)[0] not in KEYS:
            d = w + RECORD - limit
            out.append(d)
            if d > 0 or (strict and d == 0):
                break
            w += RECORD
        ps += len(p) + 1
    return out


def first_unfit(line: bytes, a: int, strict: bool = False) -> Optional[int]:
    """the first pair whose record does not fit (from it on the line's pairs come from the second walk); None: all fit"""
    ds = record_fit(line, a, strict)
    return len(ds) - 1 if ds and (ds[-1] > 0 or (strict and ds[-1] == 0)) else None


def tiny(b: B, j: int, v: int = 1) -> B:
    return b.pair(bytes([65 + j % 26]), "string", (b"%d" % (j % 10)) * v)


def records(t: int) -> List[Ln]:
    out = []
    for o in range(4):
        w0 = (-o) % RECORD_ALIGN
        for m in REC_M:
            for d in (-1, 0, 1):
                # the limit is the next part's first byte: a lead of L0 bytes, then parts of four bytes `a:1\t`
                L0 = w0 + 12 * (m + 1) - d
                b = B().host(b"x" * (L0 - 6))
                for j in range(m + 1):
                    tiny(b, j)
                limit = b.n + 1
                for j in range(m + 1, m + 3):
                    tiny(b, j)
                out.append(b.time(b"1", 1.0).build("records", "flip", limit, ("rec", o, m, d, "part"), at=(o, 4)))
                # the limit is the line's end: the last pair is `a:` + v bytes, a good line follows
                kv = w0 + 12 * m + 1 - d
                v = 1 if kv >= 1 else 0
                b = B().time(b"1", 1.0).host(b"x" * (kv - v))
                for j in range(m):
                    tiny(b, j)
                tiny(b, m, v)
                out.append(b.build("records", "flip", b.n, ("rec", o, m, d, "end"), at=(o, 4)))
                out.append(B().host(b"next").time(b"2", 2.0).pair(b"k", "string", b"v").build("records"))
    # the copy-out, four records at a time: roomy parts (every record fits) and tiny ones (none but the first few do)
    for n in PAIR_COUNTS:
        for o in range(4):
            for roomy in (True, False):
                b = B().time(*TS[n % len(TS)]).host(b"h")
                for j in range(n):
                    if j % 3 == 2:
                        b.pair(b"counter", "u64", b"%d" % (j * (1234567 if roomy else 1)), j * (1234567 if roomy else 1))
                    elif roomy:
                        b.pair(b"k%03d" % j, "string", b"v" * (12 + j % 5))
                    else:
                        tiny(b, j)
                out.append(b.build("records", f"count {n} " + ("roomy" if roomy else "tiny"), b.n, ("end", 0), at=(o, 4)))
    return out


# ---- value-end: load24, fast_ts's 40 bytes, load8 read past the value ---------------------------------------------------------------
def value_end_cases():
    """(name, the line's last part applied to a builder, what the next line starts with to extend it)"""
    return [
        ("u64", lambda b: b.pair(b"counter", "u64", b"12", 12), b"345"),
        ("i64", lambda b: b.pair(b"score", "i64", b"-7", -7), b"89"),
        ("f64", lambda b: b.pair(b"mean", "f64", b"1.5", 1.5), b"e9"),
        ("f64 dot", lambda b: b.pair(b"mean", "f64", b"1.", 1.0), b"25"),
        ("bool", lambda b: b.pair(b"done", "bool", b"true", True), b"x"),
        ("bool short", lambda b: b.fail(b"done:fals", E_BOOL), b"e"),
        ("u64 empty", lambda b: b.fail(b"counter:", E_U64), b"7"),
        ("time", lambda b: b.time(b"1.5", 1.5), b"e9"),
        ("time open", lambda b: b.fail(b"time:[1.5", E_TIME), b"]x"),
        ("time bracketed", lambda b: b.time(b"[1.5]", 1.5), b"]x"),
        ("time rfc3339", lambda b: b.time(b"2015-08-05T15:53:45Z", 1438790025.0), b"0"),
        ("time rfc3339 cut", lambda b: b.fail(b"time:2015-08-05T15:53:45", E_TIME), b"Z"),
        ("time english cut", lambda b: b.fail(b"time:[10/Oct/2000:13:55:36 -070", E_TIME), b"0]"),
        ("level", lambda b: b.level(b"3", 3), b"45"),
        ("level empty", lambda b: b.fail(b"level:", E_LEVEL), b"7"),
        ("level seven", lambda b: b.level(b"7", 7), b"0"),
        ("level eight", lambda b: b.fail(b"level:8", E_LEVEL7), b"0"),
        ("i64 sign", lambda b: b.fail(b"score:-", E_I64), b"7"),
        ("f64 exponent", lambda b: b.fail(b"mean:1e", E_F64), b"9"),
    ]


def value_end(t: int) -> List[Ln]:
    out = []
    last = None
    for name, part, nxt in value_end_cases():
        for i, r in enumerate(QUAD):
            b = B().host(b"h").time(b"1", 1.0).pad(i)
            part(b)
            h = b.build("value-end", name, b.n, ("follows", nxt), at=(r, 16))
            out.append(h)
            out.append(B().pair(nxt, "string", b"v").time(b"2", 2.0).host(b"n").build("value-end"))
            if name in ("u64", "time", "level"):
                last = h
    out.append(last._replace(want=("follows", b""), at=None))  # the same hazard as the batch's last line
    return out


# ---- head-end: where the staged head of a long line ends ----------------------------------------------------------------------------
def head_objects():
    """(name, bytes of the part in front of the object, the object's length, the part applied to a builder)"""
    return [
        ("typed", 8, 8, lambda b: b.pair(b"counter", "u64", b"12345678", 12345678)),
        ("time", 5, 12, lambda b: b.time(b"1438790025.5", 1438790025.5)),
        ("level", 6, 3, lambda b: b.level(b"007", 7)),
        ("name", 0, 9, lambda b: b.pair(b"nnnnnnnn", "string", b"v")),  # (the name and its ':')
        ("string", 2, 8, lambda b: b.pair(b"k", "string", b"vvvvvvvv")),
    ]


def head_end(t: int) -> List[Ln]:
    out = []
    for al in range(16):
        H = HEAD - al  # line index of the first byte that is not staged
        for name, lead, size, part in head_objects():
            for d in range(-1, size + 2):
                for more in (True, False):
                    s = H - d  # the object's first byte
                    b = B().host(b"h").time(b"1", 1.0)
                    b.fill(s - lead - 1, b"p")
                    part(b)
                    assert b.last + lead == s
                    if more:  # (a frame of a multiple of 16 bytes: the next line needs no filler)
                        b.fill(b.n + 300 + (-(b.n + 300 + t)) % 16)
                    out.append(b.build("head-end", name + (" +" if more else " last"), s, ("head", d), at=(al, 16)))
        for tab_at in (H - 1, H):  # the TAB as the last staged byte, as the first byte that is not staged
            b = B().host(b"h").time(b"1", 1.0).fill(tab_at, b"p").pair(b"counter", "u64", b"12", 12)
            b.fill(b.n + 300 + (-(b.n + 300 + t)) % 16)
            out.append(b.build("head-end", "tab", tab_at, ("head", H - tab_at), at=(al, 16)))
            b = B().host(b"h").time(b"1", 1.0).fill(tab_at, b"p").pair(b"k", "string", b"v")
            out.append(b.build("head-end", "tab", tab_at, ("head", H - tab_at), at=(al, 16)))
        for total in range(HEAD - 2, HEAD + 3):  # the whole-line / head boundary: len + (o0 & 15)
            n = total - al
            out.append(B().time(b"1", 1.0).host(b"h").fill(n).build("head-end", "boundary", n, ("total", total), at=(al, 16)))
            b = B().time(b"1", 1.0).host(b"h").fill(n - 11, b"p").pair(b"counter", "u64", b"12", 12)
            out.append(b.build("head-end", "boundary", n, ("total", total), at=(al, 16)))
    return out


# ---- behind-head: tab_behind_head's rows ---------------------------------------------------------------------------------------------
REST_AT = (0, 1, 15, 16, ROW - 1, ROW, ROW + 1, 2 * ROW - 1, 2 * ROW)
BIG = (NAME_LIMIT - 1, NAME_LIMIT, NAME_LIMIT + 1)


def behind_head(t: int) -> List[Ln]:
    out = []
    for al in (0, 1, 15):
        H = HEAD - al
        for r in REST_AT:  # the line's only TAB behind the head at rest offset r; the line ends five bytes on, or 1500
            for tail in (b"vv", b"v" * 1500):
                b = B().time(b"1", 1.0).host(b"h").fill(H + r).pair(b"k", "string", tail)
                out.append(b.build("behind-head", "rest-tab", H + r, ("rest", r), at=(al, 16)))
    for al in (0, 1):
        for lm in range(4):  # a TAB among the last four bytes, for every length mod 4
            for j in range(4):
                n = 1200 + lm
                b = B().time(b"1", 1.0).host(b"h").fill(n - 1 - j)
                if j == 0:
                    b.bare(b"")
                elif j == 1:
                    b.bare(b"z")
                else:
                    b.pair(b"k", "string", b"v" * (j - 2))
                assert b.n == n
                out.append(b.build("behind-head", "last-four", n - 1 - j, ("end", j + 1), at=(al, 16)))
    for i in range(8):  # no TAB behind the head; the next line starts with one, which must not count
        b = B().time(b"1", 1.0).host(b"h").fill(700 + 131 * i + i)
        out.append(b.build("behind-head", "tab-behind-end", b.n + t, ("line", b.n + t)))
        out.append(B().bare(b"").time(b"2", 2.0).host(b"n").build("behind-head"))
    for i in range(96):  # most lanes own three to five rows: well over eight rows a group, several trips of the owner lookup
        n = 2600 + (i * 397) % 2500
        b = B().time(*TS[i % len(TS)]).host(b"h%d" % i)
        if i % 3 == 0:
            out.append(b.fill(n).build("behind-head", "rows", n, ("end", 0)))
        else:
            at = 560 + (i * 977) % (n - 600)
            b.fill(at).pair(b"counter", "u64", b"%d" % i, i).fill(n)
            out.append(b.build("behind-head", "rows", at, ("line", at)))
    for n in BIG:  # the 16-bit name offsets of the in-tile records: pairs in the head, the message last
        for al in (0, 5):
            b = B().time(b"1", 1.0).host(b"h").pair(b"counter", "u64", b"12", 12).pair(b"k", "string", b"v").fill(n)
            out.append(b.build("behind-head", "name-limit", n, ("end", 0), at=(al, 16)))
            b = B().time(b"1", 1.0).host(b"h").pair(b"counter", "u64", b"12", 12).pair(b"k", "string", b"v").fill(n - 4).pair(b"z", "string", b"1")
            out.append(b.build("behind-head", "name-limit", n - 4, ("end", 4), at=(al, 16)))
    return out


# ---- the streams of the tests -------------------------------------------------------------------------------------------------------
_STREAMS: dict = {}


def streams(framing: int = NONE) -> List[Stream]:
    if framing in _STREAMS:
        return _STREAMS[framing]
    t = len(term_of(framing))
    mk = lambda name, cls, ln, cfg=CONFIG: assemble(name, cls, framing, ln, cfg)  # noqa: E731
    out = [mk("tab-index", "tab-window", tab_index(t)), mk("tab-parts", "tab-window", tab_parts(t)), mk("colon", "colon", colon(t)),
           mk("keys", "keys", keys(t)), mk("suffix", "suffix", suffix(t, SUFFIX)), mk("suffix9", "suffix", suffix(t, SUFFIX9), CONFIG9),
           mk("records", "records", records(t)), mk("value-end", "value-end", value_end(t)), mk("head-end", "head-end", head_end(t)),
           mk("behind-head", "behind-head", behind_head(t))]
    for s in out:
        check_invariants(s)
    _STREAMS[framing] = out
    return out


def head_at(a: int) -> int:
    """line index of the first byte that is not staged, for a long line that starts at absolute offset a"""
    return HEAD - (a & (CHUNK - 1))


def check_invariants(s: Stream) -> None:
    t = term_of(s.framing)
    assert len(s.offsets) == len(s.ln) + 1 and s.offsets[-1] == len(s.raw) < (4 << 20) and len(s.ln) < 6000
    for i, h in enumerate(s.ln):
        a, e = s.offsets[i], s.offsets[i + 1] - len(t)
        line, p = h.line, h.pos
        assert s.raw[a:e] == line and s.raw[e:s.offsets[i + 1]] == t
        assert t == b"" or t not in line
        assert h.at is None or a % h.at[1] == h.at[0]
        if not h.aim:
            continue
        w = h.want
        if w[0] == "line":
            assert p == w[1]
            if h.aim in ("first-tab", "tab-first"):
                assert line.index(TAB) == p
            elif h.aim == "search-start":
                assert line.index(TAB) == p - 1 and TAB in line[p:]
            elif h.aim == "tab-behind-end":
                assert s.raw[a + p:a + p + 1] == TAB and TAB not in line[head_at(a):] and len(line) > head_at(a)
            elif h.aim == "rows":
                assert line[p:p + 1] == TAB and p >= head_at(a) and (len(line) - head_at(a)) > 2 * ROW
        elif w[0] == "run":
            n = w[1]
            assert line[p:p + n] == TAB * n and (p == 0 or line[p - 1:p] != TAB) and line[p + n:p + n + 1] != TAB
        elif w[0] == "part":
            ps = line.rfind(TAB, 0, p) + 1
            assert line[p:p + 1] == b":" and p - ps == w[1] and b":" not in line[ps:p]
        elif w[0] == "next":
            n, g = w[1], w[2]
            bare_end = p - g
            ps = bare_end - n
            assert line[ps:bare_end] == b"w" * n and (ps == 0 or line[ps - 1:ps] == TAB)
            assert s.raw[a + p:a + p + 1] == b":" and b":" not in s.raw[a + ps:a + p]
            if h.aim == "bare-then-line":
                assert bare_end == len(line) and a + p == s.offsets[i + 1]
            else:
                assert line[bare_end:bare_end + 1] == TAB
            # (p - ps < CHUNK: the neighbour's ':' lies inside the 16-byte window of the bare part, in_part alone masks it)
        elif w[0] == "abs":
            assert (a + p) % w[2] == w[1]
        elif w[0] == "rec":
            _, o, m, d, where = w
            ds = record_fit(line, a)
            assert a % RECORD_ALIGN == o and len(ds) > m and ds[m] == d and all(x <= 0 for x in ds[:m]), (h, ds)
            assert (len(ds) == m + 1) == (d > 0) or where == "end"
            if where == "end":
                assert p == len(line) and len(ds) == m + 1 and s.ln[i + 1].line.startswith(b"host:next")
            else:
                assert line[p - 1:p] == TAB and p < len(line)
        elif w[0] == "follows":
            assert p == len(line)
            if w[1]:
                assert s.raw[s.offsets[i + 1]:s.offsets[i + 1] + len(w[1]) + 1] == w[1] + b":"
            else:
                assert i + 1 == len(s.ln)
        elif w[0] == "head":
            assert head_at(a) - p == w[1]
            if h.aim == "tab":
                assert line[p:p + 1] == TAB
        elif w[0] == "rest":
            assert p - head_at(a) == w[1] and line[p:p + 1] == TAB and line[head_at(a):].count(TAB) == 1
        elif w[0] == "end":
            assert len(line) - p == w[1]
            if h.aim in ("tab-last", "last-four"):
                assert line[p:p + 1] == TAB
            if h.aim == "last-four":
                assert line[head_at(a):].count(TAB) == 1
            if h.aim == "no-tab":
                assert TAB not in line
            if h.aim.startswith("count ") and h.aim.endswith("roomy"):
                assert all(x <= 0 for x in record_fit(line, a))
        elif w[0] == "total":
            assert len(line) + (a & (CHUNK - 1)) == w[1] and p == len(line)
        else:
            raise AssertionError(w)


def ledger(framing: int = NONE) -> Dict[str, Tuple[int, int]]:
    """class -> (lines, aimed positions)"""
    out: Dict[str, Tuple[int, int]] = {c: (0, 0) for c in CLASSES}
    for s in streams(framing):
        n, k = out[s.cls]
        out[s.cls] = (n + len(s.ln), k + sum(1 for h in s.ln if h.aim))
    return out
