"""Deflate streams built by hand from RFC 1951 (test infrastructure): an LSB-first bit writer, canonical codes from a list of lengths,
the header of a dynamic block with every field under the caller's control, the zlib / gzip wrappers, and a seeded generator of valid
streams over random complete code sets.  Nothing here inflates: what a stream means is asked of Python's zlib (tests/udp_model.py)."""
from __future__ import annotations

import bisect
import functools
import struct
import zlib

CLEN_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# a complete code-length code that has every symbol: 13 * 2^-4 + 6 * 2^-5 = 1 (lengths fit the header's three bits)
DEFAULT_CLEN = (4,) * 13 + (5,) * 6
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0,) * 8 + (1,) * 4 + (2,) * 4 + (3,) * 4 + (4,) * 4 + (5,) * 4 + (0,)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577)
DIST_EXTRA = (0, 0, 0, 0) + tuple(k for k in range(1, 14) for _ in (0, 1))
_REV = tuple(int(format(b, "08b")[::-1], 2) for b in range(256))
ZLIB_MIN, GZIP_MIN = 8, 24  # the gate's minimum lengths (udp_model.gate)


class BitWriter:
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value: int, nbits: int):
        """`nbits` bits of `value`, least significant first (header fields, extra bits)"""
        assert 0 <= value < (1 << nbits) or nbits == 0
        self.acc |= value << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, nbits: int):
        """a Huffman code, most significant bit first"""
        self.put(_REV[code & 0xFF] << (nbits - 8) | _REV[code >> 8] >> (16 - nbits) if nbits > 8 else _REV[code] >> (8 - nbits), nbits)

    def align(self):
        if self.n:
            self.put(0, 8 - self.n)

    def raw(self, data: bytes):
        assert self.n == 0, "raw bytes start at a byte boundary"
        self.out += data

    def bits(self) -> int:
        return len(self.out) * 8 + self.n

    def bytes(self) -> bytes:
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lengths):
    """RFC 1951 3.2.2: [(code, length) or None for a symbol without a code].  An oversubscribed set gets codes too (cut to their
    length): such a header is written to be refused, nobody decodes with it."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lengths:
        if l == 0:
            out.append(None)
        else:
            out.append((nxt[l] & ((1 << l) - 1), l))
            nxt[l] += 1
    return out


def kraft_left(lengths) -> int:
    """what is left of the code space, in units of 2^-15: < 0 oversubscribed, 0 complete, > 0 incomplete"""
    return (1 << 15) - sum(1 << (15 - l) for l in lengths if l)


class Codes:
    """the two codes of a block, and the symbols written with them"""

    def __init__(self, litlen_lengths, dist_lengths):
        self.lit, self.dst = canonical(litlen_lengths), canonical(dist_lengths)

    def sym(self, w: BitWriter, s: int):
        w.code(*self.lit[s])

    def dsym(self, w: BitWriter, s: int):
        w.code(*self.dst[s])

    def lits(self, w: BitWriter, data: bytes):
        for b in data:
            self.sym(w, b)

    def eob(self, w: BitWriter):
        self.sym(w, 256)

    def length(self, w: BitWriter, n: int, long284: bool = False):
        """the length symbol and its extra bits; long284: 258 as symbol 284 with extra 31 instead of symbol 285"""
        if n == 258 and long284:
            self.sym(w, 284)
            w.put(31, 5)
            return
        k = len_symbol(n) - 257
        assert n - LEN_BASE[k] < (1 << LEN_EXTRA[k])
        self.sym(w, 257 + k)
        w.put(n - LEN_BASE[k], LEN_EXTRA[k])

    def distance(self, w: BitWriter, d: int):
        k = dist_symbol(d)
        assert d - DIST_BASE[k] < (1 << DIST_EXTRA[k])
        self.dsym(w, k)
        w.put(d - DIST_BASE[k], DIST_EXTRA[k])

    def match(self, w: BitWriter, n: int, d: int, long284: bool = False):
        self.length(w, n, long284)
        self.distance(w, d)

    def run(self, w: BitWriter, n: int, byte: int = 0x61):
        """n >= 1 times `byte` with the fewest symbols: one literal, then matches at distance 1"""
        self.sym(w, byte)
        n -= 1
        while n:
            k = min(n, 258)
            if n - k in (1, 2):  # (no match is shorter than 3)
                k -= 3
            if k < 3:
                self.sym(w, byte)
                k = 1
            else:
                self.match(w, k, 1)
            n -= k


def len_symbol(n: int) -> int:
    return 285 if n == 258 else 256 + bisect.bisect_right(LEN_BASE, n, 0, 28)


def dist_symbol(d: int) -> int:
    return bisect.bisect_right(DIST_BASE, d) - 1


@functools.lru_cache(maxsize=None)
def fixed_codes() -> Codes:
    """RFC 1951 3.2.6, with the codes of the symbols that must not occur (286, 287; distance 30, 31)"""
    return Codes([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32)


def block_header(w: BitWriter, last: int, btype: int):
    w.put(last, 1)
    w.put(btype, 2)


def stored_block(w: BitWriter, last: int, data: bytes, *, length=None, nlength=None):
    block_header(w, last, 0)
    w.align()
    length = len(data) if length is None else length
    w.raw(struct.pack("<HH", length, (length ^ 0xFFFF) if nlength is None else nlength) + data)


def dynamic_header(w: BitWriter, last: int, litlen_lengths, dist_lengths, *, clen_lengths=DEFAULT_CLEN, clen_symbols=None, hlit=None,
                   hdist=None) -> Codes:
    """The header of a dynamic block; returns the block's codes.  clen_lengths: the 19 lengths of the code-length code, by symbol.
    clen_symbols: what the code-length code spells, as (symbol,) or (repeat symbol, extra bits' value); None: every length as itself.
    hlit / hdist: the raw 5-bit fields, when they should not say what the two lists do."""
    block_header(w, last, 2)
    w.put(len(litlen_lengths) - 257 if hlit is None else hlit, 5)
    w.put(len(dist_lengths) - 1 if hdist is None else hdist, 5)
    ncode = max([4] + [k + 1 for k in range(19) if clen_lengths[CLEN_ORDER[k]]])
    w.put(ncode - 4, 4)
    for k in range(ncode):
        w.put(clen_lengths[CLEN_ORDER[k]], 3)
    cc = canonical(clen_lengths)
    if clen_symbols is None:
        clen_symbols = [(l,) for l in list(litlen_lengths) + list(dist_lengths)]
    for s in clen_symbols:
        w.code(*cc[s[0]])
        if s[0] >= 16:
            w.put(s[1], {16: 2, 17: 3, 18: 7}[s[0]])
    return Codes(litlen_lengths, dist_lengths)


def _pad(d: bytes, least: int) -> bytes:
    return d + bytes(max(0, least - len(d)))


def wrap_zlib(body: bytes, payload: bytes, *, check_delta: int = 0, trailer: bool = True) -> bytes:
    """78 9c, the body, Adler-32 of `payload`; zero bytes up to the gate's minimum, so that a short stream still reaches the inflater"""
    t = struct.pack(">I", (zlib.adler32(payload) + check_delta) & 0xFFFFFFFF) if trailer else b""
    return _pad(b"\x78\x9c" + body + t, ZLIB_MIN)


def wrap_gzip(body: bytes, payload: bytes, *, check_delta: int = 0, trailer: bool = True, **hdr) -> bytes:
    """an RFC 1952 member around the body (header fields as udp_model.gz_member takes them), padded as wrap_zlib pads"""
    import udp_model as um

    head = um.gz_header(**hdr)
    t = struct.pack("<II", (zlib.crc32(payload) + check_delta) & 0xFFFFFFFF, len(payload) & 0xFFFFFFFF) if trailer else b""
    return _pad(head + body + t, GZIP_MIN)


# ---- seeded random code sets ---------------------------------------------------------------------------------------------------------

def random_complete_lengths(rng, nsyms: int, maxlen: int):
    """the lengths of a complete code of nsyms >= 2 symbols, none longer than maxlen: the Kraft budget starts as one leaf and a random
    leaf that may still grow is split in two until there are nsyms; half the time the deepest one, so that long codes do occur"""
    assert 2 <= nsyms <= (1 << maxlen)
    leaves = [0]
    while len(leaves) < nsyms:
        open_ = [k for k, d in enumerate(leaves) if d < maxlen]
        # (splitting takes no room away: a leaf at depth d can become 2^(maxlen - d) leaves before and after)
        k = max(open_, key=lambda j: leaves[j]) if rng.random() < 0.5 else open_[int(rng.integers(len(open_)))]
        d = leaves.pop(k)
        leaves += [d + 1, d + 1]
    return leaves


def _assign(rng, symbols, nsyms_total: int, maxlen: int):
    lens = random_complete_lengths(rng, len(symbols), maxlen)
    order = rng.permutation(len(symbols))
    out = [0] * nsyms_total
    for s, k in zip(symbols, order):
        out[s] = lens[int(k)]
    return out


def _with_extras(rng, used, universe: int, least: int):
    """`used` plus a random handful of other symbols below `universe`, at least `least` in all"""
    s = set(used)
    want = max(least, len(s) + int(rng.integers(0, 12)))
    while len(s) < min(want, universe):
        s.add(int(rng.integers(universe)))
    return sorted(s)


def _tokens(rng, payload: bytes):
    """greedy: literals, and at random a back-reference to an earlier occurrence of the next three bytes: ('l', byte) / ('m', len, dist)"""
    seen, toks, i, n = {}, [], 0, len(payload)
    while i < n:
        cand = seen.get(payload[i:i + 3], ()) if i + 3 <= n else ()
        took = 1
        if cand and rng.random() < 0.8:
            j = cand[int(rng.integers(len(cand)))]
            if i - j <= 32768:
                m = 0
                while m < 258 and i + m < n and payload[j + m] == payload[i + m]:  # (j + m may run past i: an overlapping match)
                    m += 1
                took = int(rng.integers(3, m + 1))
                toks.append(("m", took, i - j))
        if took == 1:
            toks.append(("l", payload[i]))
        for k in range(i, i + took):
            if k + 3 <= n:
                seen.setdefault(payload[k:k + 3], []).append(k)
        i += took
    return toks


def _rle(rng, seq):
    """the lengths `seq` spelt with the code-length alphabet, repeat codes taken at random where they fit"""
    out, i = [], 0
    while i < len(seq):
        v, run = seq[i], 1
        while i + run < len(seq) and seq[i + run] == v:
            run += 1
        if v == 0 and run >= 3 and rng.random() < 0.8:
            k = int(rng.integers(3, min(run, 138) + 1))
            out.append((17, k - 3) if k <= 10 and rng.random() < 0.7 else (18, k - 11) if k >= 11 else (17, k - 3))
            i += k
        elif i > 0 and seq[i - 1] == v and run >= 3 and rng.random() < 0.8:
            k = int(rng.integers(3, min(run, 6) + 1))
            out.append((16, k - 3))
            i += k
        else:
            out.append((v,))
            i += 1
    return out


def _dynamic_block(rng, w: BitWriter, last: int, toks):
    lit_used = {256} | {t[1] for t in toks if t[0] == "l"} | {len_symbol(t[1]) for t in toks if t[0] == "m"}
    dist_used = {dist_symbol(t[2]) for t in toks if t[0] == "m"}
    lit_syms = _with_extras(rng, lit_used, 286, 2)
    lmax = int(rng.integers(max(1, (len(lit_syms) - 1).bit_length()), 16))
    nlen = max(257, max(lit_syms) + 1)
    lit = _assign(rng, lit_syms, int(rng.integers(nlen, 287)), lmax)
    if not dist_used and rng.random() < 0.5:
        dst = [0]  # no distance code at all
    elif len(dist_used) <= 1 and rng.random() < 0.5:
        dst = [0] * (max(dist_used | {int(rng.integers(30))}) + 1)
        dst[max(dist_used) if dist_used else len(dst) - 1] = 1  # one 1-bit code: the incomplete set that is allowed
    else:
        dist_syms = _with_extras(rng, dist_used, 30, 2)
        dmax = int(rng.integers(max(1, (len(dist_syms) - 1).bit_length()), 16))
        dst = _assign(rng, dist_syms, int(rng.integers(max(dist_syms) + 1, 31)), dmax)
    spelt = _rle(rng, lit + dst)
    clen_syms = _with_extras(rng, {s[0] for s in spelt}, 19, 2)
    clen = _assign(rng, clen_syms, 19, int(rng.integers(max(1, (len(clen_syms) - 1).bit_length()), 8)))
    c = dynamic_header(w, last, lit, dst, clen_lengths=clen, clen_symbols=spelt)
    _symbols(w, c, toks)


def _symbols(w: BitWriter, c: Codes, toks):
    for t in toks:
        if t[0] == "l":
            c.sym(w, t[1])
        else:
            c.match(w, t[1], t[2])
    c.eob(w)


def random_dynamic_stream(rng, payload: bytes) -> bytes:
    """a valid raw deflate stream for `payload`: literals and random back-references, cut into one to three blocks of random type,
    the dynamic ones over random complete code sets with codes of up to 15 bits"""
    toks = _tokens(rng, payload)
    nblocks = min(len(toks), int(rng.integers(1, 4))) or 1
    cuts = sorted(int(c) for c in rng.integers(0, len(toks) + 1, nblocks - 1))
    parts = [toks[a:b] for a, b in zip([0] + cuts, cuts + [len(toks)])]
    w, pos = BitWriter(), 0
    types = [int(rng.integers(3)) for _ in parts]
    if 2 not in types:
        types[int(rng.integers(len(types)))] = 2  # (at least one block of every stream is dynamic)
    for k, (part, btype) in enumerate(zip(parts, types)):
        last = int(k == len(parts) - 1)
        size = sum(1 if t[0] == "l" else t[1] for t in part)
        if btype == 0:
            stored_block(w, last, payload[pos:pos + size])
        elif btype == 1:
            block_header(w, last, 1)
            _symbols(w, fixed_codes(), part)
        else:
            _dynamic_block(rng, w, last, part)
        pos += size
    assert pos == len(payload)
    return w.bytes()
