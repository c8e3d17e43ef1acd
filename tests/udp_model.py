"""What the UDP input tests share (test infrastructure): the model of handle_record_maybe_compressed (src/flowgger/input/udp_input.rs:
100-143) with Python's zlib as the inflater, the case list, the mutation pool, and the ctypes binding of
tests/native/libinflate_host.so (flowgger_amd/csrc/fg_inflate.hpp compiled for the CPU)."""
from __future__ import annotations

import ctypes as C
import functools
import gzip
import json
import struct
import subprocess
import zlib
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent / "native"
ROOT = HERE.parent.parent
LIB = HERE / "libinflate_host.so"
SRC = [HERE / "inflate_host.cpp", ROOT / "flowgger_amd" / "csrc" / "fg_inflate.hpp", ROOT / "flowgger_amd" / "csrc" / "fg_utf8.hpp"]

RAW, ZLIB, GZIP, BAD_ZLIB, BAD_GZIP, BAD_UTF8, TOO_LARGE = range(7)
DEFAULT_MAX = 65_527 * 5
ERRORS = {BAD_ZLIB: "Corrupted compressed (zlib) record", BAD_GZIP: "Corrupted compressed (gzip) record", BAD_UTF8: "Invalid UTF-8 input"}
VECTORS = json.loads((HERE.parent / "golden" / "udp_reference_vectors.json").read_text())
REF_LINE = VECTORS["line"].encode()


def gate(d: bytes) -> int:
    if len(d) >= 8 and d[0] == 0x78 and d[1] in (0x01, 0x9C, 0xDA):
        return ZLIB
    if len(d) >= 24 and d[:3] == b"\x1f\x8b\x08":
        return GZIP
    return RAW


def _valid_utf8(b: bytes) -> bool:
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


def _slot_of_check_error(d: bytes, wbits: int) -> bytes:
    """the slot of a stream whose trailer alone disagrees with its bytes: they stay in place (the row is flagged).  Fed bytewise,
    zlib has returned every byte before it raises with the trailer byte that completes the failing word -- the CRC-32 / Adler-32
    ('incorrect data check') or the gzip ISIZE ('incorrect length check').  The count pass wants the WHOLE trailer before it gives a
    slot, so a gzip member whose CRC-32 is wrong AND whose ISIZE is cut short has none."""
    o = zlib.decompressobj(wbits=wbits)
    out = bytearray()
    for k in range(len(d)):
        try:
            out += o.decompress(d[k:k + 1])
        except zlib.error as e:
            if wbits == 31 and "incorrect data check" in str(e) and len(d) - (k + 1) < 4:
                return b""
            return bytes(out)
    raise AssertionError("the bytewise walk did not meet the error of the one-shot call")


def model(d: bytes, max_inflated: int = DEFAULT_MAX):
    """-> (fg_udp_status, the bytes of the datagram's slot, kept).  The gate, then zlib.decompressobj(wbits = 15 for the zlib
    gate, 31 for the gzip gate).decompress(d, max_inflated + 1); kept iff no exception, .eof and the length <= max_inflated (and,
    as for a bare record, valid UTF-8).  Anything but zlib.error propagates: the model never raises anything else."""
    kind = gate(d)
    if kind == RAW:
        return (RAW, d, True) if _valid_utf8(d) else (BAD_UTF8, d, False)
    wbits = 15 if kind == ZLIB else 31
    bad = BAD_ZLIB if kind == ZLIB else BAD_GZIP
    o = zlib.decompressobj(wbits=wbits)
    try:
        out = o.decompress(d, max_inflated + 1)
    except zlib.error as e:
        if "incorrect data check" in str(e) or "incorrect length check" in str(e):
            return bad, _slot_of_check_error(d, wbits), False
        return bad, b"", False
    if len(out) > max_inflated:
        # (a stream that ENDS one byte past the cap had its trailer checked: its bytes take a slot for that, dropped all the same)
        return TOO_LARGE, out if o.eof else b"", False
    if not o.eof:
        return bad, b"", False
    return (kind, out, True) if _valid_utf8(out) else (BAD_UTF8, out, False)


def gz_header(extra=None, name=None, comment=None, hcrc=False, bad_hcrc=False) -> bytes:
    """the header of an RFC 1952 member"""
    flg = (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | (2 if hcrc else 0)
    h = bytes([0x1F, 0x8B, 8, flg, 0, 0, 0, 0, 0, 255])
    if extra is not None:
        h += struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", ((zlib.crc32(h) & 0xFFFF) + (1 if bad_hcrc else 0)) & 0xFFFF)
    return h


def gz_member(payload: bytes, extra=None, name=None, comment=None, hcrc=False, level=6, bad_hcrc=False, crc_delta=0, isize_delta=0) -> bytes:
    """an RFC 1952 member built by hand around a raw deflate stream"""
    h = gz_header(extra, name, comment, hcrc, bad_hcrc)
    c = zlib.compressobj(level, zlib.DEFLATED, -15)
    body = c.compress(payload) + c.flush()
    return h + body + struct.pack("<II", (zlib.crc32(payload) + crc_delta) & 0xFFFFFFFF, (len(payload) + isize_delta) & 0xFFFFFFFF)


JSON_LINE = (b'{"version":"1.1","host":"web-17.example.org","short_message":"GET /api/v2/items?id=4211 200 17ms","timestamp":1438790025.42,'
             b'"level":6,"_user":"alice","_session":"c0ffee-7f3a","_bytes":18244,"_ua":"Mozilla/5.0 (X11; Linux x86_64) Gecko/20100101",'
             b'"_trace":"9b1c2d3e4f5a6b7c","_region":"eu-west-3","_note":"caf\xc3\xa9 \xe2\x9c\x93"}')


def case_list(max_inflated: int = DEFAULT_MAX):
    """[(name, datagram)]: the issue's list.  The two cases at the cap are built for `max_inflated`."""
    rng = np.random.default_rng(1950)
    out = []
    add = lambda name, d: out.append((name, bytes(d)))
    add("ref_raw", REF_LINE)
    add("ref_zlib", zlib.compress(REF_LINE))
    add("ref_gzip", gzip.compress(REF_LINE, mtime=0))
    add("ref_gzip_trunc5", gzip.compress(REF_LINE, mtime=0)[:VECTORS["bad_record_truncate"]])
    # block types
    add("stored", zlib.compress(JSON_LINE, 0))
    add("fixed", zlib.compress(b"short line", 6))
    assert len(JSON_LINE) >= 300
    add("dynamic", zlib.compress(JSON_LINE, 6))
    for mode, nm in ((zlib.Z_SYNC_FLUSH, "sync"), (zlib.Z_FULL_FLUSH, "full")):
        c = zlib.compressobj(6)
        add("flush_" + nm, c.compress(JSON_LINE) + c.flush(mode) + c.compress(REF_LINE) + c.flush(mode) + c.compress(JSON_LINE[:90]) + c.flush())
    big = bytes(rng.integers(0x20, 0x7F, 65_536, dtype=np.uint8))
    add("stored_two_blocks", zlib.compress(big, 0))
    # matches
    add("dist1_overlap", zlib.compress(b"a" * 5000, 9))
    half = bytes(rng.integers(0x20, 0x7F, 32_768, dtype=np.uint8))
    add("dist32768", zlib.compress(half + half, 9))
    add("match_at_cap", zlib.compress(b"xyz" + b"b" * (max_inflated - 3), 9))
    add("match_past_cap", zlib.compress(b"xyz" + b"b" * (max_inflated - 2), 9))
    add("match_at_cap_gz", gzip.compress(b"xyz" + b"b" * (max_inflated - 3), mtime=0))
    add("match_past_cap_gz", gzip.compress(b"xyz" + b"b" * (max_inflated - 2), mtime=0))
    # gates
    add("zlib_len7", zlib.compress(b"")[:7] if len(zlib.compress(b"")) >= 7 else b"\x78\x9c\x03\x00\x00\x00\x00")
    assert out[-1][1][:2] == b"\x78\x9c" and len(out[-1][1]) == 7
    add("gzip_len23", gz_member(b"abc")[:23])
    assert len(out[-1][1]) == 23
    z = bytearray(zlib.compress(JSON_LINE))
    z[1] = 0x5E
    add("second_byte_5e", z)
    add("empty", b"")
    add("raw_bad_utf8", b"abc\xff def")
    add("raw_cut_utf8", b"abc\xe2\x9c")
    add("zlib_bad_utf8", zlib.compress(b"inflates to \xc3\x28 invalid text"))
    add("gzip_cut_utf8", gzip.compress(b"ends inside \xe2\x9c", mtime=0))
    # gzip headers by hand
    add("gz_plain", gz_member(JSON_LINE))
    add("gz_fextra", gz_member(JSON_LINE, extra=b"\x41\x70\x04\x00abcd"))
    add("gz_fname", gz_member(JSON_LINE, name=b"line.json"))
    add("gz_fcomment", gz_member(JSON_LINE, comment=b"a comment"))
    add("gz_fhcrc", gz_member(JSON_LINE, hcrc=True))
    add("gz_all4", gz_member(JSON_LINE, extra=b"\x01\x02\x00\x00", name=b"n", comment=b"c", hcrc=True))
    add("gz_bad_fhcrc", gz_member(JSON_LINE, name=b"n", hcrc=True, bad_hcrc=True))
    add("gz_bad_crc32", gz_member(JSON_LINE, crc_delta=1))
    add("gz_bad_isize", gz_member(JSON_LINE, isize_delta=1))
    add("gz_bad_crc32_isize_cut", gz_member(JSON_LINE, crc_delta=1)[:-2])  # zlib reports the CRC-32; no slot without the whole trailer
    add("gz_isize_cut", gz_member(JSON_LINE)[:-1])
    add("gz_reserved_flag", bytes(b | (0x20 if k == 3 else 0) for k, b in enumerate(gz_member(JSON_LINE))))
    za = bytearray(zlib.compress(JSON_LINE))
    za[-1] ^= 0x01
    add("zlib_bad_adler", za)
    add("zlib_trailing", zlib.compress(JSON_LINE) + b"trailing bytes")
    add("gzip_trailing", gz_member(JSON_LINE) + gz_member(b"a second member"))
    return out


HAND_CAPS = (DEFAULT_MAX, 259, 258, 257, 3, 1)


def _hand_bodies(cap: int):
    """[(name, raw deflate body, the payload it stands for, verdict)]: 'ok' the stream is kept, 'bad' zlib refuses it, 'big' it wants
    more than `cap` bytes.  The names that begin with 'cap_' are built for `cap` and judged there, the others are judged at DEFAULT_MAX."""
    import deflate_build as db

    out = []
    fx = db.fixed_codes()

    def add(name, verdict, build, payload=b""):
        w = db.BitWriter()
        build(w)
        out.append((name, w.bytes(), payload, verdict))

    def tail(w, nbytes=8):  # bits behind a malformation: it is refused for what it is, not for the input's end
        w.put(0, 8 * nbytes)

    def fixed(last=1):
        def start(w):
            db.block_header(w, last, 1)
        return start

    lit2 = lambda a: [a.get(s, 0) for s in range(max(257, max(a) + 1))]  # lit/len lengths from {symbol: length}

    # -- the code-length code
    def clen_zero(nbytes):
        def f(w):
            db.dynamic_header(w, 1, [0] * 257, [0], clen_lengths=[0] * 19, clen_symbols=[])
            tail(w, nbytes)  # (258 one-bit dummies are wanted: 33 bytes)
        return f
    add("clen_all_zero", "bad", clen_zero(40))
    add("clen_all_zero_cut_in_dummies", "bad", clen_zero(5))
    cl = lambda a: [a.get(s, 0) for s in range(19)]
    add("clen_oversubscribed", "bad", lambda w: (db.dynamic_header(w, 1, [0] * 257, [0], clen_lengths=cl({16: 1, 17: 1, 18: 1, 0: 1}), clen_symbols=[]), tail(w)))
    add("clen_incomplete", "bad", lambda w: (db.dynamic_header(w, 1, [0] * 257, [0], clen_lengths=cl({0: 2, 8: 2}), clen_symbols=[]), tail(w)))
    add("clen_one_code", "bad", lambda w: (db.dynamic_header(w, 1, [0] * 257, [0], clen_lengths=cl({0: 1}), clen_symbols=[]), tail(w)))

    # -- the literal/length code
    add("lit_only_eob", "ok", lambda w: db.dynamic_header(w, 1, lit2({256: 1}), [0]).eob(w))
    add("lit_only_eob_then_code_1", "bad", lambda w: (db.dynamic_header(w, 0, lit2({256: 1}), [0]), w.put(1, 1), tail(w)))
    add("lit_oversubscribed", "bad", lambda w: (db.dynamic_header(w, 1, lit2({0x61: 1, 0x62: 1, 256: 1}), [0]), tail(w)))
    add("lit_incomplete_two_2bit", "bad", lambda w: (db.dynamic_header(w, 1, lit2({0x61: 2, 256: 2}), [0]), tail(w)))
    add("lit_no_eob", "bad", lambda w: (db.dynamic_header(w, 1, lit2({0x61: 1, 0x62: 1}), [0]), tail(w)))
    text45 = bytes(0x78 + (k * 7 % 3 == 0) for k in range(45))  # 'x' and 'y'

    def lit_15bit(w):
        a = {k: k + 1 for k in range(13)}  # lengths 1 .. 13 for symbols nobody writes, 14 for the end, 15 + 15 for the text
        a.update({256: 14, 0x78: 15, 0x79: 15})
        assert db.kraft_left(lit2(a)) == 0
        c = db.dynamic_header(w, 1, lit2(a), [0])
        c.lits(w, text45)
        c.eob(w)
    add("lit_15bit_codes", "ok", lit_15bit, text45)
    head32 = bytes(range(0x40, 0x60))

    def all_symbols(w):  # hlit = hdist = 29: the largest that are valid
        lit, dst = [8] * 226 + [9] * 60, [4] * 2 + [5] * 28
        assert db.kraft_left(lit) == 0 and db.kraft_left(dst) == 0
        c = db.dynamic_header(w, 1, lit, dst)
        c.lits(w, head32)
        c.match(w, 258, 32)
        c.eob(w)
    add("all_286_and_30_symbols_hlit29_hdist29", "ok", all_symbols, (head32 * 10)[:32 + 258])

    # -- the distance code
    abc = {0x61: 2, 0x62: 2, 256: 2, 257: 2}

    def with_dist(dst, bits, last_sym=257):
        def f(w):
            c = db.dynamic_header(w, 1, lit2(abc), dst)
            c.lits(w, b"ab")
            c.sym(w, last_sym)  # length 3
            for b in bits:
                w.put(b, 1)
            c.eob(w)
        return f
    add("dist_none_length_used", "bad", with_dist([0], []))
    add("dist_none_unused", "ok", with_dist([0], [], last_sym=0x62), b"abb")
    add("dist_one_code_bit_0", "ok", with_dist([1], [0]), b"abbbb")
    add("dist_one_code_bit_1", "bad", with_dist([1], [1]))
    add("dist_one_code_not_the_first", "ok", with_dist([0, 1], [0]), b"ababa")
    add("dist_two_1bit_codes", "ok", with_dist([1, 1], [1]), b"ababa")
    add("dist_incomplete_2bit", "bad", with_dist([2, 2], [0, 0]))
    add("dist_oversubscribed", "bad", with_dist([1, 1, 1], [0]))

    # -- repeat codes
    add("repeat_16_first", "bad", lambda w: (db.dynamic_header(w, 1, lit2(abc), [0], clen_symbols=[(16, 0)]), tail(w)))
    add("repeat_18_past_the_lengths", "bad", lambda w: (db.dynamic_header(w, 1, lit2(abc), [0], clen_symbols=[(18, 127), (18, 127)]), tail(w)))
    add("repeat_16_past_the_lengths", "bad",
        lambda w: (db.dynamic_header(w, 1, lit2(abc), [0], clen_symbols=[(18, 127), (18, 107), (2,), (16, 0)]), tail(w)))  # 256 + 3 > 258

    def rep_into_dist(w):  # 97 zeros, a = 1, b = 3, 157 zeros, end = 3, length 3 = 2, then 16 carries the 2 over all four distance lengths
        a = {0x61: 1, 0x62: 3, 256: 3, 257: 2}
        c = db.dynamic_header(w, 1, lit2(a), [2, 2, 2, 2], clen_symbols=[(18, 86), (1,), (3,), (18, 127), (18, 8), (3,), (2,), (16, 1)])
        c.lits(w, b"ab")
        c.match(w, 3, 2)
        c.eob(w)
    add("repeat_16_from_literal_into_distance_lengths", "ok", rep_into_dist, b"ababa")

    def rep_after_zero_runs(w):  # 16 directly after 17 and after 18 repeats their zero
        a = {0x61: 1, 0x62: 2, 256: 2}
        spelt = [(17, 7), (16, 3), (18, 70), (1,), (2,), (18, 127), (16, 3), (17, 7), (16, 0), (2,), (0,)]
        c = db.dynamic_header(w, 1, lit2(a), [0], clen_symbols=spelt)
        c.lits(w, b"abba")
        c.eob(w)
    add("repeat_16_after_17_and_18", "ok", rep_after_zero_runs, b"abba")

    # -- header fields, block type
    add("hlit_30", "bad", lambda w: (db.dynamic_header(w, 1, lit2(abc), [0], hlit=30), tail(w)))
    add("hlit_31", "bad", lambda w: (db.dynamic_header(w, 1, lit2(abc), [0], hlit=31), tail(w)))
    add("hdist_30", "bad", lambda w: (db.dynamic_header(w, 1, lit2(abc), [0], hdist=30), tail(w)))
    add("hdist_31", "bad", lambda w: (db.dynamic_header(w, 1, lit2(abc), [0], hdist=31), tail(w)))
    add("block_type_3", "bad", lambda w: (db.block_header(w, 1, 3), tail(w)))
    add("block_type_3_second", "bad", lambda w: (fixed(0)(w), fx.lits(w, b"ab"), fx.eob(w), db.block_header(w, 1, 3), tail(w)))

    # -- symbols of the fixed codes
    for s in (286, 287):
        add(f"fixed_symbol_{s}", "bad", lambda w, s=s: (fixed()(w), fx.lits(w, b"a"), fx.sym(w, s), tail(w)))
    for s in (30, 31):
        add(f"fixed_distance_{s}", "bad", lambda w, s=s: (fixed()(w), fx.lits(w, b"a"), fx.sym(w, 257), fx.dsym(w, s), tail(w)))
    add("length_258_as_285", "ok", lambda w: (fixed()(w), fx.lits(w, b"a"), fx.match(w, 258, 1), fx.eob(w)), b"a" * 259)
    add("length_258_as_284_extra_31", "ok", lambda w: (fixed()(w), fx.lits(w, b"a"), fx.match(w, 258, 1, long284=True), fx.eob(w)), b"a" * 259)

    # -- distances against the bytes produced so far (no distance is longer than 32 768: o + 1 cannot be said at o = 32 768)
    for o, dist, verdict in ((0, 1, "bad"), (1, 2, "bad"), (1, 1, "ok"), (32767, 32768, "bad"), (32767, 32767, "ok"), (32768, 32768, "ok")):
        def f(w, o=o, dist=dist):
            fixed()(w)
            if o:
                fx.run(w, o)
            fx.match(w, 3, dist)
            fx.eob(w)
        add(f"distance_{dist}_at_{o}", verdict, f, b"a" * (o + 3))

    # -- stored blocks
    line = b"a stored line"
    add("stored_empty_then_final", "ok", lambda w: (db.stored_block(w, 0, b""), db.stored_block(w, 1, line)), line)
    add("stored_len_not_nlen", "bad", lambda w: db.stored_block(w, 1, line, nlength=len(line) ^ 0xFFFE))
    add("stored_after_unaligned_fixed", "ok", lambda w: (fixed(0)(w), fx.lits(w, b"ab"), fx.eob(w), db.stored_block(w, 1, line)), b"ab" + line)
    add("stored_len_past_the_input", "bad", lambda w: db.stored_block(w, 1, line, length=100))

    # -- fixed, dynamic, fixed: the tables are rebuilt for the second fixed block, whose match reaches into the first one's bytes
    def three_blocks(w):
        fixed(0)(w)
        fx.lits(w, b"hello ")
        fx.eob(w)
        a = {s: 3 for s in b"world "}
        a.update({256: 3, 257: 3})  # w o r l d ' ' + end + length 3: eight 3-bit codes
        c = db.dynamic_header(w, 0, lit2(a), [1, 1])
        c.lits(w, b"world ")
        c.eob(w)
        fixed(1)(w)
        fx.match(w, 5, 12)
        fx.eob(w)
    add("fixed_dynamic_fixed", "ok", three_blocks, b"hello world hello")

    # -- the order of the verdicts at the cap: cap + 1 bytes (what zlib is given room for), then one more thing
    pre = cap + 1
    after = [("eob", "big", lambda w: None), ("literal", "big", lambda w: fx.lits(w, b"a")), ("match", "big", lambda w: fx.match(w, 3, 1)),
             ("distance_30", "bad", lambda w: (fx.sym(w, 257), fx.dsym(w, 30))), ("symbol_286", "bad", lambda w: fx.sym(w, 286))]
    if pre + 1 <= 32768:
        after.append(("match_too_far", "big", lambda w: fx.match(w, 3, pre + 1)))  # (room is asked for before the distance is looked at)
    for nm, verdict, more in after:
        add(f"cap_plus_1_then_{nm}", verdict, lambda w, more=more: (fixed()(w), fx.run(w, pre), more(w), fx.eob(w)),
            b"a" * pre if nm == "eob" else b"")
    return out


@functools.lru_cache(maxsize=None)
def hand_streams(max_inflated: int = DEFAULT_MAX):
    """[(name, datagram, expected status)]: deflate streams no compressor writes (tests/deflate_build.py), every body as a zlib stream
    and as a gzip member, and every valid one once more with its checksum off by one.  The expected status is the table's, not the
    model's: tests/test_inflate_cpu.py holds the two against each other, the 'cap_' cases at `max_inflated` (they are built for it),
    the others at DEFAULT_MAX."""
    import deflate_build as db

    out = []
    for name, body, payload, verdict in _hand_bodies(max_inflated):
        for wrap, tag, ok, bad in ((db.wrap_zlib, "z", ZLIB, BAD_ZLIB), (db.wrap_gzip, "g", GZIP, BAD_GZIP)):
            out.append((f"{name}_{tag}", wrap(body, payload), {"ok": ok, "bad": bad, "big": TOO_LARGE}[verdict]))
            if verdict == "ok":
                out.append((f"{name}_{tag}_check_off_by_one", wrap(body, payload, check_delta=1), bad))
    return out


@functools.lru_cache(maxsize=None)
def random_code_set_pool(n: int = 2000, seed: int = 1952):
    """-> (n valid streams over random code sets (tests/deflate_build.py) around the lines of corpus_lines(16), alternating wrappers;
    the same streams with one bit flipped in the first 40 bytes of the deflate body)"""
    import deflate_build as db

    rng = np.random.default_rng(seed)
    lines = corpus_lines(16)
    good, flipped = [], []
    for k in range(n):
        line = lines[k % len(lines)]
        body = db.random_dynamic_stream(rng, line)
        d = db.wrap_zlib(body, line) if k % 2 == 0 else db.wrap_gzip(body, line)
        good.append(d)
        head = 2 if k % 2 == 0 else 10
        f = bytearray(d)
        f[head + int(rng.integers(min(40, len(body))))] ^= 1 << int(rng.integers(8))
        flipped.append(bytes(f))
    return good, flipped


def truncations():
    z, g = zlib.compress(JSON_LINE), gz_member(JSON_LINE, name=b"n", hcrc=True)
    return [z[:k] for k in range(len(z) + 1)] + [g[:k] for k in range(len(g) + 1)]


def corpus_lines(n_each: int = 64):
    from flowgger_amd import synth
    lines = list(synth.gelf_lines(n_each)) + list(synth.ltsv_lines(n_each)) + list(synth.rfc3164_lines(n_each))
    lines += [l.encode() if isinstance(l, str) else l for l in synth.rfc5424_lines(n_each, sd=True)]
    return [bytes(l).rstrip(b"\n") for l in lines]


def mutation_pool(n: int = 20_000, seed: int = 1951):
    """n datagrams: compressed corpus lines (levels 0/1/6/9, both wrappers) with one to three byte flips, inserts or deletes"""
    rng = np.random.default_rng(seed)
    lines = corpus_lines()
    base = []
    for i, l in enumerate(lines):
        lvl = (0, 1, 6, 9)[i % 4]
        base.append(zlib.compress(l, lvl))
        base.append(gz_member(l, level=lvl, name=b"x" if i % 8 == 0 else None, hcrc=i % 16 == 0))
    out = []
    for k in range(n):
        d = bytearray(base[int(rng.integers(len(base)))])
        for _ in range(int(rng.integers(1, 4))):
            op, at = int(rng.integers(3)), int(rng.integers(len(d)))
            if op == 0:
                d[at] ^= 1 << int(rng.integers(8))
            elif op == 1:
                d.insert(at, int(rng.integers(256)))
            elif len(d) > 1:
                del d[at]
        out.append(bytes(d))
    return out


def pack(datagrams):
    offs = np.zeros(len(datagrams) + 1, np.uint64)
    offs[1:] = np.cumsum([len(d) for d in datagrams], dtype=np.uint64)
    blob = np.frombuffer(b"".join(datagrams), np.uint8)
    return blob, offs


def expect(datagrams, max_inflated: int = DEFAULT_MAX):
    """the model over a batch -> (status[n], kept[n], the bytes of every datagram's slot)"""
    res = [model(d, max_inflated) for d in datagrams]
    return np.array([r[0] for r in res], np.uint8), np.array([r[2] for r in res], bool), [r[1] for r in res]


def check_batch(datagrams, max_inflated, offsets, packed, drop, status, what=""):
    """offsets / packed bytes / drop / status of an unpacked batch against the model, exactly"""
    st, kept, slots = expect(datagrams, max_inflated)
    n = len(datagrams)
    assert len(offsets) == n + 1 and offsets[0] == 0
    bad = np.flatnonzero(np.asarray(status[:n]) != st)
    assert bad.size == 0, f"{what}: status of datagram {bad[0]}: {status[bad[0]]} != model {st[bad[0]]} ({datagrams[bad[0]][:40]!r})"
    bad = np.flatnonzero((np.asarray(drop[:n]) != 0) != ~kept)
    assert bad.size == 0, f"{what}: drop flag of datagram {bad[0]}"
    for i in range(n):
        a, b = int(offsets[i]), int(offsets[i + 1])
        assert b >= a, f"{what}: offsets not monotonic at {i}"
        assert b - a == len(slots[i]), f"{what}: datagram {i} ({st[i]}): slot of {b - a} bytes, model {len(slots[i])}"
        assert bytes(packed[a:b]) == slots[i], f"{what}: bytes of datagram {i} differ"


def build() -> Path:
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRC):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", f"-I{ROOT / 'flowgger_amd' / 'csrc'}", "-o", str(LIB),
                        str(HERE / "inflate_host.cpp")], check=True)
    return LIB


class InflateHost:
    def __init__(self):
        self.lib = C.CDLL(str(build()))
        self.lib.fgi_unpack_batch.restype = C.c_uint64
        self.lib.fgi_classify.restype = C.c_uint32

    def unpack(self, datagrams, max_inflated: int = DEFAULT_MAX):
        """-> (offsets[n + 1], packed, drop[n], status[n]) as fg_udp_unpack_device leaves them"""
        blob, offs = pack(datagrams)
        n = len(datagrams)
        data = np.zeros(blob.size + 16, np.uint8)
        data[:blob.size] = blob
        out_offs = np.zeros(n + 1, np.uint64)
        drop, status = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
        vp = lambda a: C.c_void_p(a.ctypes.data)
        args = [vp(data), vp(offs), C.c_uint64(n), C.c_uint32(max_inflated)]
        total = self.lib.fgi_unpack_batch(*args, None, C.c_uint64(0), vp(out_offs), vp(drop), vp(status))
        packed = np.zeros(total + 16, np.uint8)
        total2 = self.lib.fgi_unpack_batch(*args, vp(packed), C.c_uint64(total), vp(out_offs), vp(drop), vp(status))
        assert total2 == total
        return out_offs, packed, drop[:n], status[:n]
