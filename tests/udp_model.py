"""What the UDP input tests share (test infrastructure): the model of handle_record_maybe_compressed (src/flowgger/input/udp_input.rs:
100-143) with Python's zlib as the inflater, the case list, the mutation pool, and the ctypes binding of
tests/native/libinflate_host.so (flowgger_amd/csrc/fg_inflate.hpp compiled for the CPU)."""
from __future__ import annotations

import ctypes as C
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
SRC = [HERE / "inflate_host.cpp", ROOT / "flowgger_amd" / "csrc" / "fg_inflate.hpp", ROOT / "flowgger_amd" / "csrc" / "fg_syslen_parse.hpp"]

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


def gz_member(payload: bytes, extra=None, name=None, comment=None, hcrc=False, level=6, bad_hcrc=False, crc_delta=0, isize_delta=0) -> bytes:
    """an RFC 1952 member built by hand around a raw deflate stream"""
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
