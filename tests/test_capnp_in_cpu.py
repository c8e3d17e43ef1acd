"""CPU: the Cap'n Proto INPUT decoder (FG_CAPNP).  flowgger_amd/csrc/fg_capnp_parse.hpp -- the per-message parser the gfx950
kernel runs -- compiled for the host (tests/native/capnp_in_host.cpp) + the product's materialiser, against the Python model of
the reference's reader (tests/capnp_read_model.py): the reference's one vector, serialised corpora, hand-built wire shapes and a
byte-mutation fuzz.  The fuzz corpus also runs through an AddressSanitizer build that parses every message out of an exact-size
heap copy: a read outside [offsets[i], offsets[i + 1]) aborts it."""
import ctypes as C
import json
import math
import random
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

import capnp_read_model as M
import capnp_wire as W
import oracle_binding as OB
from flowgger_amd import _lib as L
from flowgger_amd import pack_messages, synth
from flowgger_amd.record import (SD_BOOL, SD_F64, SD_I64, SD_NULL, SD_STRING, SD_U64, DecodeError, Record, SDValue, StructuredData,
                                 parse_canonical)
from test_abi_cpu import _host_tables

ROOT = Path(__file__).resolve().parent.parent
NATIVE = ROOT / "tests/native"
DEPS = [NATIVE / "capnp_in_host.cpp", ROOT / "flowgger_amd/csrc/fg_capnp_parse.hpp", ROOT / "include/fg_hip.h"]
ENT_CAP = 1 << 16


def pack_words(msgs):
    """pack_messages over the whole words of each message (a mutated message may be cut anywhere; pack_messages refuses those)"""
    return pack_messages([m[:len(m) & ~7] for m in msgs])


def _fresh(out):
    return out.exists() and out.stat().st_mtime >= max(p.stat().st_mtime for p in DEPS)


@pytest.fixture(scope="module")
def host():
    lib = NATIVE / "libcapnp_in_host.so"
    if not _fresh(lib):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fno-fast-math", "-o", str(lib), str(DEPS[0])], check=True)
    lib = C.CDLL(str(lib))

    def run(msgs, ent_cap=ENT_CAP):
        """-> ([Record | DecodeError], skipped[n], HostTables, data, offsets)"""
        data, offsets = pack_words(msgs)
        n = len(msgs)
        t = _host_tables(n, ent_cap)
        skipped = np.zeros(max(n, 1), np.uint32)
        assert lib.fgc_decode_batch(C.c_void_p(data.ctypes.data), C.c_void_p(offsets.ctypes.data), C.c_uint64(n), C.byref(t.struct),
                                    C.c_void_p(skipped.ctypes.data)) == 0
        blob, offs = t.serialize(L.FG_CAPNP, data, offsets)
        raw = blob.tobytes()
        return [parse_canonical(raw[int(offs[i]):int(offs[i + 1])]) for i in range(n)], skipped, t, data, offsets
    return run


def same(got, want_model, skipped=None):
    """a materialised row == the model's verdict"""
    if want_model[0] == "err":
        return isinstance(got, DecodeError) and str(got) == want_model[1]
    if isinstance(got, DecodeError):
        return False
    return W.record_key(got) == W.record_key(want_model[1]) and (skipped is None or int(skipped) == want_model[2])


def check(host, msgs):
    got, skipped, *_ = host(msgs)
    for i, m in enumerate(msgs):
        want = M.handle_message(m)
        assert same(got[i], want, skipped[i]), (i, m.hex(), got[i], int(skipped[i]), want)
    return got


# ---- hand-built wire shapes -------------------------------------------------------------------------------------------------
def words(*ws):
    return b"".join(struct.pack("<Q", w & 0xFFFF_FFFF_FFFF_FFFF) for w in ws)


def message(*segments):
    table = [len(segments) - 1] + [len(s) // 8 for s in segments]
    if len(table) % 2:
        table.append(0)
    return struct.pack(f"<{len(table)}I", *table) + b"".join(segments)


def f64(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def text_words(s: bytes):
    s = s + b"\0"
    return s + bytes(-len(s) % 8)


def struct_ptr(off, dw, pw):
    return (off << 2) & 0xFFFF_FFFC | dw << 32 | pw << 48


def list_ptr(off, es, n):
    return 1 | (off << 2) & 0xFFFF_FFFC | (es | n << 3) << 32


def far_ptr(seg, pos, dbl=False):
    return 2 | (4 if dbl else 0) | pos << 3 | seg << 32


def simple(ts=12.5, host=b"h", dw=2, pw=9, d1=0xFFFF, extra_ptrs=()):
    """root (dw, pw) in one segment: ts, d1, hostname in pointer 0, `extra_ptrs` {slot: (pointer builder, payload words)}"""
    data = [f64(ts), d1][:dw] + [0] * max(0, dw - 2)
    ptrs = [0] * pw
    tail = b""
    base = 1 + dw + pw  # word index (in the segment) where the payloads start

    def place(slot, mk, payload):
        nonlocal tail
        if slot < pw:
            at = base + len(tail) // 8
            ptrs[slot] = mk(at - (1 + dw + slot) - 1)
            tail += payload
    if host is not None:
        place(0, lambda off: list_ptr(off, 2, len(host) + 1), text_words(host))
    for slot, (mk, payload) in dict(extra_ptrs).items():
        place(slot, mk, payload)
    return message(words(struct_ptr(0, dw, pw), *data, *ptrs) + tail)


def pair_list(items, dw=2, pw=2):
    """an inline-composite List(Pair) with element size (dw, pw): items = [(key bytes | None, which, d1, value bytes | None, bool)]"""
    n, wpe = len(items), dw + pw
    body = bytearray(8 * n * wpe)
    tail = b""
    for i, (key, which, d1, val, flag) in enumerate(items):
        e = i * wpe
        if dw >= 1:
            struct.pack_into("<Q", body, 8 * e, which | (1 << 16 if flag else 0))
        if dw >= 2:
            struct.pack_into("<Q", body, 8 * (e + 1), d1 & 0xFFFF_FFFF_FFFF_FFFF)
        for k, t in ((0, key), (1, val)):
            if t is not None and k < pw:
                at = n * wpe + len(tail) // 8
                struct.pack_into("<Q", body, 8 * (e + dw + k), list_ptr(at - (e + dw + k) - 1, 2, len(t) + 1))
                tail += text_words(t)
    tag = words(n << 2 | dw << 32 | pw << 48)
    return (lambda off: list_ptr(off, 7, n * wpe)), tag + bytes(body) + tail


ALL_KINDS = [(b"s", 0, 0, b"text", False), (b"_b", 1, 0, None, True), (b"b0", 1, 0, None, False), (b"f", 2, f64(-2.5), None, False),
             (b"i", 3, -7, None, False), (b"_u", 4, 2 ** 64 - 1, None, False), (b"n", 5, 0, None, False), (b"x", 6, 1, None, False),
             (b"y", 0xFFFF, 1, None, False), (None, 0, 0, None, False), (b"\xc3\xa9", 0, 0, b"\xe2\x82\xac", False)]


def test_reference_vector(host):
    v = json.loads((ROOT / "tests/golden/capnp_splitter_vector.json").read_text())
    msg = bytes(v["message"])
    assert len(msg) == 312
    e = v["expected"]
    kinds = {"string": SD_STRING}
    want = Record(ts=e["ts"], hostname=e["hostname"], facility=e["facility"], severity=e["severity"], appname=e["appname"],
                  procid=e["procid"], msgid=e["msgid"], msg=e["msg"], full_msg=e["full_msg"],
                  sd=[StructuredData(s["sd_id"], [(k, SDValue(kinds[t], x)) for k, t, x in s["pairs"]]) for s in e["sd"]])
    model = M.handle_message(msg)
    assert model[0] == "ok" and W.record_key(model[1]) == W.record_key(want) and model[2] == 0
    got = check(host, [msg])[0]
    assert W.record_key(got) == W.record_key(want)


@pytest.mark.parametrize("fmt,lines", [(OB.RFC5424, lambda: synth.rfc5424_lines(1500, cfg=4, sd=True)), (OB.GELF, lambda: synth.gelf_lines(1500)),
                                       (OB.LTSV, lambda: synth.ltsv_lines(1500)), (OB.RFC3164, lambda: synth.rfc3164_lines(1500))],
                         ids=["rfc5424", "gelf", "ltsv", "rfc3164"])
def test_serialised_corpora_read_back(host, oracle, fmt, lines):
    """decoder corpus -> Records (oracle) -> capnp_wire.serialize -> the parser == model(first_sd_only(record))"""
    from flowgger_amd import tzdb
    cfg = None
    if fmt == OB.RFC3164:
        oracle.set_rfc3164(2020, tzdb.default_table())
    if fmt == OB.LTSV:
        cfg = {"ltsv_schema": {"counter": "u64", "score": "i64", "mean": "f64", "done": "bool"}}
    data, offsets = synth.pack([ln if isinstance(ln, bytes) else ln.encode() for ln in lines()])
    blob, offs = oracle.decode_batch(fmt, data, offsets, config=cfg)
    recs = [parse_canonical(blob[int(offs[i]):int(offs[i + 1])].tobytes(), now=1.5) for i in range(len(offsets) - 1)]
    recs = [r for r in recs if not isinstance(r, DecodeError)]
    assert len(recs) > 1000
    for extra in (None, [("_k", "shadow"), ("a", ""), ("host", "h2")]):
        msgs = [W.serialize(r, extra) for r in recs]
        got = check(host, msgs)
        n_ok = 0
        for r, g in zip(recs, got):
            if math.isnan(r.ts) or r.ts <= 0.0:
                assert str(g) == M.ERR_TS
                continue
            n_ok += 1
            w = W.first_sd_only(r)
            for f in ("appname", "procid", "msgid", "msg", "full_msg"):  # None is a null pointer on the wire: Some("") here
                assert getattr(g, f) == (getattr(w, f) or "")
            assert (g.hostname, g.facility, g.severity, struct.pack("<d", g.ts)) == (w.hostname, w.facility, w.severity, struct.pack("<d", w.ts))
            pairs = [] if w.sd is None else [(k, (v.kind, v.value)) for k, v in w.sd[0].pairs]
            assert g.sd is not None and len(g.sd) == 1 and g.sd[0].sd_id == ("" if w.sd is None or w.sd[0].sd_id is None else w.sd[0].sd_id)
            gp = [(k, (v.kind, v.value)) for k, v in g.sd[0].pairs]
            assert gp[:len(pairs)] == [(k if k.startswith("_") else "_" + k, v) for k, v in pairs]
            assert gp[len(pairs):] == [(k, (SD_STRING, v)) for k, v in (extra or [])]     # extras: keys verbatim
        assert n_ok > 1000


def test_every_field_null_and_struct_sizes(host):
    msgs = [simple(host=None),                                  # every pointer null: "" everywhere, sd Some([{"", []}])
            message(words(0)),                                   # a NULL root: ts reads 0
            simple(dw=1, pw=3), simple(dw=2, pw=9), simple(dw=3, pw=12), simple(dw=0, pw=1), simple(dw=1, pw=0),
            simple(dw=2, pw=0), simple(dw=2, pw=7), simple(dw=2, pw=8)]
    got = check(host, msgs)
    r = got[0]
    assert (r.hostname, r.appname, r.full_msg, r.facility, r.severity) == ("", "", "", None, None)
    assert r.sd is not None and r.sd[0].sd_id == "" and r.sd[0].pairs == []
    assert str(got[1]) == M.ERR_TS and str(got[5]) == M.ERR_TS
    assert got[2].hostname == "h" and got[2].facility == 0 and got[2].severity == 0   # one data word: facility / severity read as 0


@pytest.mark.parametrize("ts,ok", [(float("nan"), False), (0.0, False), (-0.0, False), (-1.0, False), (5e-324, True), (float("inf"), True),
                                   (float("-inf"), False), (1385053862.3072, True)])
def test_timestamps(host, ts, ok):
    got = check(host, [simple(ts=ts)])[0]
    assert (not isinstance(got, DecodeError)) == ok and (ok or str(got) == M.ERR_TS)
    if ok:
        assert struct.pack("<d", got.ts) == struct.pack("<d", ts)


@pytest.mark.parametrize("fac,sev", [(0, 0), (31, 7), (32, 8), (255, 255), (31, 8), (32, 7)])
def test_facility_and_severity(host, fac, sev):
    got = check(host, [simple(d1=fac | sev << 8)])[0]
    assert got.facility == (fac if fac <= 31 else None) and got.severity == (sev if sev <= 7 else None)


@pytest.mark.parametrize("dw,pw", [(2, 2), (1, 2), (0, 2), (3, 3), (2, 1), (2, 0), (0, 0), (5, 4)])
def test_pairs_every_kind_and_stride(host, dw, pw):
    """all six value kinds, unknown discriminants, keys with and without '_', a null key; element sizes other than the schema's
    (the stride comes from the tag); the same list as `extra` keeps only the strings, keys verbatim"""
    mk, payload = pair_list(ALL_KINDS, dw, pw)
    got = check(host, [simple(extra_ptrs={7: (mk, payload)}), simple(extra_ptrs={8: (mk, payload)}),
                       simple(extra_ptrs={6: (lambda off: list_ptr(off, 2, 3), text_words(b"id")), 7: (mk, payload), 8: (mk, payload)})])
    if (dw, pw) == (2, 2):
        p = got[0].sd[0].pairs
        assert [k for k, _ in p] == ["_s", "_b", "_b0", "_f", "_i", "_u", "_n", "_", "_é"]
        assert [v.kind for _, v in p] == [SD_STRING, SD_BOOL, SD_BOOL, SD_F64, SD_I64, SD_U64, SD_NULL, SD_STRING, SD_STRING]
        assert (p[1][1].value, p[2][1].value, p[3][1].value, p[4][1].value, p[5][1].value) == (True, False, -2.5, -7, 2 ** 64 - 1)
        assert [(k, v.value) for k, v in got[1].sd[0].pairs] == [("s", "text"), ("", ""), ("é", "€")]
        assert got[2].sd[0].sd_id == "id" and len(got[2].sd[0].pairs) == 12


def test_non_composite_lists_are_upgraded(host):
    """List(Pair) through a list pointer of another element size: void, byte .. eight bytes, pointer; a bit list fails"""
    cases = []
    for es, n, payload in [(0, 3, b""), (2, 5, bytes([0, 1, 5, 6, 0, 0, 0, 0])), (3, 3, struct.pack("<4H", 0, 5, 7, 0)),
                           (4, 2, struct.pack("<2I", 1 | 1 << 16, 1)), (5, 2, words(1 | 1 << 16, 4)), (1, 9, bytes(8)),
                           (6, 2, words(list_ptr(1, 2, 2), list_ptr(1, 2, 4)) + text_words(b"k") + text_words(b"key"))]:
        for slot in (7, 8):
            cases.append(simple(extra_ptrs={slot: ((lambda off, es=es, n=n: list_ptr(off, es, n)), payload + bytes(-len(payload) % 8))}))
    got = check(host, cases)
    assert [k for k, _ in got[0].sd[0].pairs] == ["_", "_", "_"] and got[1].sd[0].pairs == [("", SDValue(SD_STRING, "")), ] * 3
    assert [k for k, _ in got[12].sd[0].pairs] == ["_k", "_key"]
    assert got[10].sd[0].pairs == [] and got[11].sd[0].pairs == []   # bit list: the getter fails, sd stays Some (sd_id is Ok)


def test_far_pointers_and_segments(host):
    root = words(struct_ptr(0, 2, 9), f64(3.0), 0x0105)
    seg1_text = words(list_ptr(0, 2, 4)) + text_words(b"far")                  # landing pad at word 0, text at word 1
    hostp = far_ptr(1, 0)
    msgs = [
        message(root + words(hostp, *[0] * 8), seg1_text),                       # single far
        message(root + words(far_ptr(1, 0, True), *[0] * 8), words(far_ptr(2, 1), list_ptr(0, 2, 4)), words(0) + text_words(b"dbl")),  # double far
        message(root + words(far_ptr(1, 1), *[0] * 8), seg1_text),               # the pad is the text itself: wrong kind or out of bounds
        message(root + words(far_ptr(1, 2), *[0] * 8), seg1_text),               # pad outside its segment
        message(root + words(far_ptr(5, 0), *[0] * 8), seg1_text),               # no such segment
        message(root + words(far_ptr(1, 0), *[0] * 8), words(far_ptr(1, 0)) + text_words(b"x")),  # the pad is itself far
        message(words(far_ptr(1, 0)), words(struct_ptr(0, 2, 9), f64(3.0), 0x0105, *[0] * 9)),     # a far ROOT
        message(words(far_ptr(1, 0)), words(list_ptr(0, 2, 8), 0)),              # the root is no struct
        message(root + words(list_ptr(-2, 2, 8), *[0] * 8)),                    # negative offset: back into the root's data
        message(root + words(list_ptr(-5, 2, 8), *[0] * 8)),                    # ... and out of the segment
        message(root + words(list_ptr(8, 2, 8), *[0] * 8)),                      # target beyond the segment
        message(root + words(struct_ptr(8, 0, 0), *[0] * 8)),                    # wrong kind for a text
        message(root + words(list_ptr(8, 3, 1), *[0] * 8) + words(0)),           # list of two-byte elements
        message(root + words(list_ptr(8, 2, 0), *[0] * 8)),                      # zero-length text list
        message(root + words(list_ptr(8, 2, 3), *[0] * 8) + b"abc\0\0\0\0\0"),   # no NUL at the end
        message(root + words(list_ptr(8, 2, 3), *[0] * 8) + b"\xff\xfe\0\0\0\0\0\0"),  # not UTF-8
        message(root + words(list_ptr(8, 2, 4), *[0] * 8) + b"\xed\xa0\x80\0\0\0\0\0"),  # a surrogate
        message(root + words(list_ptr(8, 2, 4), *[0] * 8) + b"a\0b\0\0\0\0\0"),  # NUL inside is fine
        struct.pack("<4I", 1, 12, 100, 0) + root + words(far_ptr(1, 0), *[0] * 8) + seg1_text,   # segment 1 claims more than the message has
        struct.pack("<2I", 0, 100) + root + words(0, *[0] * 8),                  # segment 0 cut at the end of the message
        struct.pack("<2I", 0, 5) + root,                                         # the root struct is cut off
        struct.pack("<2I", 511, 1) + bytes(8 * 300),                             # 512 segments
        struct.pack("<2I", 510, 1) + bytes(8 * 300),                             # 511 segments: the table is all there
        b"", b"\0" * 7, words(0),                                                # nothing; no table; an empty segment 0
    ]
    got = check(host, msgs)
    assert got[0].hostname == "far" and got[1].hostname == "dbl" and got[6].severity == 1 and got[6].facility == 5
    assert [str(got[k]) for k in (2, 3, 4, 5, 9, 10, 11, 12, 13, 14, 15, 16)] == [M.ERR_HOST] * 12
    assert got[8].hostname == "\x05\x01\0\0\0\0\0"
    assert got[17].hostname == "a\0b"
    assert [str(got[k]) for k in (7, 20, 21, 23, 24, 25)] == [M.ERR_ROOT] * 6
    assert got[18].hostname == "far" and got[19].hostname == ""


def test_a_long_full_msg_and_overflow(host):
    big = ("x" * 69_990 + "é" * 5).encode()
    rec = Record(ts=9.0, hostname="h", full_msg=big.decode(), sd=[StructuredData("id", [("k", SDValue(SD_U64, 7))])])
    msg = W.serialize(rec)
    assert len(msg) > 70_000
    got = check(host, [msg])[0]
    assert got.full_msg.encode() == big and got.sd[0].pairs == [("_k", SDValue(SD_U64, 7))]
    # an entry table that is too small: the row says so, the rows before it are whole
    rows, _, t, *_ = host([msg, msg, msg], ent_cap=5)
    assert [int(m) & 0xFF for m in t.a["meta"][:3]] == [0, 0, L.FG_ST_OVERFLOW] and not isinstance(rows[1], DecodeError)


def mutate(r: random.Random, msg: bytes) -> bytes:
    b = bytearray(msg)
    for _ in range(r.choice([1, 1, 1, 2, 3, 6])):
        k = r.random()
        if k < 0.45 and len(b):       # a byte anywhere
            b[r.randrange(len(b))] = r.choice([0, 1, 2, 3, 5, 6, 7, 0xFF, 0x80, r.randrange(256)])
        elif k < 0.8 and len(b) >= 16:   # a byte of a pointer-dense region: the root struct and the table
            i = r.randrange(min(len(b), 8 * 14))
            b[i] = r.choice([b[i] ^ (1 << r.randrange(8)), r.randrange(256)])
        elif k < 0.9 and len(b) > 8:     # cut the message
            del b[r.randrange(8, len(b)):]
        else:                            # a whole word
            i = r.randrange(max(1, len(b) // 8)) * 8
            b[i:i + 8] = struct.pack("<Q", r.choice([0, r.getrandbits(64), far_ptr(r.randrange(3), r.randrange(40), r.random() < 0.3),
                                                     list_ptr(r.randrange(-20, 40), r.randrange(8), r.randrange(50)),
                                                     struct_ptr(r.randrange(-20, 40), r.randrange(4), r.randrange(12))]) & 0xFFFF_FFFF_FFFF_FFFF)
    return bytes(b)


def fuzz_corpus(n, seed):
    r = random.Random(seed)
    mk, payload = pair_list(ALL_KINDS)
    mk2, payload2 = pair_list(ALL_KINDS[:4], 3, 3)
    v = bytes(json.loads((ROOT / "tests/golden/capnp_splitter_vector.json").read_text())["message"])
    seeds = [v, simple(extra_ptrs={6: (lambda off: list_ptr(off, 2, 3), text_words(b"id")), 7: (mk, payload), 8: (mk2, payload2)}),
             message(words(struct_ptr(0, 2, 9), f64(3.0), 0x0105, far_ptr(1, 0), *[0] * 8), words(list_ptr(0, 2, 4)) + text_words(b"far")),
             message(words(struct_ptr(0, 2, 9), f64(3.0), 0x0105, far_ptr(1, 0, True), *[0] * 8), words(far_ptr(2, 1), list_ptr(0, 2, 4)),
                     words(0) + text_words(b"dbl")),
             W.serialize(Record(ts=1.0, hostname="hé", appname="a", msg="m" * 40, sd=[StructuredData(None, [("k", SDValue(SD_STRING, "v")),
                                                                                                            ("_b", SDValue(SD_BOOL, True))])]),
                         [("x", "y")])]
    return [mutate(r, r.choice(seeds)) for _ in range(n)]


def test_mutation_fuzz_equals_the_model(host):
    """20 000 mutated messages, fixed seed: parser and model agree on the status, the Record and the skipped pairs"""
    msgs = fuzz_corpus(20_000, 20261016)
    got, skipped, t, *_ = host(msgs)
    n_ok = n_err = n_skip = 0
    seen = set()
    for i, m in enumerate(msgs):
        want = M.handle_message(m, max_pairs=ENT_CAP // 2)
        if want[0] == "big":   # (a mutated count of zero-sized elements: more entries than this test's table holds)
            assert (int(t.a["meta"][i]) & 0xFF) == L.FG_ST_OVERFLOW, (i, m.hex())
            continue
        assert same(got[i], want, skipped[i]), (i, m.hex(), got[i], int(skipped[i]), want)
        if want[0] == "ok":
            n_ok += 1
            n_skip += want[2] > 0
        else:
            n_err += 1
            seen.add(want[1])
    assert seen == {M.ERR_TS, M.ERR_HOST, M.ERR_ROOT} and n_ok > 5000 and n_err > 1000 and n_skip > 100


def test_fuzz_never_reads_outside_the_message():
    """the same corpus through the AddressSanitizer build: every message parsed out of an exact-size heap copy"""
    exe = NATIVE / "capnp_in_host_asan"
    if not _fresh(exe):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fno-fast-math", "-fsanitize=address", "-static-libasan", "-DFGC_MAIN", "-o", str(exe),
                        str(DEPS[0])], check=True)
    msgs = fuzz_corpus(20_000, 20261016) + fuzz_corpus(5_000, 7)
    data, offsets = pack_words(msgs)
    path = NATIVE / "capnp_in_fuzz.bin"
    try:
        path.write_bytes(struct.pack("<Q", len(msgs)) + offsets.tobytes() + data.tobytes())
        r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=600)
    finally:
        path.unlink(missing_ok=True)
    assert r.returncode == 0 and "messages" in r.stdout, (r.returncode, r.stdout[-400:], r.stderr[-2000:])


def test_abi_constants_and_error_strings():
    assert L.FG_CAPNP == 4 and L.FG_EF_NAME_VERBATIM == 8
    lib = L.lib()
    assert lib.fg_abi_version() == 4
    es = lambda k: lib.fg_error_string(L.FG_CAPNP, k)  # noqa: E731
    assert (es(0), es(1), es(2)) == (b"", b"Missing timestamp", b"Missing host name") and es(3) == M.ERR_ROOT.encode() and es(4) is None
    hdr = (ROOT / "include/fg_hip.h").read_text()
    assert "FG_CAPNP = 4" in hdr and "FG_EF_NAME_VERBATIM = 8" in hdr


def test_pack_messages_refuses_ragged_messages():
    with pytest.raises(ValueError):
        pack_messages([simple(), simple() + b"\0\0\0"])
    data, offsets = pack_messages([simple(), simple()])
    assert list(offsets) == [0, len(simple()), 2 * len(simple())]
