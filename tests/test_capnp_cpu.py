"""CPU: the Cap'n Proto encoder (output.format = "capnp") the kernels run -- flowgger_amd/csrc/fg_emit.hpp CapnpEmitter with its
configuration (fg_enc_cfg.hpp), host build in tests/native/capnp_host.cpp -- against a clean-room model of the wire format
(tests/capnp_wire.py), which reproduces the reference's own test vectors (encoder/capnp_encoder.rs, tests/golden).  Every record
goes through the count pass and the write pass at all sixteen output alignments inside a guarded buffer; the bytes must equal the
model's, and the model's reader must get the record back."""
import ctypes as C
import json
import random
import struct
import subprocess
from pathlib import Path

import pytest

import capnp_wire as W
from flowgger_amd.record import Record, SDValue, StructuredData, parse_canonical
from test_emit_cpu import rrecord, rstr
from test_encoder_cpu import canonical

ROOT = Path(__file__).resolve().parent.parent
RFC5424, LTSV, GELF, RFC3164 = 0, 1, 2, 3
SRC_IDS = {RFC5424: "rfc5424", LTSV: "ltsv", GELF: "gelf", RFC3164: "rfc3164"}
NAN_PAYLOAD = struct.unpack("<d", struct.pack("<Q", 0x7FF8_0000_DEAD_BEEF))[0]


@pytest.fixture(scope="module")
def capnp():
    src, lib = ROOT / "tests/native/capnp_host.cpp", ROOT / "tests/native/libcapnp_host.so"
    deps = [src, ROOT / "tests/native/emit_host.cpp"] + [ROOT / "flowgger_amd/csrc" / n for n in (
        "fg_emit.hpp", "fg_enc_cfg.hpp", "fg_shortest.hpp", "fg_dtoa.hpp", "fg_tables_view.hpp", "fg_timeconv.hpp",
        "fg_unicode_ws.hpp")] + [ROOT / "include/fg_hip.h"]
    if not lib.exists() or lib.stat().st_mtime < max(p.stat().st_mtime for p in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fPIC", "-shared", "-fno-fast-math", "-Wno-unknown-pragmas", "-o", str(lib), str(src)],
                       check=True)
    L = C.CDLL(str(lib))
    L.fgc_encode_canonical.restype = C.c_int64
    L.fgc_encode_canonical.argtypes = [C.c_int, C.c_int, C.c_uint64, C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32,
                                       C.c_double, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint32)]

    def run(rec: dict, src: int, merger: int = 0, extra=None, now_ts: float = 0.0, seed: int = 1):
        cb = canonical(**rec)
        items = sorted((extra or {}).items())
        ks = (C.c_char_p * max(len(items), 1))(*[k.encode() for k, _ in items])
        vs = (C.c_char_p * max(len(items), 1))(*[v.encode() for _, v in items])
        st = C.c_uint32()
        cap = 8 * len(cb) + 65536
        buf = C.create_string_buffer(cap)
        n = L.fgc_encode_canonical(merger, src, seed, cb, len(cb), ks, vs, len(items), now_ts, buf, cap, C.byref(st))
        assert n >= 0, n
        assert st.value == 0
        return buf.raw[:n]
    return run


def model(rec: dict, extra=None, now_ts: float = 0.0):
    """the Record the row stands for, and its message"""
    r = parse_canonical(canonical(**rec), now=now_ts)
    return r, W.serialize(r, sorted((extra or {}).items()))


def check(capnp, rec, src, merger=0, extra=None, now_ts=0.0, seed=1, segments=None):
    got = capnp(rec, src, merger, extra, now_ts, seed)
    r, want = model(rec, extra, now_ts)
    assert got == W.frame(want, merger)
    back, ex, used = W.parse(W.unframe(got, merger))
    assert used == len(want)
    assert W.record_key(back) == W.record_key(W.first_sd_only(r))
    assert ex == sorted((extra or {}).items())
    if segments is not None:
        assert struct.unpack_from("<I", W.unframe(got, merger))[0] + 1 == segments
    return got


def vector_record(v, decoded_keys=False):
    """the vector's Record as canonical() kwargs; decoded_keys: every key with the '_' a decoder gives it (sd[1] of the
    multiple-SD vector has "info", which no decoder produces and which is not on the wire)"""
    r = dict(v["record"])
    sd = r.pop("sd")
    if sd is not None:
        fix = (lambda k: k if k.startswith("_") else "_" + k) if decoded_keys else (lambda k: k)
        sd = [(e["sd_id"], [(fix(k), ({"String": 0, "F64": 2}[kind], val)) for k, kind, val in e["pairs"]]) for e in sd]
    return dict(r, sd=sd)


VECTORS = json.loads((ROOT / "tests/golden/capnp_reference_vectors.json").read_text())["vectors"]


def test_the_model_reproduces_the_reference_vectors():
    for v in VECTORS:
        r = parse_canonical(canonical(**vector_record(v)))
        msg = W.serialize(r, sorted(v["extra"].items()))
        assert msg.decode("utf-8", "replace") == v["expected_lossy"], v["source"]
        back, _, _ = W.parse(msg)
        assert W.record_key(back) == W.record_key(W.first_sd_only(r))
    # the multiple-SD vector: sd[1] is not on the wire -- its message is the one-element vector's
    one, multi = (parse_canonical(canonical(**vector_record(VECTORS[k]))) for k in (0, 2))
    assert len(multi.sd) == 2 and W.serialize(multi) == W.serialize(one)
    assert b"someid2" not in W.serialize(multi)


def test_reference_vectors_through_the_emitter(capnp):
    for v in VECTORS:
        got = capnp(vector_record(v, decoded_keys=True), RFC5424, extra=v["extra"])
        assert got.decode("utf-8", "replace") == v["expected_lossy"], v["source"]


BASE = dict(ts=1385053862.3072, hostname="example.org", severity=1, appname="appname", procid="44", msg="m", full_msg="full")


def test_every_value_type(capnp):
    pairs = [("_t", (1, True)), ("_f", (1, False)), ("_z", (2, 0.0)), ("_nz", (2, -0.0)), ("_nan", (2, NAN_PAYLOAD)),
             ("_inf", (2, float("-inf"))), ("_x", (2, 123.456)), ("_neg", (3, -42)), ("_min", (3, -2 ** 63)), ("_max", (4, 2 ** 64 - 1)),
             ("_null", (5, None)), ("_s", (0, "v"))]
    for src in (LTSV, GELF, RFC3164):
        check(capnp, dict(BASE, sd=[(None, pairs)]), src)
    check(capnp, dict(BASE, sd=[("id", pairs)]), RFC5424)


def test_padding_edges_and_nul_bytes(capnp):
    for n in (0, 1, 7, 8, 9, 15, 16, 17, 23, 24, 31, 32, 33):
        s = "".join("abcdefghij"[i % 10] for i in range(n))
        rec = dict(ts=1.5, hostname=s, appname=s[:7], procid=s[:8], msgid=s[:9], msg=s + "\0x\0", full_msg="\0" * n,
                   sd=[("i" * n, [("_" + "k" * n, (0, s)), ("_e", (0, "")), ("_n", (0, "a\0b"))])])
        check(capnp, rec, RFC5424)
        check(capnp, dict(rec, sd=[(None, rec["sd"][0][1])]), LTSV)
    check(capnp, dict(ts=0.0, hostname=""), LTSV)  # nothing but an empty hostname


def test_structured_data_shapes(capnp):
    check(capnp, dict(BASE, sd=[(None, [("_a", (0, "1"))])]), LTSV)                      # sd_id None
    check(capnp, dict(BASE, sd=[("empty", [])]), RFC5424)                                 # `[empty]`: a list of 0 pairs
    check(capnp, dict(BASE, sd=[("", [])]), RFC5424)
    got = check(capnp, dict(BASE, sd=[("a", [("_k", (0, "v"))]), ("b", [("_dropped", (0, "x"))]), ("c", [])]), RFC5424)
    assert b"_dropped" not in got  # only sd[0] is encoded
    check(capnp, dict(BASE, sd=[("a", []), ("b", [("_k", (0, "v"))])]), RFC5424)
    check(capnp, dict(BASE, sd=None), RFC5424)


def test_escaped_sources_are_decoded(capnp):
    vals = ['q"uote', "back\\slash", "br]acket", 'all"\\]', "x\\y", "plain"]
    check(capnp, dict(BASE, sd=[("id", [("_k%d" % i, (0, v)) for i, v in enumerate(vals)])]), RFC5424)
    r = random.Random(7)
    for i in range(200):  # JSON-escaped GELF spans: host, msg, full_msg, keys and values (random escape forms)
        rec = dict(ts=r.uniform(0, 2e9), hostname=rstr(r, 0, 20), msg=rstr(r, 0, 40), full_msg=rstr(r, 0, 60),
                   sd=[(None, [("_" + rstr(r, 0, 6), (0, rstr(r, 0, 30))) for _ in range(r.randint(1, 4))])])
        check(capnp, rec, GELF, seed=i)
    for i in range(50):  # RFC3164 msg: the whitespace-joined text, from source text with runs of spaces and tabs
        words = ["".join(r.choice("abcXYZ09.:-") for _ in range(r.randint(1, 9))) for _ in range(r.randint(1, 8))]
        check(capnp, dict(BASE, msg=" ".join(words)), RFC3164, seed=i)


@pytest.mark.parametrize("merger", [0, 1, 2, 3], ids=["none", "line", "nul", "syslen"])
def test_extras_and_mergers(capnp, merger):
    extra = {"x-header1": "header1 value", "a": "", "zz\t": 'v"\tw', "k" * 9: "v" * 17}
    check(capnp, dict(BASE, sd=None), RFC5424, merger, extra)
    check(capnp, dict(BASE, sd=[("id", [("_a", (0, "b"))])]), RFC5424, merger, extra)
    check(capnp, dict(BASE, sd=[(None, [("_a", (3, -1))])]), LTSV, merger, {"one": "1"})
    check(capnp, dict(BASE, sd=None), GELF, merger)


def test_ts_now_takes_the_callers_clock(capnp):
    rec = dict(BASE)
    cb = bytearray(canonical(**rec))
    cb[1] = 1  # FG_F_TS_NOW
    r = parse_canonical(bytes(cb), now=1234.5)
    assert r.ts == 1234.5
    got = capnp(rec, GELF, now_ts=1234.5)  # (the canonical ts travels as written: 1385053862.3072 -- not NOW)
    assert W.parse(got)[0].ts == rec["ts"]


def test_messages_beyond_the_first_segment(capnp):
    big = lambda n, c="m": (c * (n // len(c) + 1))[:n]
    # msg + full_msg past 1024 words: full_msg lands in a second segment behind a far pointer
    check(capnp, dict(BASE, msg=big(5000), full_msg=big(5000, "f")), RFC5424, segments=2)
    # msg alone past the first segment (segment 1: 2048 words), full_msg past both (segment 2: 4096 words)
    check(capnp, dict(BASE, msg=big(9000), full_msg=big(17000, "F")), RFC5424, segments=3)
    # a large text goes to segment 1, the next small one back into segment 0
    got = check(capnp, dict(BASE, msg=big(9000), full_msg="tiny", sd=[("id", [("_k", (0, "v"))])]), RFC5424, segments=2)
    assert got.index(b"tiny\0") < got.index(big(100).encode())
    # the pairs list does not fit segment 0: it opens segment 1, and its keys and values follow it there
    check(capnp, dict(BASE, msg=big(8050), sd=[("id", [("_key%d" % i, (0, "val%d" % i)) for i in range(12)])]), RFC5424, segments=2)
    # the list fits segment 0 but its texts do not: far pointers out of the Pair structs
    for n in range(7960, 8100, 8):
        check(capnp, dict(BASE, msg=big(n), sd=[("id", [("_key%d" % i, (0, big(40, "v"))) for i in range(6)])]), RFC5424)
    # the extra list spills too
    check(capnp, dict(BASE, msg=big(8130), sd=None), RFC5424, 3, {"k%d" % i: "v" * i for i in range(20)})
    check(capnp, dict(BASE, msg=big(30000), full_msg=big(30000, "g"), sd=[(None, [("_k", (0, big(20000, "z")))])]), LTSV, 1, {"e": "x"})


@pytest.mark.parametrize("src", [RFC5424, LTSV, GELF, RFC3164], ids=lambda s: "src_" + SRC_IDS[s])
def test_random_records(capnp, src):
    r = random.Random(4242 + src)
    extras = [None, {"x-header1": "header1 value"}, {"_k": "", "host": 'h"2', "zz": "\n"}]
    for i in range(400):
        rec = rrecord(r, src)
        if src == RFC3164 and rec["msg"] is not None:
            rec["msg"] = " ".join("".join(r.choice("abc:[]09") for _ in range(r.randint(1, 6))) for _ in range(r.randint(1, 5)))
        if r.random() < 0.08:
            rec["full_msg"] = "L" * r.randint(7000, 20000)
        check(capnp, rec, src, r.randint(0, 3), r.choice(extras), 99.25, seed=i)


def test_python_api_for_the_capnp_encoder():
    from flowgger_amd import CapnpEncoder, _lib as L
    e = CapnpEncoder({"output": {"capnp_extra": {"zz": "1", "aa": "2", "x-header1": "header1 value"}}})
    assert e.enc == L.FG_ENC_CAPNP == 5
    assert e.extra == [("aa", "2"), ("x-header1", "header1 value"), ("zz", "1")]
    assert e.merger == L.FG_MERGE_NONE
    for f in ("capnp", "noop", "nop", "none"):
        assert CapnpEncoder({"output": {"framing": f}}).merger == L.FG_MERGE_NONE
    assert CapnpEncoder({"output": {"framing": "line"}}).merger == L.FG_MERGE_LINE
    with pytest.raises(TypeError):
        CapnpEncoder({"output": {"capnp_extra": {"x-header1": 123}}})
