"""CPU: the octet-counted framer's device logic (flowgger_amd/csrc/fg_syslen.hpp: tile resolve, inbox, chain ranking, emit + pack) on the
wave emulation, and its prefix parser, against a restatement of read_msglen (src/flowgger/splitter/syslen_splitter.rs:17-25) and the
sequential walk (syslen_binding.py)."""
from __future__ import annotations

import numpy as np
import pytest

from flowgger_amd import synth
from syslen_binding import BAD_LEN, CLEAN, LONG_PREFIX, TAIL, VALID, SyslenHost, read_msglen, valid_utf8, walk


@pytest.fixture(scope="module")
def host():
    return SyslenHost()


def as_bytes(ln):
    return ln if isinstance(ln, bytes) else ln.encode()


def wrap(msgs, nl=True):
    return b"".join(b"%d %s" % (len(m) + (1 if nl else 0), m + (b"\n" if nl else b"")) for m in map(as_bytes, msgs))


def check(host, buf, may_decline=False):
    """every run reproduces the frames, `consumed` and the stop reason of the sequential walk (with the parser's bound)"""
    starts, plens, lens, consumed, stop = walk(buf, host.max_prefix)
    r = host.frame(buf)
    if r["declined"]:
        assert may_decline, "the device logic declined"
        return None
    assert (r["n"], r["consumed"], r["stop"]) == (len(starts), consumed, stop)
    assert list(r["starts"]) == starts + [consumed]
    payloads = [buf[s + p:s + p + n] for s, p, n in zip(starts, plens, lens)]
    assert list(r["offsets"]) == [0] + list(np.cumsum([len(p) for p in payloads], dtype=np.int64))
    exp = b"".join(payloads)
    assert bytes(r["packed"][:len(exp)]) == exp
    assert list(r["bad"]) == [0 if valid_utf8(p) else 1 for p in payloads]
    return r


def verdict(r):
    """(status, prefix length, payload length); the lengths mean something only for a well-formed prefix whose payload fits"""
    return r if r[0] == VALID else (r[0],)


def test_prefix_parser_equals_read_msglen(host):
    b = host.max_prefix
    cases = [b"+5 hello", b"005 hello", b"+ x", b" x", b"-1 x", b"5x hello", b"5", b"+", b"", b"0 ", b"0", b"12 short",
             b"18446744073709551615 x", b"18446744073709551616 x", b"99999999999999999999 x", b"00000000000000000000000 ",
             b"0" * (b - 2) + b"1 x", b"0" * (b - 1) + b" ", b"0" * b + b" ", b"0" * (b - 1), b"0" * b, b"0" * (b + 5), b"1" * b + b"x",
             b"0" * (b - 1) + b"x", b"+" + b"0" * (b - 2) + b" ", b"++1 a", b"1+ a", b"1\t a"]
    for buf in cases:
        for bound in (b, None):
            assert verdict(host.parse(buf, 0, bound)) == verdict(read_msglen(buf, 0, bound)), (buf, bound)
    rng = np.random.default_rng(5)
    alphabet = np.frombuffer(b"0123456789 +x", np.uint8)
    for _ in range(3000):
        buf = alphabet[rng.integers(0, len(alphabet), rng.integers(0, 40))].tobytes()
        p = int(rng.integers(0, len(buf) + 1))
        assert verdict(host.parse(buf, p, b)) == verdict(read_msglen(buf, p, b)), (buf, p)


def test_utf8_rule_equals_str_from_utf8(host):
    rng = np.random.default_rng(6)
    alphabet = [b"a", b"\xc3\xa9", b"\xe2\x82\xac", b"\xf0\x9f\x98\x80", b"\x80", b"\xc0", b"\xe0\x80", b"\xed\xa0\x80", b"\xf4\x90", b"\xff", b"\xe2", b"\xf0\x9f"]
    for _ in range(4000):
        s = b"".join(alphabet[k] for k in rng.integers(0, len(alphabet), rng.integers(0, 8)))
        assert host.utf8_bad(s) == (not valid_utf8(s)), s


def mixed(n):
    _, (la, ia), (lb, ib) = synth.mixed_cfg5(n)
    out = [None] * n
    for lines, idx in ((la, ia), (lb, ib)):
        for ln, i in zip(lines, idx):
            out[int(i)] = ln
    return out


CORPORA = {
    "cfg2": lambda: synth.rfc5424_lines(600, cfg=2), "cfg4_sd": lambda: synth.rfc5424_lines(500, cfg=4, sd=True),
    "cfg5_long_tail": lambda: synth.rfc5424_lines(300, cfg=5, long_tail=True), "gelf": lambda: synth.gelf_lines(500),
    "ltsv": lambda: synth.ltsv_lines(500), "ltsv_long_tail": lambda: synth.ltsv_lines(300, long_tail=True),
    "rfc3164": lambda: synth.rfc3164_lines(600), "mixed": lambda: mixed(400),
}


@pytest.mark.parametrize("nl", [True, False], ids=["nl", "bare"])
@pytest.mark.parametrize("name", sorted(CORPORA))
def test_synth_corpora_are_framed_exactly_and_never_decline(host, name, nl):
    r = check(host, wrap(CORPORA[name](), nl))  # (may_decline = False: zero declines on the synth corpora is a condition)
    assert r["stop"] == CLEAN


def test_payloads_that_look_like_prefixes_long_frames_and_empty_frames(host):
    check(host, wrap([b"12 34 56 7 8 9 10 11 300 ", b"+5 005 ", b"1 2 3 4 5 6 7 8 9 ", b"3 abc"] * 40, nl=False))
    check(host, wrap([b"x" * 20000, b"", b"y" * 4095, b"", b"", b"z" * 4096, b"w" * 9000] * 2, nl=False))
    check(host, b"0 " * 9000)
    check(host, b"+0 00 " * 3000 + b"7 ")
    check(host, wrap([b"caf\xc3\xa9", b"cut \xe2\x82", b"ok", b"\xff", b"tail \xc3"] * 300, nl=False))


def test_chunks_cut_at_every_offset(host):
    stream = wrap([b"<13>1 - h a 1 m - hello", b"", b"0 1 ", b"x" * 70, b"gr\xc3\xbc\xc3\x9fe"], nl=False) + b"5 abcde"
    for cut in range(len(stream) + 1):
        r = check(host, stream[:cut])
        assert r["stop"] in (CLEAN, TAIL)
    for bad in (b" ", b"x", b"+ ", b"5x ", b"-1 "):
        r = check(host, stream + bad + stream)
        assert (r["stop"], r["consumed"]) == (BAD_LEN, len(stream))
    r = check(host, stream + b"0" * 30 + b"1 a")
    assert (r["stop"], r["consumed"]) == (LONG_PREFIX, len(stream))


def test_a_list_of_distinct_numbers_near_a_tile_end_declines(host):
    body = b" ".join(b"%d" % i for i in range(1000, 1900))
    raw = wrap([b"first", body] + [b"filler " + b"x" * 200] * 40)
    assert host.frame(raw)["declined"] != 0
    assert walk(raw)[4] == CLEAN  # (the stream itself is fine: the caller hops it on the host)
