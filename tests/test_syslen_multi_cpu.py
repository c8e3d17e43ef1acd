"""CPU: the SEGMENTED octet-counted framer's device logic (flowgger_amd/csrc/fg_syslen_multi.hpp: the chunks of many connections in one
launch) on the wave emulation, against the sequential walk of every segment (syslen_multi_model.py)."""
from __future__ import annotations

import numpy as np
import pytest

from syslen_binding import BAD_LEN, CLEAN, LONG_PREFIX, TAIL, SyslenHost
from syslen_multi_binding import SyslenMultiHost
from syslen_multi_model import assert_equal, declining_stream, edge_boundaries, model, stream_with_a_frame_at, with_boundaries
from test_syslen_cpu import CORPORA, wrap

UTF8_PIECES = [b"a", b"\xc3\xa9", b"\xe2\x82\xac", b"\xf0\x9f\x98\x80", b"\x80", b"\xc0", b"\xe0\x80", b"\xed\xa0\x80", b"\xf4\x90", b"\xff", b"\xe2",
               b"\xf0\x9f"]  # (test_syslen_cpu.py's alphabet of the UTF-8 rule)


@pytest.fixture(scope="module")
def host():
    return SyslenMultiHost()


def check(host, buf, seg_starts, may_decline=False):
    m = model(buf, seg_starts, host.max_prefix)
    r = host.frame(buf, seg_starts)
    if r["declined"]:
        assert may_decline, "the device logic declined"
        return None, m
    assert_equal(r, m)
    return r, m


def deal(msgs, n_conn, rng, nl=True):
    """the messages dealt round-robin onto n_conn connections, every connection's stream cut into chunks at random places:
    -> (buffer, seg_starts) with one segment per chunk"""
    pieces = []
    for k in range(n_conn):
        stream = wrap(msgs[k::n_conn], nl)
        cuts = sorted(int(x) for x in rng.integers(0, len(stream) + 1, int(rng.integers(0, 4))))
        pieces += [stream[a:b] for a, b in zip([0] + cuts, cuts + [len(stream)])]
    starts = [0]
    for p in pieces:
        starts.append(starts[-1] + len(p))
    return b"".join(pieces), starts


@pytest.mark.parametrize("n_conn", [1, 7, 64])
@pytest.mark.parametrize("name", sorted(CORPORA))
def test_synth_corpora_on_many_connections_are_framed_exactly_and_never_decline(host, name, n_conn):
    rng = np.random.default_rng(n_conn)
    buf, starts = deal(CORPORA[name](), n_conn, rng)
    check(host, buf, starts)  # (may_decline = False: zero declines is a condition)


SHORT = wrap([b"<13>1 - h a 1 m - hi", b"", b"gr\xc3\xbc\xc3\x9fe", b"0 1 "], nl=False) + b"12 abc"


def test_one_stream_cut_in_two_at_every_offset(host):
    """every way to cut a prefix and a payload; both neighbours' verdicts are the model's (and are looked at here)"""
    seen = set()
    for cut in range(len(SHORT) + 1):
        r, m = check(host, SHORT, [0, cut, len(SHORT)])
        seen.add((int(r["seg_stop"][0]), int(r["seg_stop"][1])))
        assert r["seg_stop"][0] in (CLEAN, TAIL)  # a prefix of a well-formed stream
        assert r["seg_consumed"][0] <= cut and r["seg_consumed"][1] <= len(SHORT) - cut
    assert {(CLEAN, TAIL), (TAIL, BAD_LEN), (TAIL, CLEAN)} <= seen


def test_every_boundary_list_of_a_short_stream(host):
    rng = np.random.default_rng(11)
    for _ in range(60):
        cuts = rng.integers(0, len(SHORT) + 1, int(rng.integers(1, 9)))
        check(host, SHORT, with_boundaries(len(SHORT), cuts) if rng.integers(0, 2) else [0] + sorted(int(c) for c in cuts) + [len(SHORT)])


def test_boundaries_at_tile_edges_a_six_tile_segment_and_forty_segments_in_one_tile(host):
    msgs = [ln if isinstance(ln, bytes) else ln.encode() for ln in CORPORA["cfg2"]()]
    buf = stream_with_a_frame_at(msgs, 8 * host.tile + 1)
    assert len(buf) >= 19 * host.tile
    starts = with_boundaries(len(buf), edge_boundaries(len(buf), host.tile))
    r, m = check(host, buf, starts)
    k = starts.index(8 * host.tile + 1)
    assert starts[k + 1] - starts[k] >= 6 * host.tile and r["seg_first"][k + 1] - r["seg_first"][k] > 100  # a chain through six tiles
    assert sum(1 for a, b in zip(starts, starts[1:]) if a == b) >= 3 and sum(1 for a, b in zip(starts, starts[1:]) if b - a == 1) >= 3
    assert len([s for s in starts if s // host.tile == 16]) >= 40 > host.inbox


def test_forty_connections_of_a_hundred_bytes_in_one_tile_do_not_decline(host):
    chunk = wrap([b"<13>1 - h a 1 m - " + b"x" * 70], nl=False)
    assert 90 <= len(chunk) <= 100
    buf = chunk * 40
    assert len(buf) < host.tile
    r, m = check(host, buf, [len(chunk) * k for k in range(41)])
    assert r["n"] == 40 and list(r["seg_stop"]) == [CLEAN] * 40


def test_nbytes_a_multiple_of_the_tile(host):
    for tiles in (1, 2, 3):
        msgs = [b"y" * 300] * 200
        buf = wrap(msgs, nl=False)[:tiles * host.tile - 5]
        buf += b"3 ab"[:4] + b"c"
        assert len(buf) == tiles * host.tile
        check(host, buf, [0, len(buf)])
        check(host, buf, [0, host.tile // 2, len(buf), len(buf)])
        check(host, buf, [0, len(buf) - 1, len(buf)])


def test_empty_and_one_byte_segments(host):
    buf = b"3 abc" + b"7" + b" " + b"x" + b"2 ok"
    check(host, buf, [0, 0, 5, 5, 6, 7, 8, 8, 12, 12])
    check(host, b"5", [0, 1])
    check(host, b"", [0, 0, 0])


def test_digits_at_a_segment_end_do_not_continue_in_the_next_segment(host):
    buf = b"3 abc" + b"12" + b" hello world!" + b"2 ok"
    r, m = check(host, buf, [0, 7, 20, len(buf)])
    assert list(r["seg_stop"]) == [TAIL, BAD_LEN, CLEAN] and list(r["seg_consumed"]) == [5, 0, 4]
    r, m = check(host, b"1" + b"2 ab", [0, 1, 5])  # "12 ab" across the boundary: TAIL, then "2 ab" on its own
    assert list(r["seg_stop"]) == [TAIL, CLEAN] and r["n"] == 1


def test_a_payload_whose_length_points_into_the_next_segment_is_a_tail(host):
    buf = b"2 ok" + b"10 abcd" + b"5 hello" + b"2 ok"
    r, m = check(host, buf, [0, 11, len(buf)])
    assert list(r["seg_stop"]) == [TAIL, CLEAN] and list(r["seg_consumed"]) == [4, 11] and list(r["seg_first"]) == [0, 1, 3]
    # ... also where the frame would end exactly on the NEXT segment's end, and across a tile end
    pad = wrap([b"p" * 500] * 8, nl=False)
    buf = pad + b"600 " + b"q" * 90 + b"3 abc" + b"z" * 505
    check(host, buf, [0, len(pad) + 94, len(buf)])


def test_a_utf8_sequence_cut_at_a_payload_end_that_is_a_segment_end(host):
    r, m = check(host, b"5 abc\xe2\x82" + b"\xac2 ok", [0, 7, 12])  # the buffer holds the sequence's last byte: not this payload's
    assert list(r["bad"]) == [1] and list(r["seg_stop"]) == [CLEAN, BAD_LEN]
    r, m = check(host, b"3 a\xe2\x82" + b"3 \xacxy", [0, 5, 10])  # the next payload starts with a continuation byte
    assert list(r["bad"]) == [1, 1] and list(r["seg_stop"]) == [CLEAN, CLEAN]
    r, m = check(host, b"3 a\xe2\x82" + b"1 a" + b"4 \xf0\x9f\x98\x80", [0, 8, 14])
    assert list(r["bad"]) == [1, 0, 0]


def five_stops(host):
    segs = [wrap([b"clean one", b"clean two"]), b"2 ok" + b"123", wrap([b"before"]) + b"2 ok" + b"50 short", b"3 abc" + b"x7 no", wrap([b"intact"]),
            b"1 a" + b"0" * (host.max_prefix + 2) + b"1 b", wrap([b"intact too", b"caf\xc3\xa9", b"bad \xff"])]
    starts = [0]
    for s in segs:
        starts.append(starts[-1] + len(s))
    return b"".join(segs), starts


def test_all_stop_reasons_in_one_run_with_intact_neighbours(host):
    buf, starts = five_stops(host)
    r, m = check(host, buf, starts)
    assert list(r["seg_stop"]) == [CLEAN, TAIL, TAIL, BAD_LEN, CLEAN, LONG_PREFIX, CLEAN]
    assert list(np.diff(r["seg_first"])) == [2, 1, 2, 1, 1, 1, 3]


def test_random_sweep(host):
    rng = np.random.default_rng(2024)
    letters = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz <>-=[]\"\n\t", np.uint8)
    declined = 0
    for case in range(300):
        msgs = []
        for _ in range(int(rng.integers(1, 60))):
            n = int(rng.integers(0, 1000)) if rng.integers(0, 4) else int(rng.integers(0, 12))
            body = letters[rng.integers(0, len(letters), n)].tobytes()
            if rng.integers(0, 5) == 0:
                body = body[:n // 2] + b"".join(UTF8_PIECES[k] for k in rng.integers(0, len(UTF8_PIECES), 3)) + body[n // 2:]
            msgs.append(body[:999])
        buf = wrap(msgs, nl=False)
        if rng.integers(0, 6) == 0:
            buf += [b"17", b"x", b" ", b"5 ab", b"0" * 30 + b" "][int(rng.integers(0, 5))]
        k = int(rng.integers(1, 51))
        starts = [0] + sorted(int(x) for x in rng.integers(0, len(buf) + 1, k - 1)) + [len(buf)]
        r, m = check(host, buf, starts, may_decline=True)
        declined += r is None
    assert declined == 0  # (a condition: payloads without digits give the resolve stage nothing to speculate on)


def test_a_declining_stream_among_clean_segments_declines(host):
    clean = wrap([b"<13>1 - h a 1 m - fine"] * 30)
    bad = declining_stream()
    buf = clean + bad + clean
    starts = [0, len(clean), len(clean) + len(bad), len(buf)]
    assert host.frame(buf, starts)["declined"] != 0
    assert model(buf, starts)["seg_stop"] == [CLEAN, CLEAN, CLEAN]  # (the segments themselves are fine: the caller hops them on the host)


@pytest.mark.parametrize("name", ["cfg2", "gelf"])
def test_one_segment_equals_the_single_stream_framer(host, name):
    one = SyslenHost()
    for buf in (wrap(CORPORA[name]()), wrap(CORPORA[name]())[:-7], wrap(CORPORA[name]()[:50]) + b"x1 ", five_stops(host)[0]):
        a, r = one.frame(buf), host.frame(buf, [0, len(buf)])
        assert not a["declined"] and not r["declined"]
        n = a["n"]
        assert (r["n"], int(r["seg_consumed"][0]), int(r["seg_stop"][0]), r["total"]) == (n, a["consumed"], a["stop"], a["total"])
        assert list(r["offsets"]) == list(a["offsets"]) and list(r["starts"]) == list(a["starts"][:n]) and list(r["bad"]) == list(a["bad"])
        assert bytes(r["packed"][:a["total"]]) == bytes(a["packed"][:a["total"]])


def test_capacity_overflow_reports_the_need_and_writes_nothing(host):
    buf, starts = five_stops(host)
    need = model(buf, starts)["n"]
    for cap in (0, 1, need - 1):
        r = host.frame(buf, starts, cap=cap)  # (the binding checks the guard entries of every output array)
        assert r["overflow"] and r["n"] == need
    r = host.frame(buf, starts, cap=need)
    assert not r["overflow"]
    assert_equal(r, model(buf, starts))
