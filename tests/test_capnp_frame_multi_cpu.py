"""CPU: the SEGMENTED Cap'n Proto framer's device logic (flowgger_amd/csrc/fg_capnp_frame_multi.hpp: the chunks of many connections in
one launch) on the wave emulation, against CapnpFramer.frame of every segment (capnp_frame_multi_model.py)."""
from __future__ import annotations

import struct

import numpy as np
import pytest

import capnp_frame_binding as B
from capnp_frame_binding import CLEAN, TAIL, TOO_LARGE, TOO_MANY_SEGMENTS, CapnpFrameHost
from capnp_frame_multi_binding import CapnpFrameMultiHost
from capnp_frame_multi_model import CARRY, FRAME, assert_equal, model, with_boundaries
from syslen_multi_model import edge_boundaries


@pytest.fixture(scope="module")
def host():
    return CapnpFrameMultiHost()


@pytest.fixture(scope="module")
def single():
    return CapnpFrameHost()


def check(host, buf, seg_starts, may_decline=False):
    m = model(buf, seg_starts)
    r = host.frame(buf, seg_starts)
    if r["declined"]:
        assert may_decline, "the device logic declined"
        return None, m
    assert not r["overflow"]
    assert_equal(r, m)
    return r, m


def same_as_single(host, single, buf):
    s = single.frame(buf)
    r = host.frame(buf, [0, len(buf)])
    assert s["declined"] == 0 and r["declined"] == 0
    frames = [int(o) for o, k in zip(r["offsets"], r["kind"]) if k == FRAME]
    assert frames == [int(x) for x in s["offsets"][:s["n"]]]
    assert (int(r["seg_consumed"][0]), int(r["seg_stop"][0])) == (s["consumed"], s["stop"])
    assert list(r["kind"]).count(CARRY) == (1 if s["consumed"] < len(buf) else 0)
    assert int(r["offsets"][-1]) == len(buf)


def test_one_segment_is_the_single_stream_framer_on_the_shapes(host, single):
    for name, buf in B.shapes(host.tile_words).items():
        same_as_single(host, single, buf)


def test_one_segment_is_the_single_stream_framer_on_every_cut_of_a_small_stream(host, single):
    stream = B.msg(0) + B.msg(2, 1, fill=b"ab") + B.msg(7, fill=struct.pack("<2I", 0, 1)) + B.msg(1, 0, 2) + B.msg(0)
    for cut in range(len(stream) + 1):
        same_as_single(host, single, stream[:cut])
        check(host, stream[:cut], [0, cut])


def mixed_stream(tile_words, tiles=3):
    """8-byte and multi-word messages, bodies that read as small messages themselves, a little more than `tiles` tiles"""
    rng = np.random.default_rng(7)
    fills = [b"\0", struct.pack("<2I", 0, 1), struct.pack("<2I", 0, 3), b"text"]
    parts, n = [], 0
    while n < tiles * tile_words * 8 + 40:
        m = B.msg(0) if rng.random() < 0.6 else B.msg(int(rng.integers(1, 90)), fill=fills[int(rng.integers(0, 4))])
        parts.append(m)
        n += len(m)
    return b"".join(parts)


def test_a_boundary_at_every_word_of_a_three_tile_stream(host):
    t = host.tile_words
    buf = mixed_stream(t)[:3 * t * 8 + 24]
    stops = set()
    for w in range(1, len(buf) // 8):
        r, m = check(host, buf, [0, 8 * w, len(buf)])
        stops.add(m["seg_stop"][0])
    assert stops == {CLEAN, TAIL}
    for w in (t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1):  # two boundaries round a tile's edge, an empty segment between them
        check(host, buf, [0, 8 * w, 8 * w, 8 * w + 8, len(buf)])


def test_a_message_that_ends_exactly_on_a_segment_end_counts_and_ends_clean(host):
    t = host.tile_words
    a = B.msg(3, fill=b"a") + B.msg(40, fill=b"b")                   # ends mid-tile
    b = B.msg(t - len(a) // 8 - 1 - 100, fill=b"c") + B.msg(99, fill=b"d")  # ends on the tile's edge
    c = B.msg(5, fill=b"e") + B.msg(0)
    buf = a + b + c
    assert len(a + b) == t * 8
    r, m = check(host, buf, [0, len(a), len(a) + len(b), len(buf)])
    assert m["seg_stop"] == [CLEAN, CLEAN, CLEAN] and m["seg_first"] == [0, 2, 4, 6] and CARRY not in m["kind"]
    assert [int(x) for x in r["seg_consumed"]] == [len(a), len(b), len(c)]


def test_a_body_or_a_table_that_reaches_into_the_next_segment_is_a_tail(host):
    small = B.msg(2, fill=b"s")
    body = small + B.msg(10, fill=b"x")            # the boundary cuts the body; the bytes are there
    r, m = check(host, body + small, [0, len(body) - 16, len(body) + len(small)])
    assert m["seg_stop"][0] == TAIL and m["seg_consumed"][0] == len(small) and m["kind"][:2] == [FRAME, CARRY]
    table = small + B.msg(*([1] * 9), fill=b"t")   # the boundary cuts the table of ten words' sizes
    r, m = check(host, table + small, [0, len(small) + 16, len(table) + len(small)])
    assert m["seg_stop"][0] == TAIL and m["seg_consumed"][0] == len(small)


def test_a_body_word_that_reads_as_a_message_landing_in_the_next_segment_changes_nothing_there(host):
    t = host.tile_words
    # segment 0: one message whose body words are tables "1 segment of 600 + j words": each reaches far into segment 1's tiles
    body = b"".join(struct.pack("<2I", 0, 600 + j) for j in range(40))
    seg0 = B.msg(3, fill=b"p") + struct.pack("<2I", 0, 40) + body
    seg1 = b"".join(B.msg(k % 7, fill=b"q") for k in range(400))
    assert len(seg1) > 2 * t * 8
    r, m = check(host, seg0 + seg1, [0, len(seg0), len(seg0) + len(seg1)])
    alone = model(seg1, [0, len(seg1)])
    assert [o - len(seg0) for o in m["offsets"][m["seg_first"][1]:]] == alone["offsets"]
    assert m["seg_stop"] == [CLEAN, CLEAN]


def test_512_segments_of_one_8_byte_message_each_in_one_tile(host):
    t = host.tile_words
    buf = B.msg(0) * t
    r, m = check(host, buf, [8 * k for k in range(t)] + [len(buf)])
    assert r["n"] == t and m["seg_stop"] == [CLEAN] * t and m["seg_first"] == list(range(t + 1))


def test_empty_segments(host):
    buf = B.msg(4, fill=b"a") + B.msg(0) + B.msg(9, fill=b"b")
    at = len(B.msg(4))
    r, m = check(host, buf, [0] + [at] * 41 + [len(buf)])                     # 40 empty segments in a row
    assert m["seg_stop"] == [CLEAN] * 42 and m["seg_consumed"][1:41] == [0] * 40
    r, m = check(host, buf, [0, 0, at, len(buf), len(buf)])                   # an empty first and an empty last segment
    assert m["seg_first"] == [0, 0, 1, 3, 3]
    check(host, b"", [0, 0, 0])
    check(host, buf, [0, 0, 0, len(buf)])


@pytest.mark.parametrize("bad, stop", [(struct.pack("<2I", 511, 0) + bytes(64), TOO_MANY_SEGMENTS),
                                       (struct.pack("<4I", 1, B.MAX_WORDS - 5, 6, 0) + bytes(64), TOO_LARGE)])
def test_a_stop_in_a_middle_segment_leaves_its_neighbours_alone(host, bad, stop):
    left = b"".join(B.msg(k % 5, fill=b"l") for k in range(30))
    mid = B.msg(3, fill=b"m") + B.msg(0) + bad
    right = b"".join(B.msg(k % 9, fill=b"r") for k in range(200))
    r, m = check(host, left + mid + right, [0, len(left), len(left + mid), len(left + mid + right)])
    assert m["seg_stop"] == [CLEAN, stop, CLEAN]
    a, b = m["seg_first"][1], m["seg_first"][2]
    assert m["kind"][a:b] == [FRAME, FRAME, CARRY]
    assert m["offsets"][b - 1] == len(left) + m["seg_consumed"][1] and m["offsets"][b] == len(left + mid)


def test_a_last_segment_that_ends_off_a_word(host):
    buf = B.msg(2, fill=b"a") + B.msg(1, fill=b"b") + B.msg(3, fill=b"c")[:-3]
    r, m = check(host, buf, [0, len(B.msg(2)), len(buf)])
    assert len(buf) % 8 == 5 and m["seg_stop"] == [CLEAN, TAIL]
    assert m["kind"][-1] == CARRY and m["offsets"][-1] == len(buf)
    for k in range(1, 8):
        r, m = check(host, B.msg(1) + bytes(k), [0, 16, 16 + k])
        assert m["seg_stop"] == [CLEAN, TAIL]


def test_cap_slots_one_too_small_reports_the_need_and_writes_nothing(host):
    buf = B.msg(0) * 700 + B.msg(600) + B.msg(3) * 5 + B.msg(7)[:-8]
    starts = [0, 800, 5608, len(buf)]
    full, m = check(host, buf, starts)
    r = host.frame(buf, starts, cap=full["n"] - 1)   # (the binding checks that every output still holds its guard values)
    assert not r["declined"] and r["overflow"] and r["n"] == full["n"]
    r = host.frame(buf, starts, cap=full["n"])
    assert_equal(r, m)


def test_a_misaligned_start_is_rounded_down_and_a_disordered_list_is_clamped(host):
    buf = B.msg(0) * 6
    r, m = check(host, buf, [0, 21, len(buf)])
    assert m["seg_first"] == [0, 2, 6]
    r, m = check(host, buf, [0, 5, 3, len(buf)])            # -> 0, 0, 0
    assert m["seg_first"] == [0, 0, 0, 6]
    r, m = check(host, buf, [7, 1 << 40, 16, 1 << 63])      # -> 0, 48, 48 | 48
    assert m["seg_first"] == [0, 6, 6, 6]


def test_a_node_heavy_segment_declines(host):
    heavy = B.node_heavy_stream()
    small = B.msg(5, fill=b"abcdefgh") * 3
    buf = small + heavy + small
    starts = [0, len(small), len(small + heavy), len(buf)]
    r = host.frame(buf, starts)
    assert r["declined"] and r["nodes"] > host.node_cap(len(buf), 3)


def test_seeded_fuzz_never_declines(host):
    rng = np.random.default_rng(20261020)
    for _ in range(12):
        stream = B.fuzz_stream(rng, 300)
        for n_cuts in (1, 7, 60):
            cuts = rng.integers(1, len(stream) // 8, n_cuts) * 8
            check(host, stream, with_boundaries(len(stream), cuts))  # (may_decline = False: zero declines is a condition)
        check(host, stream, with_boundaries(len(stream), edge_boundaries(len(stream))))  # (asserts 18 tiles or more)
