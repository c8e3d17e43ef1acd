"""The Kafka message-set core (flowgger_amd/csrc/fg_kafka.hpp) compiled for the CPU, a wave being 64 fibers, in the order the kernels of
fg_kafka.hip run it (tests/native/kafka_host.cpp), byte for byte against the plain-Python wire format of tests/kafka_wire.py."""
import zlib

import numpy as np
import pytest

import deflate_model as dm
import kafka_model as km
import kafka_wire as kw


@pytest.fixture(scope="module")
def host():
    return km.KafkaHost()


def gzip_member(data):
    c = zlib.compressobj(6, zlib.DEFLATED, 31)
    return c.compress(data) + c.flush()


def check_set(host, values, skip, what):
    got = host.messageset(values, skip)
    assert got is not None, what
    s, so = got
    assert so.tolist() == kw.set_offsets(values, skip), what
    want = kw.message_set(values, skip)
    if bytes(s) != want:  # (name the first message that differs: the whole sets do not fit a report)
        for i, v in enumerate(values):
            a, b = int(so[i]), int(so[i + 1])
            assert bytes(s[a:b]) == (b"" if skip is not None and skip[i] else kw.message(v)), f"{what}: row {i}, {len(v)} value bytes, set offset {a}"
    assert bytes(s) == want, what
    n = len(values)
    assert len(s) <= host.bound(sum(map(len, values)), n, max(1, n)), what
    return s, so


def test_the_wire_reference_against_a_hand_built_message():
    """the reference itself: one message spelt out byte by byte, and its parser"""
    m = kw.message(b"hi")
    body = bytes([0, 0, 0xFF, 0xFF, 0xFF, 0xFF, 0, 0, 0, 2]) + b"hi"
    assert m == bytes(8) + bytes([0, 0, 0, 16]) + zlib.crc32(body).to_bytes(4, "big") + body and len(m) == kw.OVERHEAD + 2
    assert kw.parse_set(m + kw.message(b"")) == [(True, 0, b"hi"), (True, 0, b"")]
    bad = bytearray(m)
    bad[-1] ^= 1
    assert kw.parse_set(bytes(bad)) == [(False, 0, b"h" + bytes([ord("i") ^ 1]))]
    assert kw.records(kw.wrapper(gzip_member(m))) == [(True, b"hi")]
    with pytest.raises(ValueError):
        kw.parse_set(m[:-1])


@pytest.mark.parametrize("align", range(16))
def test_every_length_at_every_source_alignment(host, align):
    """row 0 shifts the source; skipped or not it shifts the destination too"""
    values = km.alignment_batch(align)
    n = len(values)
    for skip in (None, [True] + [False] * (n - 1)):
        check_set(host, values, skip, f"align {align} skip {skip is not None}")


@pytest.mark.parametrize("align", [0, 7, 15])
def test_long_values_take_the_wave(host, align):
    values = km.alignment_batch(align, km.LENGTHS_LONG)
    check_set(host, values, None, f"long, align {align}")
    check_set(host, values, [True] + [False] * (len(values) - 1), f"long, align {align}, row 0 skipped")


def test_a_value_of_a_mebibyte_and_three(host):
    values = km.values_of([3, km.LONGEST, 40], 11)
    check_set(host, values, None, "1 MiB + 3")


@pytest.mark.parametrize("skip", km.SKIPS)
def test_skipped_rows(host, skip):
    values = km.values_of([5, 0, 300, 17, 4097, 0, 0, 64, 1, 700, 26, 255, 4096, 33, 2], 21)
    sk = km.skip_case(skip, len(values))
    s, so = check_set(host, values, sk, f"skip {skip}")
    if skip == "all":
        assert len(s) == 0 and so.tolist() == [0] * (len(values) + 1)
    for one in range(len(values)):  # n = 1
        check_set(host, values[one:one + 1], None if sk is None else sk[one:one + 1], f"skip {skip}, row {one} alone")


def test_an_empty_batch(host):
    s, so = host.messageset([], None)
    assert len(s) == 0 and so.tolist() == [0]
    w, wo = host.wrap([])
    assert len(w) == 0 and wo.tolist() == [0]


def test_refused_offsets(host):
    blob, off = km.pack([b"abc", b"defg"])
    assert host.messageset_raw(blob, 7, np.array([0, 5, 3, 7], np.uint64), None) is None
    assert host.messageset_raw(blob, 7, np.array([0, 3, 8], np.uint64), None) is None
    assert host.messageset_raw(blob, 2**33, np.array([0, 2**31 - 26], np.uint64), None) is None  # (the message would not fit int32)
    assert host.wrap_raw(blob, np.array([0, 5, 3], np.uint64)) is None


def test_two_runs_give_the_same_bytes(host):
    values = km.alignment_batch(3)
    a, b = host.messageset(values), host.messageset(values)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    m = km.wrap_members()
    a, b = host.wrap(m), host.wrap(m)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_wrappers(host):
    members = km.wrap_members()
    w, wo = host.wrap(members)
    assert bytes(w) == km.expect_wrapped(members)
    assert wo.tolist() == np.cumsum([0] + [kw.OVERHEAD + len(m) if m else 0 for m in members]).tolist()
    msgs = kw.parse_set(bytes(w))
    assert [m[2] for m in msgs] == [m for m in members if m] and all(ok and attr == kw.ATTR_GZIP for ok, attr, _ in msgs)
    for m, (a, b) in zip(members, zip(wo[:-1], wo[1:])):  # the CRC field itself, against zlib
        if m:
            head = bytes(w[int(a):int(a) + kw.OVERHEAD])
            assert int.from_bytes(head[12:16], "big") == zlib.crc32(head[16:] + m)
    assert len(w) <= host.bound(sum(map(len, members)), 0, len(members))
    w1, _ = host.wrap([b"", b"", b""])
    assert len(w1) == 0


@pytest.mark.parametrize("coalesce,member_bytes", [(1, 0), (4, 0), (0, 700)])
def test_members_through_the_compressor(host, coalesce, member_bytes):
    """the whole chain on the emulation: set, member cuts, deflate, wrap.  One message a member (coalesce 1), a partial last member
    (11 rows by 4), and a member whose rows are all skipped between two that are not"""
    dh = dm.DeflateHost()
    values = km.values_of([50, 0, 300, 17, 90, 61, 5, 260, 1, 700, 26], 31)
    values = [bytes(b"k=v "[i % 4] for i in range(len(v))) if k % 2 else v for k, v in enumerate(values)]
    skip = [False] * len(values)
    for i in (4, 5, 6, 7):  # rows 4 .. 7: the whole of member 1 of coalesce 4
        skip[i] = True
    skip[1 if coalesce == 1 else 9] = True
    s, so = check_set(host, values, skip, "members")
    off = np.cumsum([0] + [len(v) for v in values]).astype(np.uint64)
    first, _ = dm.model_members(off, coalesce, member_bytes, dh.block)
    cuts = host.cuts(so, first)
    assert cuts.tolist() == [int(so[int(i)]) for i in first]
    blob = km.aligned(len(s))
    blob[:len(s)] = s
    z, zoff = dh.deflate_raw(blob, len(s), cuts)
    w, wo = host.wrap_raw(np.ascontiguousarray(z), zoff)
    zs = dm.split(z, zoff)
    assert bytes(w) == km.expect_wrapped(zs)
    nm = len(first) - 1
    assert len(w) <= host.bound(int(off[-1]), len(values), nm)
    empty = 0
    for k in range(nm):
        rows = range(int(first[k]), int(first[k + 1]))
        member = bytes(w[int(wo[k]):int(wo[k + 1])])
        want = [values[i] for i in rows if not skip[i]]
        if not want:
            assert member == b""
            empty += 1
        else:
            assert kw.records(member) == [(True, v) for v in want], k
    if coalesce == 4:
        assert nm == 3 and empty == 1 and int(first[-1]) - int(first[-2]) == 3  # (a partial last member; the middle one all skipped)
