"""GPU: Kafka v0 message sets (fg_kafka.hip) -- fg_kafka_messageset_device and fg_kafka_wrap_device against the plain-Python wire format
of tests/kafka_wire.py and, byte for byte, against the same core on the wave emulation (tests/kafka_model.py); Pipeline(wire="kafka")
through every transcode entry point against the same call with wire="raw"; the wrappers' values back through the project's own inflater."""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import pytest

import deflate_model as dm
import kafka_model as km
import kafka_wire as kw
from flowgger_amd import Encoder, GelfDecoder, GelfEncoder, Pipeline, RFC5424Decoder, synth
from flowgger_amd import _lib as L

pytestmark = pytest.mark.gpu
NOW = 1_700_000_000.0


@pytest.fixture(scope="module")
def dec():
    d = GelfDecoder()
    yield d
    d.close()


@pytest.fixture(scope="module")
def host():
    return km.KafkaHost()


@pytest.fixture(scope="module")
def block():
    return int(L.lib().fg_deflate_block_bytes())


def gpu_set(dec, values, skip=None, out=None):
    import torch

    dev = torch.device("cuda", dec.device)
    blob, off = km.pack(values)
    d_bytes = torch.from_numpy(blob[:int(off[-1])].copy()).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_skip = None if skip is None else torch.from_numpy(km.skip_array(skip, len(values))).to(dev)
    d_set, d_soff = Encoder.kafka_messageset_device(dec, d_bytes, d_off, d_skip, out=out)
    torch.cuda.synchronize(dev)
    return d_set.cpu().numpy(), d_soff.cpu().numpy().astype(np.uint64)


def gpu_wrap(dec, members):
    import torch

    dev = torch.device("cuda", dec.device)
    z, zo = km.pack(members)
    d_z = torch.from_numpy(z[:int(zo[-1])].copy()).to(dev)
    d_w, d_woff = Encoder.kafka_wrap_device(dec, d_z, torch.from_numpy(zo.astype(np.int64)).to(dev))
    torch.cuda.synchronize(dev)
    return d_w.cpu().numpy(), d_woff.cpu().numpy().astype(np.uint64)


def test_overhead_and_bound(host):
    assert int(L.lib().fg_kafka_message_overhead()) == kw.OVERHEAD
    for nbytes, n, nm in ((0, 0, 0), (1, 1, 1), (5000, 7, 2), (1 << 30, 1 << 22, 1 << 14)):
        assert int(L.lib().fg_kafka_bound(nbytes, n, nm)) == host.bound(nbytes, n, nm) >= nbytes + 26 * n + 44 * nm


@pytest.fixture(scope="module")
def case_list(host):
    """the CPU suite's cases as one batch: every length behind every source alignment (the pad row of the odd alignments skipped, which
    moves the destinations), the long values that take the whole wave, and the longest"""
    values, skip = [], []
    for align in range(16):
        v = km.alignment_batch(align)
        values += v
        skip += [align % 2 == 1] + [False] * (len(v) - 1)
    v = km.alignment_batch(7, km.LENGTHS_LONG) + km.values_of([km.LONGEST, 3], 11)
    values += v
    skip += [False] * len(v)
    skip[-1] = True
    s, so = host.messageset(values, skip)
    return values, skip, s, so


def test_case_list_equals_the_wire_format_and_the_emulation(dec, case_list):
    values, skip, hs, hso = case_list
    s, so = gpu_set(dec, values, skip)
    assert so.tolist() == kw.set_offsets(values, skip) == hso.tolist()
    if not np.array_equal(s, hs):
        for i, v in enumerate(values):
            a, b = int(so[i]), int(so[i + 1])
            assert bytes(s[a:b]) == (b"" if skip[i] else kw.message(v)), f"row {i}, {len(v)} value bytes, set offset {a}"
    assert np.array_equal(s, hs) and bytes(s) == kw.message_set(values, skip)
    assert len(s) <= int(L.lib().fg_kafka_bound(sum(map(len, values)), len(values), 1))
    s2, so2 = gpu_set(dec, values, skip)  # the same input again: the same bytes
    assert np.array_equal(s, s2) and np.array_equal(so, so2)


@pytest.mark.parametrize("skip", km.SKIPS)
def test_skipped_rows_one_row_and_none(dec, skip):
    values = km.values_of([5, 0, 300, 17, 4097, 0, 0, 64, 1, 700, 26, 255, 4096, 33, 2], 21)
    sk = km.skip_case(skip, len(values))
    s, so = gpu_set(dec, values, sk)
    assert bytes(s) == kw.message_set(values, sk) and so.tolist() == kw.set_offsets(values, sk)
    for one in (0, 4, 5):  # n = 1
        s, so = gpu_set(dec, values[one:one + 1], None if sk is None else sk[one:one + 1])
        assert bytes(s) == kw.message_set(values[one:one + 1], None if sk is None else sk[one:one + 1])
    s, so = gpu_set(dec, [])  # n = 0
    assert len(s) == 0 and so.tolist() == [0]


def test_sizing_call_exact_capacity_and_overflow(dec):
    import torch

    dev = torch.device("cuda", dec.device)
    values = [b"\n".join(synth.gelf_lines(20)), b"", bytes(range(256)) * 10, b"q" * 700]
    skip = np.array([0, 0, 1, 0], np.uint8)
    blob, off = km.pack(values)
    n, nbytes = len(values), int(off[-1])
    d_bytes = torch.from_numpy(blob[:nbytes].copy()).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_skip = torch.from_numpy(skip).to(dev)
    d_soff = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    total = C.c_uint64()
    lib = L.lib()
    head = (dec._ctx, d_bytes.data_ptr(), nbytes, d_off.data_ptr(), d_skip.data_ptr(), n)
    tail = (d_soff.data_ptr(), C.byref(total), None)
    assert lib.fg_kafka_messageset_device(*head, None, 0, *tail) == L.FG_OK
    need = int(total.value)
    want = kw.message_set(values, skip)
    assert need == len(want) and d_soff.cpu().numpy().tolist() == kw.set_offsets(values, skip)
    d_set = torch.full((need + 64,), 0xEE, dtype=torch.uint8, device=dev)
    assert lib.fg_kafka_messageset_device(*head, d_set.data_ptr(), need - 1, *tail) == L.FG_ERR_ENT_OVERFLOW and int(total.value) == need
    torch.cuda.synchronize(dev)
    assert bool((d_set == 0xEE).all()), "an overflowing call wrote message bytes"
    assert lib.fg_kafka_messageset_device(*head, d_set.data_ptr(), need, *tail) == L.FG_OK and int(total.value) == need
    torch.cuda.synchronize(dev)
    out = d_set.cpu().numpy()
    assert bool((out[need:] == 0xEE).all()), "bytes written behind the last message"
    assert bytes(out[:need]) == want
    for bad in ([0, 10, 5, nbytes, nbytes], [0, 10, 10, 10, nbytes + 1]):
        d_bad = torch.tensor(bad, dtype=torch.int64, device=dev)
        assert lib.fg_kafka_messageset_device(dec._ctx, d_bytes.data_ptr(), nbytes, d_bad.data_ptr(), None, n, None, 0, *tail) == L.FG_ERR_ARG
    assert lib.fg_kafka_messageset_device(None, *head[1:], None, 0, *tail) == L.FG_ERR_ARG
    # the wrappers, in the same way
    members = [b"z" * 300, b"", bytes(range(256)) * 70]
    z, zo = km.pack(members)
    d_z = torch.from_numpy(z[:int(zo[-1])].copy()).to(dev)
    d_zo = torch.from_numpy(zo.astype(np.int64)).to(dev)
    d_wo = torch.zeros(len(members) + 1, dtype=torch.int64, device=dev)
    whead = (dec._ctx, d_z.data_ptr(), d_zo.data_ptr(), len(members))
    wtail = (d_wo.data_ptr(), C.byref(total), None)
    assert lib.fg_kafka_wrap_device(*whead, None, 0, *wtail) == L.FG_OK
    need = int(total.value)
    want = km.expect_wrapped(members)
    assert need == len(want)
    d_w = torch.full((need + 64,), 0xEE, dtype=torch.uint8, device=dev)
    assert lib.fg_kafka_wrap_device(*whead, d_w.data_ptr(), need - 1, *wtail) == L.FG_ERR_ENT_OVERFLOW and int(total.value) == need
    torch.cuda.synchronize(dev)
    assert bool((d_w == 0xEE).all()), "an overflowing call wrote wrapper bytes"
    assert lib.fg_kafka_wrap_device(*whead, d_w.data_ptr(), need, *wtail) == L.FG_OK
    torch.cuda.synchronize(dev)
    out = d_w.cpu().numpy()
    assert bool((out[need:] == 0xEE).all()) and bytes(out[:need]) == want
    d_down = torch.tensor([0, 9, 5], dtype=torch.int64, device=dev)
    assert lib.fg_kafka_wrap_device(dec._ctx, d_z.data_ptr(), d_down.data_ptr(), 2, None, 0, *wtail) == L.FG_ERR_ARG


def test_wrappers_equal_the_wire_format_and_the_emulation(dec, host):
    members = km.wrap_members()
    w, wo = gpu_wrap(dec, members)
    hw, hwo = host.wrap(members)
    assert np.array_equal(w, hw) and np.array_equal(wo, hwo) and bytes(w) == km.expect_wrapped(members)
    for m, a in zip(members, wo[:-1]):  # the CRC field itself, against zlib
        if m:
            head = bytes(w[int(a):int(a) + kw.OVERHEAD])
            assert int.from_bytes(head[12:16], "big") == zlib.crc32(head[16:] + m)


def test_many_more_members_than_waves(dec, host):
    """2000 small random members: a piece each, and the same members as values, 500 steps of the write kernel.  The grids are 24 waves a
    CU, so on a part of up to 83 CUs (20 for the write kernel) waves take further work grid-stride; on a larger part every wave has one
    piece or step and what this holds is the binary search for a piece's member and 2000 offsets at once"""
    rng = np.random.default_rng(11)
    members = [rng.integers(0, 256, int(rng.integers(1, 301)), dtype=np.uint8).tobytes() for _ in range(2000)]
    w, wo = gpu_wrap(dec, members)
    hw, hwo = host.wrap(members)
    assert np.array_equal(w, hw) and np.array_equal(wo, hwo) and bytes(w) == km.expect_wrapped(members)
    s, so = gpu_set(dec, members)
    assert bytes(s) == kw.message_set(members)
    # ... and more than the grids of a 256-CU part hold (6 144 waves): 28 000 values, 7 000 steps; 7 000 members, a piece each
    many = [rng.integers(0, 256, int(rng.integers(0, 90)), dtype=np.uint8).tobytes() for _ in range(28_000)]
    skip = [i % 11 == 3 for i in range(len(many))]
    s, so = gpu_set(dec, many, skip)
    assert bytes(s) == kw.message_set(many, skip) and so.tolist() == kw.set_offsets(many, skip)
    w, wo = gpu_wrap(dec, many[:7000])
    assert bytes(w) == km.expect_wrapped(many[:7000])


def test_one_member_of_five_pieces_and_seven_bytes(dec, host):
    member = km.values_of([5 * km.PIECE + 7], 3)[0]
    w, wo = gpu_wrap(dec, [member])
    hw, hwo = host.wrap([member])
    assert np.array_equal(w, hw) and bytes(w) == kw.wrapper(member) and wo.tolist() == [0, kw.OVERHEAD + len(member)]


# ---- Pipeline(wire="kafka") -----------------------------------------------------------------------------------------------------------
CORPORA = {"rfc5424": (RFC5424Decoder, lambda: synth.rfc5424_lines(3000, cfg=2)), "gelf": (GelfDecoder, lambda: synth.gelf_lines(3000))}
POLICIES = [(1, 0), (7, 0), (4096, 0), (0, 0), (0, 4096)]


def runs(p, lines):
    """the four entry shapes over one corpus: name -> result"""
    data, offsets = synth.pack(lines)
    stream = b"\n".join(lines)  # (an unterminated tail)
    thirds = [b"\n".join(lines[k::3]) + (b"\n" if k != 1 else b"") for k in range(3)]
    starts = np.cumsum([0] + [len(t) for t in thirds]).astype(np.uint64)
    return {"packed": p.run_packed(data, offsets, now_ts=NOW),
            "stream": p.run_stream(stream, L.FG_FRAME_LINE, final=True, now_ts=NOW),
            "multi": p.run_multi(b"".join(thirds), starts, [0, 1, 0], L.FG_FRAME_LINE, now_ts=NOW),
            "datagrams": p.run_datagrams([zlib.compress(x) if i % 3 == 0 else x for i, x in enumerate(lines)], now_ts=NOW)}


@pytest.fixture(scope="module")
def plain():
    out = {}
    for name, (make, corpus) in CORPORA.items():
        d = make()
        try:
            lines = corpus()
            out[name] = (lines, runs(Pipeline(d, GelfEncoder(None, merger="line")), lines))
        finally:
            d.close()
    return out


@pytest.mark.parametrize("coalesce,member_bytes", POLICIES)
@pytest.mark.parametrize("compression", [None, "gzip"])
@pytest.mark.parametrize("corpus", sorted(CORPORA))
def test_pipeline_message_sets_carry_the_plain_messages(plain, block, corpus, compression, coalesce, member_bytes):
    lines, want = plain[corpus]
    d = CORPORA[corpus][0]()
    try:
        enc = GelfEncoder(None, merger="line")
        got = runs(Pipeline(d, enc, compression=compression, coalesce=coalesce, member_bytes=member_bytes, wire="kafka"), lines)
        for shape, t in got.items():
            w = want[shape]
            tag = f"{corpus} {shape} {compression} coalesce={coalesce} member_bytes={member_bytes}"
            assert w.out is not None and w.out.size > 100_000 and w.z is None and w.wire == "raw", tag
            assert t.out is None and t.wire == "kafka" and t.raw_bytes == w.out.size, tag
            assert np.array_equal(t.out_offsets, w.out_offsets) and np.array_equal(t.meta, w.meta) and np.array_equal(t.enc_status, w.enc_status), tag
            failed = t.enc_status != 0
            assert int(failed.sum()) >= 10, tag  # (the corpus' invalid lines: in no set)
            first, _ = dm.model_members(w.out_offsets, coalesce, member_bytes, block)
            assert np.array_equal(t.member_first, first), tag
            zo = t.z_offsets.astype(np.int64)
            assert len(zo) == len(first) and zo[0] == 0 and zo[-1] == t.z.size and (np.diff(zo) >= 0).all(), tag
            assert t.z.size <= int(L.lib().fg_kafka_bound(w.out.size, w.n, len(first) - 1)), tag
            members, recs = t.members(), t.kafka_records()
            for k, (member, rec) in enumerate(zip(members, recs)):
                rows = [i for i in range(int(first[k]), int(first[k + 1])) if not failed[i]]
                assert rec == [(True, w.message(i)) for i in rows], (tag, k)  # every CRC verifies; the values are the plain run's messages
                assert (member == b"") == (not rows), (tag, k)
                assert kw.records(member) == rec, (tag, k)  # (the library's parser and the tests' agree)
                if rows and compression == "gzip":
                    outer = kw.parse_set(member)
                    assert len(outer) == 1 and outer[0][1] == kw.ATTR_GZIP, (tag, k)
                elif rows:
                    assert member == kw.message_set([w.message(i) for i in rows]), (tag, k)
            assert t.messages() == [w.message(i) for i in range(w.n)], tag
            if compression == "gzip" and coalesce != 1:
                assert t.z.size < 0.8 * w.out.size, tag
        # the same ctx with wire="raw" right after: what it gave before the wire was ever set
        t = Pipeline(d, enc, compression=compression, coalesce=coalesce, member_bytes=member_bytes).run_packed(*synth.pack(lines), now_ts=NOW)
        if compression == "gzip":
            assert t.wire == "raw" and b"".join(zlib.decompress(m, 31) for m in t.members() if m) == want["packed"].out.tobytes()
        else:
            assert t.out.tobytes() == want["packed"].out.tobytes() and t.z is None
            c = L.fg_compressed()
            assert L.lib().fg_last_compressed(d._ctx, C.byref(c)) == L.FG_OK and c.n_members == 0 and c.z_bytes == 0 and not c.z
    finally:
        d.close()


def test_raw_gzip_after_kafka_equals_raw_gzip_before(plain):
    """byte for byte: the members of a wire="raw" gzip run on a ctx that has built message sets in between"""
    lines, _ = plain["gelf"]
    d = GelfDecoder()
    try:
        enc = GelfEncoder(None, merger="line")
        raw = Pipeline(d, enc, compression="gzip", coalesce=7)
        before = raw.run_packed(*synth.pack(lines), now_ts=NOW)
        Pipeline(d, enc, compression="gzip", coalesce=7, wire="kafka").run_packed(*synth.pack(lines), now_ts=NOW)
        after = raw.run_packed(*synth.pack(lines), now_ts=NOW)
        assert np.array_equal(before.z, after.z) and np.array_equal(before.z_offsets, after.z_offsets) and np.array_equal(before.member_first, after.member_first)
    finally:
        d.close()


def test_from_config_with_the_kafka_output(capfd):
    d = GelfDecoder()
    try:
        enc = GelfEncoder(None, merger="line")
        capfd.readouterr()
        p = Pipeline.from_config(d, enc, {"output": {"type": "kafka", "kafka_compression": "gzip", "kafka_coalesce": 5}})
        assert capfd.readouterr().err.splitlines() == ["Output framing is ignored with the Kafka output"]
        assert p.wire == L.FG_WIRE_KAFKA_V0 and p.compression == L.FG_COMP_GZIP and p.coalesce == 5 and enc.merger == L.FG_MERGE_LINE
        lines = synth.gelf_lines(23, invalid_frac=0)
        t = p.run_packed(*synth.pack(lines), now_ts=NOW)
        assert t.out is None and t.wire == "kafka" and len(t.members()) == 5 and t.member_first.tolist() == [0, 5, 10, 15, 20, 23]
        framed = [Pipeline(d, enc).run_packed(*synth.pack(lines), now_ts=NOW).message(i) for i in range(23)]
        assert all(m.endswith(b"\n") for m in framed) and t.messages() == [m[:-1] for m in framed]  # (without the merger's newline)
        assert all(ok for member in t.kafka_records() for ok, _ in member)
        assert capfd.readouterr().err == ""  # (said once, not per call)
        # an encoder without a merger: nothing to say; without output.type: as ever
        Pipeline.from_config(d, GelfEncoder(None), {"output": {"type": "kafka"}})
        q = Pipeline.from_config(d, enc, {"output": {"kafka_compression": "gzip"}})
        assert capfd.readouterr().err == "" and q.wire == L.FG_WIRE_RAW and q._merger is None
    finally:
        d.close()


def test_wrappers_round_trip_through_the_projects_inflater(dec, block):
    """set -> cuts -> deflate -> wrap on resident tensors; the wrappers' values through fg_udp_unpack_device come out as the inner sets"""
    import test_gpu_udp as TU
    import torch
    import udp_model as um

    dev = torch.device("cuda", dec.device)
    lines = synth.gelf_lines(600, invalid_frac=0)
    skip = [i % 37 == 5 for i in range(len(lines))]
    first = list(range(0, len(lines), 40)) + [len(lines)]
    blob, off = km.pack(lines)
    d_bytes = torch.from_numpy(blob[:int(off[-1])].copy()).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_set, d_soff = Encoder.kafka_messageset_device(dec, d_bytes, d_off, torch.from_numpy(km.skip_array(skip, len(lines))).to(dev))
    d_cuts = d_soff[torch.tensor(first, device=dev)].contiguous()
    d_z, d_zoff = Encoder.deflate_device(dec, d_set, d_cuts)
    d_w, d_woff = Encoder.kafka_wrap_device(dec, d_z, d_zoff)
    torch.cuda.synchronize(dev)
    w, wo = d_w.cpu().numpy(), d_woff.cpu().numpy()
    sets = [kw.message_set(lines[a:b], skip[a:b]) for a, b in zip(first[:-1], first[1:])]
    outer = kw.parse_set(bytes(w))
    assert len(outer) == len(sets) and all(ok and attr == kw.ATTR_GZIP for ok, attr, _ in outer)
    grams = [v for _, _, v in outer]
    assert all(24 <= len(g) <= 65527 for g in grams)
    offs, packed, drop, st = TU.unpack(dec, grams, max(map(len, sets)))
    # Every member inflated and passed its CRC-32 and ISIZE (else FG_UDP_BAD_GZIP and an empty slot).  What the UDP input then says of
    # the content is FG_UDP_BAD_UTF8: a message set is binary -- a null key is the length ff ff ff ff --, so as a datagram it would be
    # dropped; the inflated bytes are in its slot all the same, and they are the inner sets.
    assert st.tolist() == [um.BAD_UTF8] * len(sets) and drop.all()
    assert [um.model(g, max(map(len, sets))) for g in grams] == [(um.BAD_UTF8, s, False) for s in sets]
    assert [bytes(packed[int(offs[k]):int(offs[k + 1])]) for k in range(len(sets))] == sets
