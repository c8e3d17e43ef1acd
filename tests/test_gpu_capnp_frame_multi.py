"""GPU tests of Cap'n Proto framing of the chunks of MANY connections in one launch (flowgger_amd/csrc/fg_capnp_frame_multi.hip /
fg_capnp_frame_multi.hpp; fg_frame_capnp_multi_device, fg_frame_decode_capnp_multi_batch, MultiCapnpSplitter) against CapnpFramer.frame of
every segment (capnp_frame_multi_model.py: a CapnpSplitter per connection, src/flowgger/splitter/capnp_splitter.rs:24-46)."""
from __future__ import annotations

import ctypes as C
import random
import struct

import numpy as np
import pytest

import capnp_frame_binding as B
import capnp_wire as W
from capnp_frame_binding import CLEAN, TAIL, TOO_LARGE, TOO_MANY_SEGMENTS
from capnp_frame_multi_model import CARRY, FRAME, assert_equal, model, with_boundaries
from flowgger_amd import CapnpDecoder, CapnpSplitter, CapnpStreamError, FlushPolicy, MultiCapnpSplitter
from flowgger_amd import _lib as L
from flowgger_amd.decoder import pack_messages
from flowgger_amd.record import Record, SDValue, StructuredData
from flowgger_amd.tables import DeviceTables
from syslen_multi_model import edge_boundaries

pytestmark = pytest.mark.gpu
T = 512  # fg::capnpf::kTileWords (the CPU suite asks the core itself)
G8, G64 = 0xEE, -0x1111111111111112  # (0xEEEE... as int64)
GUARD = 8
COLS = ["meta", "ts", "hostname", "appname", "procid", "msgid", "msg", "full_msg", "ent_count"]


@pytest.fixture(scope="module")
def dec():
    return CapnpDecoder()


@pytest.fixture(scope="module")
def messages():
    """600 messages of the record schema, sizes from a few words to past a tile"""
    rng = np.random.default_rng(11)
    out = []
    for i in range(600):
        pairs = [(f"k{j}", SDValue("String", "v" * int(rng.integers(0, 20)))) for j in range(int(rng.integers(0, 5)))]
        full = "f" * int(rng.integers(0, 6000)) if i % 97 == 0 else None
        out.append(W.serialize(Record(ts=1.5 + i, hostname=f"host{i % 13}", appname="app", msg="m" * int(rng.integers(0, 200)), full_msg=full,
                                      facility=i % 24, severity=i % 8, sd=[StructuredData("id", pairs)] if pairs else None)))
    return out


def to_dev(raw, dev):
    import torch

    buf = np.zeros((len(raw) + 15) // 16 * 16 + 16, np.uint8)
    buf[:len(raw)] = np.frombuffer(raw, np.uint8)
    return torch.from_numpy(buf).to(dev)[:len(raw)]


def run(dec, raw, starts, cap=None):
    """fg_frame_capnp_multi_device on device arrays with guard entries behind each -> (rc, result as capnp_frame_multi_binding gives it)"""
    import torch

    dev = torch.device("cuda", dec.device)
    n, k = len(raw), len(starts) - 1
    cap = n // 8 + k if cap is None else cap
    full = lambda cnt, dt, v: torch.full((cnt + GUARD,), v, dtype=dt, device=dev)
    d_bytes = to_dev(raw, dev)
    d_starts = torch.from_numpy(np.asarray(starts, np.uint64).view(np.int64)).to(dev)
    offsets, kind = full(cap + 1, torch.int64, G64), full(cap, torch.uint8, G8)
    first, cons, stop = full(k + 1, torch.int64, G64), full(k, torch.int64, G64), full(k, torch.uint8, G8)
    ns = C.c_uint64()
    rc = L.lib().fg_frame_capnp_multi_device(dec._ctx, d_bytes.data_ptr(), n, d_starts.data_ptr(), k, offsets.data_ptr(), kind.data_ptr(), cap,
                                             first.data_ptr(), cons.data_ptr(), stop.data_ptr(), C.byref(ns),
                                             C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    offsets, kind, first, cons, stop = (t.cpu().numpy() for t in (offsets, kind, first, cons, stop))
    # nothing is ever written behind the capacities
    assert (offsets[cap + 1:] == G64).all() and (kind[cap:] == G8).all()
    assert (first[k + 1:] == G64).all() and (cons[k:] == G64).all() and (stop[k:] == G8).all()
    if rc != L.FG_OK:  # (overflow or declined: no slot output, no per-segment output)
        assert (offsets == G64).all() and (kind == G8).all() and (first == G64).all() and (cons == G64).all() and (stop == G8).all()
        return rc, {"n": int(ns.value)}
    s = int(ns.value)
    assert (offsets[s + 1:] == G64).all() and (kind[s:] == G8).all()
    return rc, {"n": s, "offsets": offsets[:s + 1], "kind": kind[:s], "seg_first": first[:k + 1], "seg_consumed": cons[:k], "seg_stop": stop[:k]}


def check(dec, raw, starts):
    rc, r = run(dec, raw, starts)
    assert rc == L.FG_OK
    m = model(raw, starts)
    assert_equal(r, m)
    return r, m


def deal(msgs, n_conn):
    """the messages dealt round-robin onto n_conn connections, one segment each -> (buffer, seg_starts)"""
    segs = [b"".join(msgs[c::n_conn]) for c in range(n_conn)]
    return b"".join(segs), [0] + [int(x) for x in np.cumsum([len(s) for s in segs])]


def test_one_segment_is_bit_identical_to_the_single_stream_framer(dec):
    import torch

    dev = torch.device("cuda", dec.device)
    rng = np.random.default_rng(5)
    whole = b"".join(B.msg(int(rng.integers(0, 40)), fill=struct.pack("<2I", 0, int(rng.integers(0, 4)))) for _ in range(3000))
    assert len(whole) < 1 << 20
    for raw in (whole, whole[:-9]):
        d_offs, n, consumed, stop = dec.frame_capnp_device(to_dev(raw, dev), True)
        torch.cuda.synchronize(dev)
        rc, r = run(dec, raw, [0, len(raw)])
        assert rc == L.FG_OK and n >= 2999
        frames = r["offsets"][:-1][r["kind"] == FRAME]
        assert np.array_equal(frames, d_offs.cpu().numpy()[:n])
        assert (int(r["seg_consumed"][0]), int(r["seg_stop"][0])) == (consumed, stop)
        assert r["n"] == n + (1 if consumed < len(raw) else 0) and int(r["offsets"][-1]) == len(raw)


def test_boundaries_round_the_tile_edges(dec):
    rng = np.random.default_rng(7)
    fills = [b"\0", struct.pack("<2I", 0, 1), struct.pack("<2I", 0, 3), b"text"]
    buf = b"".join(B.msg(0) if rng.random() < 0.6 else B.msg(int(rng.integers(1, 90)), fill=fills[int(rng.integers(0, 4))]) for _ in range(400))
    buf = buf[:3 * T * 8 + 24]
    assert len(buf) == 3 * T * 8 + 24
    for w in (T - 1, T, T + 1):
        check(dec, buf, [0, 8 * w, len(buf)])
        check(dec, buf, [0, 8 * w, 8 * w, 8 * w + 8, 8 * (T + w), len(buf)])


@pytest.mark.parametrize("n_conn", [8, 300])
def test_encoded_records_on_many_connections(dec, messages, n_conn):
    raw, starts = deal(messages, n_conn)
    r, m = check(dec, raw, starts)
    assert m["seg_stop"] == [CLEAN] * n_conn and r["n"] == len(messages)
    cut = raw[:-13]                                                  # the last connection's last message is cut, off a word
    r, m = check(dec, cut, starts[:-1] + [len(cut)])
    assert m["seg_stop"][-1] == TAIL and m["kind"][-1] == CARRY
    stream = b"".join(messages)[:20 * 4096 + 800]                    # one stream cut where the tiles meet
    check(dec, stream, with_boundaries(len(stream), edge_boundaries(len(stream))))


def test_512_one_message_segments_in_one_tile(dec):
    buf = B.msg(0) * T
    r, m = check(dec, buf, [8 * k for k in range(T)] + [len(buf)])
    assert r["n"] == T and m["seg_first"] == list(range(T + 1))
    buf = B.msg(0) * (3 * T)                                         # ... and in three tiles, with 40 empty segments among them
    check(dec, buf, sorted([8 * k for k in range(3 * T)] + [8 * 700] * 40) + [len(buf)])


@pytest.mark.parametrize("bad, stop", [(struct.pack("<2I", 511, 0) + bytes(64), TOO_MANY_SEGMENTS),
                                       (struct.pack("<4I", 1, B.MAX_WORDS - 5, 6, 0) + bytes(64), TOO_LARGE)])
def test_a_stop_in_a_middle_segment_leaves_its_neighbours_alone(dec, bad, stop):
    left = b"".join(B.msg(k % 5, fill=b"l") for k in range(300))
    mid = B.msg(3, fill=b"m") + B.msg(0) + bad
    right = b"".join(B.msg(k % 9, fill=b"r") for k in range(200))
    r, m = check(dec, left + mid + right, [0, len(left), len(left + mid), len(left + mid + right)])
    assert m["seg_stop"] == [CLEAN, stop, CLEAN]
    a, b = m["seg_first"][1], m["seg_first"][2]
    assert m["kind"][a:b] == [FRAME, FRAME, CARRY]
    # a body that reaches into the next segment, a table that does: TAIL, although the bytes are there
    small = B.msg(2, fill=b"s")
    body = small + B.msg(10, fill=b"x")
    r, m = check(dec, body + small, [0, len(body) - 16, len(body) + len(small)])
    assert m["seg_stop"][0] == TAIL


def test_overflow_writes_nothing_and_a_misaligned_list_is_rounded_and_clamped(dec):
    buf = B.msg(0) * 700 + B.msg(600) + B.msg(3) * 5 + B.msg(7)[:-8]
    starts = [0, 800, 5608, len(buf)]
    full, m = check(dec, buf, starts)
    rc, r = run(dec, buf, starts, cap=full["n"] - 1)                 # (run checks that every output still holds its guard values)
    assert rc == L.FG_ERR_ENT_OVERFLOW and r["n"] == full["n"]
    rc, r = run(dec, buf, starts, cap=full["n"])
    assert rc == L.FG_OK
    assert_equal(r, m)
    check(dec, buf, [0, 21, len(buf)])
    check(dec, buf, [0, 5, 3, len(buf)])
    check(dec, buf, [7, 1 << 40, 16, 1 << 63])


def test_a_node_heavy_segment_declines_with_the_outputs_untouched(dec):
    small = B.msg(5, fill=b"abcdefgh") * 3
    buf = small + B.node_heavy_stream() + small
    rc, r = run(dec, buf, [0, len(small), len(buf) - len(small), len(buf)])
    assert rc == L.FG_ERR_UNSUPPORTED


def col(tab, c):
    """a fixed column of a table, one row per line (a span column holds two words per line)"""
    return tab.a[c][:tab.a[c].size // tab.n * tab.n].reshape(tab.n, -1)


def assert_decode(dec, raw, starts, path):
    """frame_decode_capnp_multi: the slots are the model's, the rows of FRAME slots equal decode_packed of the same messages, CARRY rows
    are skipped"""
    m = model(raw, starts)
    tab, offsets, kind, first, cons, stop = dec.frame_decode_capnp_multi(raw, starts)
    assert dec.last_host_path() == path
    assert_equal({"n": len(kind), "offsets": offsets, "kind": kind, "seg_first": first, "seg_consumed": cons, "seg_stop": stop}, m)
    fr, ca = np.nonzero(kind == FRAME)[0], np.nonzero(kind == CARRY)[0]
    msgs = [raw[int(offsets[i]):int(offsets[i + 1])] for i in fr]
    data, offs = pack_messages(msgs)
    want = dec.decode_packed(data, offs)
    for c in COLS:
        assert np.array_equal(col(tab, c)[fr], col(want, c)), c
    for j, i in enumerate(fr):  # the entries of every message, wherever its slice of the table lies
        k = int(tab.a["ent_count"][i])
        fa, fb = int(tab.a["ent_first"][i]), int(want.a["ent_first"][j])
        for c, w in (("ent_name", 2), ("ent_val", 1), ("ent_type", 1), ("ent_flags", 1)):  # (a name is a span: two words)
            assert np.array_equal(tab.a[c][w * fa:w * (fa + k)], want.a[c][w * fb:w * (fb + k)]), (c, int(i))
    assert len(ca) and ((tab.a["meta"][ca] & 0xFF) == L.FG_ST_BAD_UTF8).all() and (tab.a["ent_count"][ca] == 0).all()
    return m


def test_frame_decode_capnp_multi_decodes_the_frames_and_skips_the_carries(dec, messages):
    segs = [b"".join(messages[c:200:20]) for c in range(20)]
    segs[3] += messages[300][:40]                                    # a cut message: a CARRY
    segs[7] += struct.pack("<2I", 511, 0) + bytes(24)                # a table that ends the connection: a CARRY
    segs[19] += messages[301][:-11]                                  # ... and one off a word at the buffer's end
    raw, starts = b"".join(segs), [0] + [int(x) for x in np.cumsum([len(s) for s in segs])]
    m = assert_decode(dec, raw, starts, L.FG_PATH_FRAME_CAPNP_MULTI_DEVICE)
    assert m["seg_stop"][3] == TAIL and m["seg_stop"][7] == TOO_MANY_SEGMENTS and m["seg_stop"][19] == TAIL
    with pytest.raises(L.FgError):                                   # the host entry checks the list
        dec.frame_decode_capnp_multi(raw, [0, 12, len(raw)])
    with pytest.raises(L.FgError):
        dec.frame_decode_capnp_multi(raw, [0, len(raw) - 8])
    # the same call with a segment the device framer declines: the host walks, equal results
    heavy = B.node_heavy_stream()
    raw2 = raw[:starts[5]] + heavy + raw[starts[5]:]
    starts2 = starts[:6] + [s + len(heavy) for s in starts[5:]]
    assert_decode(dec, raw2, starts2, L.FG_PATH_FRAME_CAPNP_MULTI_HOST)


def test_decode_frames_device_without_a_skip_array_is_unchanged(dec, messages):
    """(guards the plumbing of d_bad_utf8 through the capnp launcher)"""
    import torch

    dev = torch.device("cuda", dec.device)
    msgs = messages[:150]
    data, offs = pack_messages(msgs)
    want = dec.decode_packed(data, offs)
    d_bytes = to_dev(data.tobytes(), dev)
    d_offs = torch.from_numpy(offs.view(np.int64)).to(dev)
    tables = DeviceTables(len(msgs), 16 * len(msgs), dev)
    dec.decode_frames_device(d_bytes, d_offs, len(msgs), tables, L.FG_FRAME_NONE, None)
    torch.cuda.synchronize(dev)
    got = tables.to_host()
    for c in COLS:
        assert np.array_equal(col(got, c), col(want, c)), c
    # ... and with one: the flagged rows are skipped, the others are the same
    d_bad = torch.zeros(len(msgs), dtype=torch.uint8, device=dev)
    d_bad[::7] = 2
    tables = DeviceTables(len(msgs), 16 * len(msgs), dev)
    dec.decode_frames_device(d_bytes, d_offs, len(msgs), tables, L.FG_FRAME_NONE, d_bad)
    torch.cuda.synchronize(dev)
    got = tables.to_host()
    keep = np.arange(len(msgs)) % 7 != 0
    assert ((got.a["meta"][:len(msgs)][~keep] & 0xFF) == L.FG_ST_BAD_UTF8).all()
    for c in COLS:
        assert np.array_equal(col(got, c)[keep], col(want, c)[keep]), c


def test_multi_capnp_splitter_against_a_splitter_per_connection(dec, messages):
    rnd = random.Random(3)
    n_conn = 20
    streams = [b"".join(messages[c:400:n_conn]) for c in range(n_conn)]
    streams[4] = b"".join(messages[4:100:n_conn]) + struct.pack("<2I", 600, 0) + bytes(64)  # ends in "Too many segments"
    streams[9] = streams[9][:len(streams[9]) - 21]                                          # is closed mid-message
    want, chunks = [], []
    for c, s in enumerate(streams):
        cuts = sorted(rnd.randrange(len(s) + 1) for _ in range(rnd.randrange(2, 7)))  # random BYTE positions
        chunks.append([s[a:b] for a, b in zip([0] + cuts, cuts + [len(s)])])
        one, res = CapnpSplitter(decoder=dec, gpu_framing=False), []
        try:
            for ch in chunks[-1]:
                res += one.feed(ch)
            one.feed(b"")
        except CapnpStreamError as e:
            res.append(e)
        want.append(res)
    multi = MultiCapnpSplitter(dec, FlushPolicy(max_bytes=1 << 30, max_latency_ms=1e9))
    got = [[] for _ in range(n_conn)]
    for rnd_no in range(max(len(ch) for ch in chunks)):  # one flush per round of chunks
        for c in range(n_conn):
            ended = bool(got[c]) and isinstance(got[c][-1], CapnpStreamError)  # (the reference's thread has left its loop)
            if rnd_no < len(chunks[c]) and not ended:
                assert multi.push(c, chunks[c][rnd_no]) == []
        if rnd_no == len(chunks[9]) - 1:
            multi.close(9)
        for c, res in multi.flush():
            got[c] += res
    assert multi.pending_bytes() == 0
    for c in range(n_conn):
        assert len(got[c]) == len(want[c]), c
        for a, b in zip(got[c], want[c]):
            if isinstance(b, CapnpStreamError):
                assert isinstance(a, CapnpStreamError) and str(a) == str(b), c
            else:
                assert type(a) is type(b) and (W.record_key(a) == W.record_key(b) if isinstance(b, Record) else str(a) == str(b)), c
    assert isinstance(got[4][-1], CapnpStreamError) and str(got[4][-1]).startswith("Too many segments")
    assert not any(isinstance(x, CapnpStreamError) for x in got[9]) and len(got[9]) == len(messages[9:400:n_conn]) - 1
    for c in (4, 9):
        with pytest.raises(ValueError):
            multi.push(c, b"more")
