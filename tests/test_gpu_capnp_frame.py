"""GPU tests of Cap'n Proto stream framing on the device (flowgger_amd/csrc/fg_capnp_frame.hip / fg_capnp_frame.hpp;
fg_frame_capnp_device and FG_FRAME_CAPNP in fg_frame_decode_batch / fg_transcode_batch) against CapnpFramer.frame -- the walk of
capnp::serialize::read_message as CapnpSplitter::run calls it (splitter/capnp_splitter.rs:24-46) -- and the host-framed route:
the same messages through decode_packed / Pipeline.run_packed."""
from __future__ import annotations

import ctypes as C
import struct

import numpy as np
import pytest

import capnp_frame_binding as B
import capnp_wire as W
from capnp_frame_binding import CLEAN, TAIL, TOO_LARGE, TOO_MANY_SEGMENTS, model
from flowgger_amd import CapnpDecoder, CapnpSplitter, CapnpStreamError, RFC5424Decoder
from flowgger_amd import _lib as L
from flowgger_amd.encoder import GelfEncoder, Pipeline
from flowgger_amd.record import Record, SDValue, StructuredData
from flowgger_amd.tables import DeviceTables, HostTables

pytestmark = pytest.mark.gpu
TILE_WORDS = 512  # fg::capnpf::kTileWords (the CPU suite asks the core itself)


@pytest.fixture(scope="module")
def dec():
    return CapnpDecoder()


@pytest.fixture(scope="module")
def messages():
    """about 2 K messages of the record schema, sizes from a few words to past a tile"""
    rng = np.random.default_rng(7)
    out = []
    for i in range(2000):
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


def frame_on_device(dec, raw, final=True, cap=None):
    import torch

    dev = torch.device("cuda", dec.device)
    d_bytes = to_dev(raw, dev)
    d_offs, n, consumed, stop = dec.frame_capnp_device(d_bytes, final, cap)
    torch.cuda.synchronize(dev)
    return d_bytes, d_offs, n, consumed, stop


def assert_frames(dec, raw, final=True):
    offs, consumed, stop = model(raw)
    d_bytes, d_offs, n, got_consumed, got_stop = frame_on_device(dec, raw, final)
    assert (n, got_consumed, got_stop) == (len(offs) - 1, consumed, stop)
    assert [int(x) for x in d_offs.cpu().numpy()] == offs
    return d_bytes, d_offs, n


def test_shapes_equal_the_model_for_final_0_and_1(dec):
    want = {"empty": CLEAN, "512_segments_behind_good": TOO_MANY_SEGMENTS, "sum_8mi_words_is_a_tail": TAIL,
            "sum_8mi_plus_1_is_too_large": TOO_LARGE, "tail_inside_the_table": TAIL, "tail_inside_the_body": TAIL, "511_segments": CLEAN}
    for name, raw in B.shapes(TILE_WORDS).items():
        for final in (True, False):
            assert_frames(dec, raw, final)
        if name in want:
            assert model(raw)[2] == want[name], name


def test_seeded_fuzz_with_cuts(dec):
    rng = np.random.default_rng(20261018)
    stream = B.fuzz_stream(rng, 600)
    assert len(stream) < 600 << 10
    assert_frames(dec, stream)
    for _ in range(4):
        assert_frames(dec, stream[:int(rng.integers(0, len(stream) + 1))], final=False)


def test_cap_frames_too_small_then_retry(dec):
    raw = B.msg(0) * 700 + B.msg(600) + B.msg(3) * 5
    offs, consumed, stop = model(raw)
    with pytest.raises(L.FgError) as e:
        frame_on_device(dec, raw, cap=10)
    assert e.value.code == L.FG_ERR_ENT_OVERFLOW
    import torch
    dev = torch.device("cuda", dec.device)
    d_bytes = to_dev(raw, dev)
    d_offs = torch.empty(11, dtype=torch.int64, device=dev)
    n, cons, st = C.c_uint64(), C.c_uint64(), C.c_int()
    rc = L.lib().fg_frame_capnp_device(dec._ctx, d_bytes.data_ptr(), len(raw), 1, d_offs.data_ptr(), 10, C.byref(n), C.byref(cons), C.byref(st), None)
    assert rc == L.FG_ERR_ENT_OVERFLOW and n.value == 706 == len(offs) - 1     # the need
    d_bytes, d_offs, k, got_consumed, got_stop = frame_on_device(dec, raw, cap=706)
    assert (k, got_consumed, got_stop) == (706, consumed, stop) and [int(x) for x in d_offs.cpu().numpy()] == offs


def test_frame_then_decode_equals_decode_packed_of_host_framed_input(dec, messages):
    import torch

    raw = b"".join(messages)
    d_bytes, d_offs, n = assert_frames(dec, raw)
    assert n == len(messages)
    tables = DeviceTables(n, len(raw) // 8 + 1024, d_bytes.device)
    dec.decode_frames_device(d_bytes, d_offs, n, tables, L.FG_FRAME_NONE)
    torch.cuda.synchronize(d_bytes.device)
    data = np.frombuffer(raw + bytes(32), np.uint8)
    offs = np.array(model(raw)[0], np.uint64)
    # (compared through the canonical serialisation of every row: the slices of the entry table may lie in any order)
    got = tables.to_host().serialize(L.FG_CAPNP, data, offs)
    want = dec.decode_packed(data, offs).serialize(L.FG_CAPNP, data, offs)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


def call_frame_decode_batch(dec, ptr, nbytes, final, framing=L.FG_FRAME_CAPNP):
    st = L.fg_tables()
    off = C.c_void_p()
    n, used = C.c_uint64(), C.c_uint64()
    L.check(L.lib().fg_frame_decode_batch(dec._ctx, dec.fmt, framing, ptr, nbytes, int(final), C.byref(st), C.byref(off), C.byref(n),
                                          C.byref(used)), "fg_frame_decode_batch")
    k = int(n.value)
    offs = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), (k + 1,)).copy() if k else np.zeros(1, np.uint64)
    return (HostTables.from_struct(st) if k else None), offs, int(used.value)


class Pinned:
    def __init__(self, raw):
        self.p = C.c_void_p()
        L.check(L.lib().fg_alloc_pinned(len(raw) + 32, C.byref(self.p)), "fg_alloc_pinned")
        C.memset(self.p, 0, len(raw) + 32)
        C.memmove(self.p, raw, len(raw))

    def __del__(self):
        L.lib().fg_free_pinned(self.p)


def feed_in_chunks(dec, raw, cuts, pinned):
    """the stream in chunks with carry-over -> (canonical blobs of all rows, messages, last stop, paths taken)"""
    blobs, carry, frames, paths = [], b"", 0, set()
    for k in range(len(cuts) - 1):
        chunk = carry + raw[cuts[k]:cuts[k + 1]]
        final = k + 2 == len(cuts)
        if pinned:
            pin = Pinned(chunk)
            tab, offs, consumed = call_frame_decode_batch(dec, pin.p, len(chunk), final)
        else:
            tab, offs, consumed = dec.frame_decode_batch(chunk, L.FG_FRAME_CAPNP, final)
        paths.add(dec.last_host_path())
        moffs, mconsumed, mstop = model(chunk)
        assert consumed == mconsumed and dec.last_capnp_stop() == mstop
        assert [int(x) for x in offs] == moffs
        if tab is not None:
            data, o = np.frombuffer(chunk + bytes(32), np.uint8), np.array(moffs, np.uint64)
            got = tab.serialize(L.FG_CAPNP, data, o)
            want = dec.decode_packed(data, o).serialize(L.FG_CAPNP, data, o)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
            blobs.append(got[0].tobytes())
            frames += tab.n
        carry = chunk[consumed:]
    return b"".join(blobs), frames, dec.last_capnp_stop(), paths


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_frame_decode_batch_equals_the_host_framed_route(dec, messages, pinned):
    raw = b"".join(messages)
    whole, frames, stop, paths = feed_in_chunks(dec, raw, [0, len(raw)], pinned)
    assert frames == len(messages) and stop == CLEAN and paths == {L.FG_PATH_FRAME_CAPNP_DEVICE}
    cuts = [0, len(raw) // 3 + 1, len(raw) // 3 + 3, 2 * len(raw) // 3, len(raw)]   # (odd cuts: inside a table, inside a body)
    parts, frames2, stop2, paths2 = feed_in_chunks(dec, raw, cuts, pinned)
    assert parts == whole and frames2 == len(messages) and stop2 == CLEAN and paths2 == {L.FG_PATH_FRAME_CAPNP_DEVICE}


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_run_stream_equals_the_host_framed_route(dec, messages, pinned):
    pipe = Pipeline(dec, GelfEncoder(None, merger="line"))
    raw = b"".join(messages[:1200])
    carry = b""
    cuts = [0, len(raw) // 2 + 5, len(raw)]
    for k in range(2):
        chunk = carry + raw[cuts[k]:cuts[k + 1]]
        if pinned:
            pin = Pinned(chunk)
            data = np.ctypeslib.as_array(C.cast(pin.p, C.POINTER(C.c_uint8)), (len(chunk),))
            res = pipe.run_stream(data, L.FG_FRAME_CAPNP, final=k == 1, now_ts=2.5)
        else:
            res = pipe.run_stream(chunk, L.FG_FRAME_CAPNP, final=k == 1, now_ts=2.5)
        assert dec.last_host_path() == L.FG_PATH_FRAME_CAPNP_DEVICE
        moffs, consumed, stop = model(chunk)
        want = pipe.run_packed(np.frombuffer(chunk + bytes(32), np.uint8), np.array(moffs, np.uint64), now_ts=2.5)
        assert res.consumed == consumed and dec.last_capnp_stop() == stop and res.n == want.n == len(moffs) - 1
        assert [int(x) for x in res.frame_offsets] == moffs
        assert np.array_equal(res.out, want.out) and np.array_equal(res.out_offsets, want.out_offsets)
        assert np.array_equal(res.meta, want.meta) and np.array_equal(res.enc_status, want.enc_status)
        carry = chunk[consumed:]
    assert carry == b""


def test_a_declining_stream_takes_the_host_walk_with_identical_results(dec):
    import torch

    raw = B.node_heavy_stream()
    with pytest.raises(L.FgError) as e:
        dec.frame_capnp_device(to_dev(raw, torch.device("cuda", dec.device)))
    assert e.value.code == L.FG_ERR_UNSUPPORTED
    _, frames, stop, paths = feed_in_chunks(dec, raw, [0, len(raw)], False)
    assert frames == 3 and stop == CLEAN and paths == {L.FG_PATH_FRAME_CAPNP_HOST}
    pipe = Pipeline(dec, GelfEncoder(None, merger="line"))
    res = pipe.run_stream(raw, L.FG_FRAME_CAPNP, now_ts=2.5)
    assert dec.last_host_path() == L.FG_PATH_FRAME_CAPNP_HOST
    moffs, consumed, stop = model(raw)
    want = pipe.run_packed(np.frombuffer(raw + bytes(32), np.uint8), np.array(moffs, np.uint64), now_ts=2.5)
    assert np.array_equal(res.out, want.out) and [int(x) for x in res.frame_offsets] == moffs and np.array_equal(res.meta, want.meta)


def splitter_outcome(splitter, chunks):
    """everything a caller of feed() sees: the Records per call, then the error that ended the connection"""
    out = []
    for c in chunks:
        try:
            out.append([str(r) for r in splitter.feed(c)])
        except CapnpStreamError as e:
            out.append(("error", str(e)))
            break
    return out


def test_the_gpu_framing_splitter_equals_the_host_framed_one(messages):
    good = b"".join(messages[:300])
    stream = good + struct.pack("<2I", 511, 0) + bytes(64)                # ends in a 512-segment table
    first = len(messages[0])
    cuts = [0, 3, first + 2, first + 4 + 20, len(good) // 2 + 1, len(good) - 5, len(good) + 4, len(stream)]   # inside tables and bodies
    chunks = [stream[a:b] for a, b in zip(cuts, cuts[1:])] + [b""]
    want = splitter_outcome(CapnpSplitter(), chunks)
    got = splitter_outcome(CapnpSplitter(gpu_framing=True), chunks)
    assert got == want
    assert want[-1] == ("error", "Too many segments: 512") and sum(len(x) for x in want[:-1]) == 300
    # nothing whole in front of the bad table: raised at once, on both routes
    for gpu in (False, True):
        with pytest.raises(CapnpStreamError):
            CapnpSplitter(gpu_framing=gpu).feed(struct.pack("<2I", 0, (8 << 20) + 1))


def test_what_is_refused(dec):
    raw = B.msg(3)
    st, off = L.fg_tables(), C.c_void_p()
    n, used = C.c_uint64(), C.c_uint64()
    other = RFC5424Decoder()
    buf = np.frombuffer(raw + bytes(32), np.uint8)
    rc = L.lib().fg_frame_decode_batch(other._ctx, L.FG_RFC5424, L.FG_FRAME_CAPNP, buf.ctypes.data, len(raw), 1, C.byref(st), C.byref(off),
                                       C.byref(n), C.byref(used))
    assert rc == L.FG_ERR_ARG
    with pytest.raises(L.FgError) as e:
        Pipeline(other, GelfEncoder(None, merger="line")).run_stream(raw, L.FG_FRAME_CAPNP)
    assert e.value.code == L.FG_ERR_ARG
    for framing in (L.FG_FRAME_LINE, L.FG_FRAME_NUL, L.FG_FRAME_SYSLEN):  # (a capnp stream has its own framing only)
        rc = L.lib().fg_frame_decode_batch(dec._ctx, L.FG_CAPNP, framing, buf.ctypes.data, len(raw), 1, C.byref(st), C.byref(off), C.byref(n),
                                           C.byref(used))
        assert rc == L.FG_ERR_ARG
    import torch
    d = to_dev(raw + bytes(16), torch.device("cuda", dec.device))
    with pytest.raises(L.FgError) as e:  # a chunk that does not start at a 16-byte aligned address
        dec.frame_capnp_device(d[8:])
    assert e.value.code == L.FG_ERR_ARG
