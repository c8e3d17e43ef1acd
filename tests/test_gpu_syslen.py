"""GPU tests of octet-counted ("syslen") framing on the device (flowgger_amd/csrc/fg_syslen.hip / fg_syslen.hpp; fg_frame_syslen_device and
FG_FRAME_SYSLEN in fg_frame_decode_batch / fg_transcode_batch) against the sequential walk -- read_msglen + read_exact of
src/flowgger/splitter/syslen_splitter.rs:17-57, restated in syslen_binding.py -- and the host-hop route: the hopped messages
through decode_packed / Pipeline.run_packed."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from flowgger_amd import GelfDecoder, LTSVDecoder, RFC5424Decoder, synth
from flowgger_amd import _lib as L
from flowgger_amd.encoder import GelfEncoder, Pipeline
from flowgger_amd.tables import DeviceTables, HostTables
from syslen_binding import BAD_LEN, CLEAN, TAIL, valid_utf8, walk

pytestmark = pytest.mark.gpu
RFC5424, LTSV, GELF = 0, 1, 2


def make_decoder(fmt):
    if fmt == RFC5424:
        return RFC5424Decoder()
    if fmt == LTSV:
        return LTSVDecoder(synth.LTSV_CONFIG)
    return GelfDecoder()


def corpus(fmt, n):
    if fmt == RFC5424:
        return synth.rfc5424_lines(n, cfg=2)
    if fmt == LTSV:
        return synth.ltsv_lines(n)
    return synth.gelf_lines(n)


def as_bytes(ln):
    return ln if isinstance(ln, bytes) else ln.encode()


def wrap(msgs, nl=True):
    return b"".join(b"%d %s" % (len(m) + (1 if nl else 0), m + (b"\n" if nl else b"")) for m in map(as_bytes, msgs))


def declining_stream():
    """a message whose body is a long list of distinct numbers across a tile end: every "1234 " is a candidate that leaves its tile
    somewhere else -- more exits than the kernels track"""
    body = b" ".join(b"%d" % i for i in range(1000, 1900))
    msgs = [b"<13>1 2024-01-02T03:04:05Z h a 1 m - first", body] + [b"<13>1 2024-01-02T03:04:05Z h a 1 m - filler %d " % i + b"x" * 200 for i in range(40)]
    return wrap(msgs)


def hop(raw):
    """the host hop: -> (packed payloads uint8 (padded), offsets uint64[n + 1], starts, consumed, stop, bad flags)"""
    starts, plens, lens, consumed, stop = walk(raw)
    payloads = [raw[s + p:s + p + n] for s, p, n in zip(starts, plens, lens)]
    offs = np.zeros(len(payloads) + 1, np.uint64)
    offs[1:] = np.cumsum([len(p) for p in payloads], dtype=np.uint64) if payloads else []
    packed = np.frombuffer(b"".join(payloads) + bytes(32), np.uint8)
    return packed, offs, np.array(starts + [consumed], np.uint64), consumed, stop, np.array([0 if valid_utf8(p) else 1 for p in payloads], np.uint8)


def to_dev(raw, dev):
    import torch

    buf = np.zeros((len(raw) + 15) // 16 * 16 + 16, np.uint8)
    buf[:len(raw)] = np.frombuffer(raw, np.uint8)
    return torch.from_numpy(buf).to(dev)[:len(raw)]


def frame_on_device(dec, raw, final=True):
    import torch

    dev = torch.device("cuda", dec.device)
    d_packed, d_offs, d_starts, d_bad, n, consumed, stop = dec.frame_syslen_device(to_dev(raw, dev), final)
    torch.cuda.synchronize(dev)
    return d_packed, d_offs, d_starts, d_bad, n, consumed, stop


def assert_frames(dec, raw, final=True):
    packed, offs, starts, consumed, stop, bad = hop(raw)
    d_packed, d_offs, d_starts, d_bad, n, got_consumed, got_stop = frame_on_device(dec, raw, final)
    assert (n, got_consumed, got_stop) == (len(offs) - 1, consumed, stop)
    assert np.array_equal(d_offs.cpu().numpy().astype(np.uint64), offs)
    assert np.array_equal(d_starts.cpu().numpy().astype(np.uint64), starts)
    assert np.array_equal(d_bad.cpu().numpy(), bad)
    total = int(offs[-1])
    assert np.array_equal(d_packed[:total].cpu().numpy(), packed[:total])
    return d_packed, d_offs, d_bad, n, (packed, offs)


@pytest.mark.parametrize("fmt", [RFC5424, LTSV, GELF], ids=["rfc5424", "ltsv", "gelf"])
@pytest.mark.parametrize("nl", [True, False], ids=["nl", "bare"])
def test_frame_syslen_device_equals_the_host_walk_and_decodes_like_the_hopped_messages(fmt, nl):
    import torch

    dec = make_decoder(fmt)
    raw = wrap(corpus(fmt, 3000), nl)
    d_packed, d_offs, d_bad, n, (packed, offs) = assert_frames(dec, raw)
    assert n == 3000
    dev = d_packed.device
    tables = DeviceTables(n, len(raw) // 8 + 1024, dev)
    dec.decode_frames_device(d_packed[:int(offs[-1])], d_offs, n, tables, L.FG_FRAME_NONE, d_bad)
    torch.cuda.synchronize(dev)
    got = tables.to_host().serialize(fmt, packed, offs, cfg=dec._cfg)
    want = dec.decode_packed(packed, offs).serialize(fmt, packed, offs, cfg=dec._cfg)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


def test_long_frames_empty_frames_and_prefix_lookalikes():
    dec = RFC5424Decoder()
    msgs = [b"x" * 20000, b"", b"", b"12 34 56 7 8 9 10 11 300 ", b"+5 005 ", b"y" * 4096, b""] * 5 + [b"7 " * 3000]
    assert_frames(dec, wrap(msgs, nl=False))
    assert_frames(dec, b"0 " * 20000)
    assert_frames(dec, b"+3 abc003 def")


def test_round_trip_of_the_syslen_merger():
    """our own FG_MERGE_SYSLEN output, framed where it lies: the payloads are the encoder's messages, "\\n" included"""
    import torch

    dec = RFC5424Decoder()
    lines = [as_bytes(ln) for ln in synth.rfc5424_lines(2000, cfg=4, sd=True)]
    data, offsets = synth.pack(lines)
    dev = torch.device("cuda", dec.device)
    d_bytes = to_dev(bytes(data[:int(offsets[-1])]), dev)
    d_offsets = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    n = len(lines)
    tables = DeviceTables(n, len(data) // 8 + 1024, dev)
    dec.decode_device(d_bytes, d_offsets, tables)
    d_sys, _ = GelfEncoder(None, merger="syslen").encode_device(dec, d_bytes, d_offsets, n, tables, now_ts=1.5)
    d_line, d_line_off = GelfEncoder(None, merger="line").encode_device(dec, d_bytes, d_offsets, n, tables, now_ts=1.5)
    torch.cuda.synchronize(dev)
    line_off = d_line_off.cpu().numpy()
    kept = np.flatnonzero(line_off[1:] > line_off[:-1])  # (a line whose decode failed produces nothing, not an empty frame)
    stream = torch.zeros((d_sys.numel() + 15) // 16 * 16 + 16, dtype=torch.uint8, device=dev)
    stream[:d_sys.numel()] = d_sys
    d_packed, d_offs, d_starts, d_bad, k, consumed, stop = dec.frame_syslen_device(stream[:d_sys.numel()])
    torch.cuda.synchronize(dev)
    assert (k, consumed, stop) == (len(kept), d_sys.numel(), CLEAN)
    assert np.array_equal(d_packed[:d_line.numel()].cpu().numpy(), d_line.cpu().numpy())
    assert np.array_equal(d_offs.cpu().numpy(), np.concatenate([line_off[kept], line_off[-1:]]))
    assert not d_bad.cpu().numpy().any()


def call_frame_decode_batch(dec, ptr, nbytes, final):
    st, off = L.fg_tables(), C.c_void_p()
    n, used = C.c_uint64(), C.c_uint64()
    L.check(L.lib().fg_frame_decode_batch(dec._ctx, dec.fmt, L.FG_FRAME_SYSLEN, ptr, nbytes, int(final), C.byref(st), C.byref(off), C.byref(n),
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
    """the stream in chunks with carry-over -> (canonical blobs of all rows, frame count, last stop reason, paths taken)"""
    blobs, carry, frames, paths = [], b"", 0, set()
    for k in range(len(cuts) - 1):
        chunk = carry + raw[cuts[k]:cuts[k + 1]]
        final = k + 2 == len(cuts)
        if pinned:
            pin = Pinned(chunk)
            tab, offs, consumed = call_frame_decode_batch(dec, pin.p, len(chunk), final)
        else:
            tab, offs, consumed = dec.frame_decode_batch(chunk, L.FG_FRAME_SYSLEN, final)
        paths.add(L.lib().fg_last_host_path(dec._ctx))
        packed, poffs, starts, hconsumed, hstop, bad = hop(chunk)
        assert consumed == hconsumed and dec.last_syslen_stop() == hstop
        assert np.array_equal(offs, starts)
        if tab is not None:
            assert tab.n == len(poffs) - 1
            got = tab.serialize(dec.fmt, packed, poffs, cfg=dec._cfg)
            want = dec.decode_packed(packed, poffs).serialize(dec.fmt, packed, poffs, cfg=dec._cfg)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])
            blobs.append(got[0].tobytes())
            frames += tab.n
        carry = chunk[consumed:]
    return b"".join(blobs), frames, dec.last_syslen_stop(), paths


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
@pytest.mark.parametrize("fmt", [RFC5424, LTSV, GELF], ids=["rfc5424", "ltsv", "gelf"])
def test_frame_decode_batch_syslen_equals_the_host_hop_route(fmt, pinned):
    dec = make_decoder(fmt)
    msgs = [as_bytes(m) for m in corpus(fmt, 4000)]
    raw = wrap(msgs)
    whole, frames, stop, paths = feed_in_chunks(dec, raw, [0, len(raw)], pinned)
    assert frames == 4000 and stop == CLEAN and paths == {L.FG_PATH_FRAME_SYSLEN_DEVICE}
    cuts = [0, len(raw) // 3 + 1, len(raw) // 3 + 3, 2 * len(raw) // 3, len(raw)]
    parts, frames2, stop2, paths2 = feed_in_chunks(dec, raw, cuts, pinned)
    assert parts == whole and frames2 == 4000 and stop2 == CLEAN and paths2 == {L.FG_PATH_FRAME_SYSLEN_DEVICE}


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_transcode_syslen_equals_the_host_hop_route(pinned):
    dec = RFC5424Decoder()
    pipe = Pipeline(dec, GelfEncoder(None, merger="syslen"))
    raw = wrap([as_bytes(m) for m in synth.rfc5424_lines(3000, cfg=4, sd=True)])
    carry, outs, want_outs = b"", [], []
    cuts = [0, len(raw) // 2 + 5, len(raw)]
    for k in range(2):
        chunk = carry + raw[cuts[k]:cuts[k + 1]]
        if pinned:
            pin = Pinned(chunk)
            data = np.ctypeslib.as_array(C.cast(pin.p, C.POINTER(C.c_uint8)), (len(chunk),))
            res = pipe.run_stream(data, L.FG_FRAME_SYSLEN, final=k == 1, now_ts=2.5)
        else:
            res = pipe.run_stream(chunk, L.FG_FRAME_SYSLEN, final=k == 1, now_ts=2.5)
        assert L.lib().fg_last_host_path(dec._ctx) == L.FG_PATH_FRAME_SYSLEN_DEVICE
        packed, poffs, starts, consumed, stop, bad = hop(chunk)
        want = pipe.run_packed(packed, poffs, now_ts=2.5)
        assert res.consumed == consumed and dec.last_syslen_stop() == stop and res.n == want.n
        assert np.array_equal(res.frame_offsets, starts)
        assert np.array_equal(res.out, want.out) and np.array_equal(res.out_offsets, want.out_offsets)
        assert np.array_equal(res.meta, want.meta) and np.array_equal(res.enc_status, want.enc_status)
        carry = chunk[consumed:]
    assert carry == b""


def test_a_declining_stream_takes_the_host_hop_with_identical_results():
    import torch

    dec = RFC5424Decoder()
    raw = declining_stream()
    with pytest.raises(L.FgError) as e:
        dec.frame_syslen_device(to_dev(raw, torch.device("cuda", dec.device)))
    assert e.value.code == L.FG_ERR_UNSUPPORTED
    _, frames, stop, paths = feed_in_chunks(dec, raw, [0, len(raw)], False)
    assert frames == 42 and stop == CLEAN and paths == {L.FG_PATH_FRAME_SYSLEN_HOST}
    pipe = Pipeline(dec, GelfEncoder(None, merger="line"))
    res = pipe.run_stream(raw, L.FG_FRAME_SYSLEN, now_ts=2.5)
    assert L.lib().fg_last_host_path(dec._ctx) == L.FG_PATH_FRAME_SYSLEN_HOST
    packed, poffs, starts, consumed, stop, bad = hop(raw)
    want = pipe.run_packed(packed, poffs, now_ts=2.5)
    assert np.array_equal(res.out, want.out) and np.array_equal(res.frame_offsets, starts) and np.array_equal(res.meta, want.meta)


def test_stop_reasons():
    dec = RFC5424Decoder()
    good = wrap([as_bytes(m) for m in synth.rfc5424_lines(300, cfg=2)])
    for tail, stop in ((b"", CLEAN), (b"12", TAIL), (b"+", TAIL), (b"50 <13>1 2024", TAIL), (b" 5 hello", BAD_LEN), (b"5x hello", BAD_LEN),
                       (b"+ abc", BAD_LEN), (b"-1 a", BAD_LEN), (b"18446744073709551616 a", BAD_LEN), (b"18446744073709551615 a", TAIL)):
        more = wrap([b"<13>1 2024-01-02T03:04:05Z h a 1 m - never reached"])
        raw = good + tail + (more if stop == BAD_LEN else b"")
        for final in (True, False):
            d_packed, d_offs, d_bad, n, _ = assert_frames(dec, raw, final)
            assert n == 300
        tab, offs, consumed = dec.frame_decode_batch(raw, L.FG_FRAME_SYSLEN, False)
        assert tab.n == 300 and consumed == len(good) and dec.last_syslen_stop() == stop  # rows before it, nothing after it
    # a prefix longer than the device parser reads: the entry points hop it on the host
    raw = good + b"0" * 40 + b"3 abc" + good
    tab, offs, consumed = dec.frame_decode_batch(raw, L.FG_FRAME_SYSLEN, True)
    assert tab.n == 601 and consumed == len(raw) and dec.last_syslen_stop() == CLEAN
    assert L.lib().fg_last_host_path(dec._ctx) == L.FG_PATH_FRAME_SYSLEN_HOST


def test_invalid_utf8_flags_only_its_own_frame():
    dec = RFC5424Decoder()
    msgs = [as_bytes(m) for m in synth.rfc5424_lines(200, cfg=2, invalid_frac=0.0)]
    for i, damage in ((17, b"\xff"), (50, b"\xc3"), (51, b"\xe2\x82"), (120, b"\xf0\x9f\x98"), (199, b"\xe2")):
        msgs[i] = msgs[i] + b" caf\xc3\xa9 " + damage  # (a sequence truncated at the payload's last byte: the next byte is a prefix's)
    msgs[60] = msgs[60] + " grüße €".encode()
    raw = wrap(msgs, nl=False)
    d_packed, d_offs, d_bad, n, _ = assert_frames(dec, raw)
    assert list(np.flatnonzero(d_bad.cpu().numpy())) == [17, 50, 51, 120, 199]
    tab, offs, consumed = dec.frame_decode_batch(raw, L.FG_FRAME_SYSLEN, True)
    st = tab.a["meta"] & 0xFF
    assert list(np.flatnonzero(st == 0xFD)) == [17, 50, 51, 120, 199] and consumed == len(raw)
