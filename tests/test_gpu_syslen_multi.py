"""GPU tests of octet-counted framing of the chunks of MANY connections in one launch (flowgger_amd/csrc/fg_syslen_multi.hip /
fg_syslen_multi.hpp; fg_frame_syslen_multi_device, fg_frame_decode_syslen_multi_batch, MultiSyslenSplitter) against the sequential walk
of every segment (syslen_multi_model.py: a SyslenSplitter per connection, src/flowgger/splitter/syslen_splitter.rs:10-57)."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

from flowgger_amd import FlushPolicy, GelfDecoder, LTSVDecoder, MultiSyslenSplitter, RFC5424Decoder, synth
from flowgger_amd import _lib as L
from flowgger_amd.decoder import SYSLEN_BAD_LENGTH, SYSLEN_PANIC, SYSLEN_SHORT_READ
from flowgger_amd.record import DecodeError
from syslen_binding import BAD_LEN, CLEAN, LONG_PREFIX, TAIL, VALID, read_msglen, valid_utf8
from syslen_multi_model import MAX_PREFIX, assert_equal, declining_stream, edge_boundaries, model, stream_with_a_frame_at, with_boundaries

pytestmark = pytest.mark.gpu
RFC5424, LTSV, GELF = 0, 1, 2
TILE = 4096
G8, G64 = 0xEE, -0x1111111111111112  # (0xEEEE... as int64)
GUARD = 8
RUST_WS = "\t\n\x0b\x0c\r \x85\xa0\u1680\u2000\u2001\u2002\u2003\u2004\u2005\u2006\u2007\u2008\u2009\u200a\u2028\u2029\u202f\u205f\u3000"  # char::is_whitespace


def as_bytes(ln):
    return ln if isinstance(ln, bytes) else ln.encode()


def wrap(msgs, nl=True):
    return b"".join(b"%d %s" % (len(m) + (1 if nl else 0), m + (b"\n" if nl else b"")) for m in map(as_bytes, msgs))


def make_decoder(fmt):
    return RFC5424Decoder() if fmt == RFC5424 else LTSVDecoder(synth.LTSV_CONFIG) if fmt == LTSV else GelfDecoder()


def corpus(fmt, n):
    return synth.rfc5424_lines(n, cfg=2) if fmt == RFC5424 else synth.ltsv_lines(n) if fmt == LTSV else synth.gelf_lines(n)


@pytest.fixture(scope="module")
def dec():
    return RFC5424Decoder()


def to_dev(raw, dev):
    import torch

    buf = np.zeros((len(raw) + 15) // 16 * 16 + 16, np.uint8)
    buf[:len(raw)] = np.frombuffer(raw, np.uint8)
    return torch.from_numpy(buf).to(dev)[:len(raw)]


def run(dec, raw, starts, cap=None):
    """fg_frame_syslen_multi_device on device arrays with guard entries behind each -> (rc, result as syslen_multi_binding gives it)"""
    import torch

    dev = torch.device("cuda", dec.device)
    n, k = len(raw), len(starts) - 1
    cap = n // 2 + 1 if cap is None else cap
    full = lambda cnt, dt, v: torch.full((cnt + GUARD,), v, dtype=dt, device=dev)
    d_bytes = to_dev(raw, dev)
    d_starts = torch.from_numpy(np.asarray(starts, np.int64)).to(dev)
    room = (n + 15) // 16 * 16 + 16
    packed, offsets, fstarts, bad = full(room, torch.uint8, G8), full(cap + 1, torch.int64, G64), full(cap, torch.int64, G64), full(cap, torch.uint8, G8)
    first, cons, stop = full(k + 1, torch.int64, G64), full(k, torch.int64, G64), full(k, torch.uint8, G8)
    nf, payload = C.c_uint64(), C.c_uint64()
    rc = L.lib().fg_frame_syslen_multi_device(dec._ctx, d_bytes.data_ptr(), n, d_starts.data_ptr(), k, packed.data_ptr(), offsets.data_ptr(),
                                              fstarts.data_ptr(), bad.data_ptr(), cap, first.data_ptr(), cons.data_ptr(), stop.data_ptr(),
                                              C.byref(nf), C.byref(payload), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    packed, offsets, fstarts, bad, first, cons, stop = (t.cpu().numpy() for t in (packed, offsets, fstarts, bad, first, cons, stop))
    # nothing is ever written behind the capacities
    assert (offsets[cap + 1:] == G64).all() and (fstarts[cap:] == G64).all() and (bad[cap:] == G8).all()
    assert (first[k + 1:] == G64).all() and (cons[k:] == G64).all() and (stop[k:] == G8).all() and (packed[room:] == G8).all()
    if rc != L.FG_OK:  # (overflow or declined: no frame output, no per-segment output)
        assert (offsets == G64).all() and (fstarts == G64).all() and (first == G64).all() and (cons == G64).all() and (stop == G8).all()
        return rc, {"n": int(nf.value)}
    f, total = int(nf.value), int(payload.value)
    assert (packed[total:] == G8).all() and (fstarts[f:] == G64).all() and (offsets[f + 1:] == G64).all()
    return rc, {"n": f, "total": total, "packed": packed, "offsets": offsets[:f + 1], "starts": fstarts[:f], "bad": bad[:f], "seg_first": first[:k + 1],
                "seg_consumed": cons[:k], "seg_stop": stop[:k]}


def check(dec, raw, starts):
    rc, r = run(dec, raw, starts)
    assert rc == L.FG_OK
    m = model(raw, starts)
    assert_equal(r, m)
    return r, m


def test_one_segment_is_bit_identical_to_the_single_stream_framer(dec):
    import torch

    for raw in (wrap(synth.rfc5424_lines(3000, cfg=2)), wrap(synth.rfc5424_lines(3000, cfg=2))[:-9]):
        dev = torch.device("cuda", dec.device)
        d_packed, d_offs, d_starts, d_bad, n, consumed, stop = dec.frame_syslen_device(to_dev(raw, dev), True)
        torch.cuda.synchronize(dev)
        rc, r = run(dec, raw, [0, len(raw)])
        assert rc == L.FG_OK and n >= 2999
        assert (r["n"], int(r["seg_consumed"][0]), int(r["seg_stop"][0])) == (n, consumed, stop)
        offs = d_offs.cpu().numpy()
        assert np.array_equal(r["offsets"], offs) and np.array_equal(r["starts"], d_starts.cpu().numpy()[:n]) and np.array_equal(r["bad"], d_bad.cpu().numpy())
        assert r["total"] == int(offs[-1]) and np.array_equal(r["packed"][:r["total"]], d_packed[:r["total"]].cpu().numpy())


@pytest.mark.parametrize("n_conn", [8, 300])
def test_a_stream_on_many_connections_with_boundaries_at_the_tile_edges(dec, n_conn):
    """~200 KiB; connection 0 holds the first 18 tiles (cut by the boundary list of the CPU suite: tile edges +-1, empty and one-byte
    segments, a six-tile segment, 40 segments in one tile), the others share the rest"""
    lines = [as_bytes(ln) for ln in synth.rfc5424_lines(800, cfg=2)]
    k = next(k for k in range(len(lines)) if len(wrap(lines[:k])) >= 18 * TILE + 200)
    rest = lines[k:]
    streams = [stream_with_a_frame_at(lines[:k], 8 * TILE + 1)] + [wrap(rest[c::n_conn - 1]) for c in range(n_conn - 1)]
    raw = b"".join(streams)
    assert 180_000 <= len(raw) <= 260_000
    starts = with_boundaries(len(raw), edge_boundaries(len(raw), TILE), np.cumsum([len(s) for s in streams])[:-1])
    r, m = check(dec, raw, starts)
    k = starts.index(8 * TILE + 1)
    assert starts[k + 1] - starts[k] >= 6 * TILE and r["seg_first"][k + 1] - r["seg_first"][k] > 100  # a chain through six tiles
    assert sum(1 for s in starts if s // TILE == 16) >= 40
    assert r["n"] > 500 and {CLEAN, TAIL, BAD_LEN} <= set(m["seg_stop"])


def five_stops():
    segs = [wrap([b"clean one", b"clean two"]), b"2 ok" + b"123", wrap([b"before"]) + b"2 ok" + b"50 short", b"3 abc" + b"x7 no", wrap([b"intact"]),
            b"1 a" + b"0" * (MAX_PREFIX + 2) + b"1 b", wrap([b"intact too", b"caf\xc3\xa9", b"bad \xff"])]
    starts = [0]
    for s in segs:
        starts.append(starts[-1] + len(s))
    return b"".join(segs), starts


def test_lookalikes_utf8_at_segment_ends_and_all_stop_reasons(dec):
    # digits at a segment end, then a segment that starts with ' '; a payload whose length points into the next segment
    r, m = check(dec, b"3 abc" + b"12" + b" hello world!" + b"2 ok", [0, 7, 20, 24])
    assert list(r["seg_stop"]) == [TAIL, BAD_LEN, CLEAN]
    r, m = check(dec, b"2 ok" + b"10 abcd" + b"5 hello" + b"2 ok", [0, 11, 22])
    assert list(r["seg_stop"]) == [TAIL, CLEAN] and list(r["seg_consumed"]) == [4, 11]
    pad = wrap([b"p" * 500] * 8, nl=False)
    check(dec, pad + b"600 " + b"q" * 90 + b"3 abc" + b"z" * 505, [0, len(pad) + 94, len(pad) + 94 + 510])
    # payload text that looks like prefixes, in forty small segments of one tile and across tile ends
    look = wrap([b"12 34 56 7 8 9 10 11 300 ", b"+5 005 ", b"1 2 3 4 5 6 7 8 9 ", b"3 abc"] * 60, nl=False)
    check(dec, look, with_boundaries(len(look), range(97, 97 * 41, 97), [TILE - 1, TILE, TILE + 1, 2 * TILE]))
    # a UTF-8 sequence cut at a payload end that is a segment end; the next segment starts with a continuation byte
    r, m = check(dec, b"5 abc\xe2\x82" + b"\xac2 ok", [0, 7, 12])
    assert list(r["bad"]) == [1] and list(r["seg_stop"]) == [CLEAN, BAD_LEN]
    r, m = check(dec, b"3 a\xe2\x82" + b"3 \xacxy", [0, 5, 10])
    assert list(r["bad"]) == [1, 1]
    raw, starts = five_stops()
    r, m = check(dec, raw, starts)
    assert list(r["seg_stop"]) == [CLEAN, TAIL, TAIL, BAD_LEN, CLEAN, LONG_PREFIX, CLEAN]
    # empty buffers and empty segments
    check(dec, b"", [0, 0, 0])
    check(dec, b"3 abc", [0, 0, 5, 5])


def test_capacity_overflow_reports_the_need_and_writes_nothing(dec):
    raw, starts = five_stops()
    need = model(raw, starts)["n"]
    for cap in (0, 1, need - 1):
        rc, r = run(dec, raw, starts, cap=cap)  # (run looks at every output array)
        assert rc == L.FG_ERR_ENT_OVERFLOW and r["n"] == need
    rc, r = run(dec, raw, starts, cap=need)
    assert rc == L.FG_OK
    assert_equal(r, model(raw, starts))


def serialized(d, fmt, payloads):
    data, offs = synth.pack(payloads)
    return d.decode_packed(data, offs).serialize(fmt, data, offs, cfg=d._cfg)


def test_a_declining_segment_declines_the_launch_and_the_host_entry_hops(dec):
    clean = wrap(synth.rfc5424_lines(40, cfg=2))
    bad = declining_stream()
    raw = clean + bad + clean
    starts = [0, len(clean), len(clean) + len(bad), len(raw)]
    rc, _ = run(dec, raw, starts)
    assert rc == L.FG_ERR_UNSUPPORTED
    m = model(raw, starts, None)
    tab, fstarts, first, cons, stop = dec.frame_decode_syslen_multi(raw, starts)
    assert dec.last_host_path() == L.FG_PATH_FRAME_SYSLEN_MULTI_HOST
    assert (list(fstarts), list(first), list(cons), list(stop)) == (m["starts"], m["seg_first"], m["seg_consumed"], m["seg_stop"])
    data, offs = synth.pack(m["payloads"])
    got, want = tab.serialize(RFC5424, data, offs, cfg=dec._cfg), serialized(dec, RFC5424, m["payloads"])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


@pytest.mark.parametrize("fmt", [RFC5424, LTSV, GELF], ids=["rfc5424", "ltsv", "gelf"])
def test_frame_decode_syslen_multi_equals_the_decode_of_the_hopped_messages(fmt):
    d = make_decoder(fmt)
    lines = [as_bytes(ln) for ln in corpus(fmt, 16 * 200)]
    rng = random.Random(fmt)
    streams = []
    for c in range(16):
        s = wrap(lines[c * 200:(c + 1) * 200], nl=fmt != GELF)
        streams.append(s[:len(s) - rng.randint(0, 300)] if c % 3 == 0 else s)  # (some chunks end inside a frame)
    raw = b"".join(streams)
    starts = [0] + [int(x) for x in np.cumsum([len(s) for s in streams])]
    m = model(raw, starts)
    tab, fstarts, first, cons, stop = d.frame_decode_syslen_multi(raw, starts)
    assert d.last_host_path() == L.FG_PATH_FRAME_SYSLEN_MULTI_DEVICE
    assert (list(fstarts), list(first), list(cons), list(stop)) == (m["starts"], m["seg_first"], m["seg_consumed"], m["seg_stop"])
    assert m["n"] > 16 * 190 and TAIL in m["seg_stop"]
    data, offs = synth.pack(m["payloads"])
    got, want = tab.serialize(fmt, data, offs, cfg=d._cfg), serialized(d, fmt, m["payloads"])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[0], want[0])


def sequential(d, stream):
    """what SyslenSplitter::run makes of one connection's whole stream, EOF included (flowgger_amd/host/fg_decoder.hpp's Syslen branch)"""
    out, pos = [], 0
    while True:
        st, pl, ln = read_msglen(stream, pos)
        if st != VALID:
            break
        payload = stream[pos + pl:pos + pl + ln]
        pos += pl + ln
        if not valid_utf8(payload):
            return out + [SYSLEN_PANIC]
        r = d.decode_batch([payload])[0]
        out.append(f"{r}: [{payload.decode('utf-8').strip(RUST_WS)}]" if isinstance(r, DecodeError) else r)
    tail = stream[pos:]
    if st in (CLEAN, BAD_LEN) or len(tail) <= 1:
        return out + [SYSLEN_BAD_LENGTH]
    if b" " in tail:
        return out + [SYSLEN_SHORT_READ]  # EOF inside a payload
    num = tail[:-1].lstrip(b"+") if tail[:1] == b"+" else tail[:-1]  # EOF inside a length: read_until drops the last byte it read
    if not num.isdigit():
        return out + [SYSLEN_BAD_LENGTH]
    if int(num) != 0:
        return out + [SYSLEN_SHORT_READ]
    r = d.decode_batch([b""])[0]
    return out + [f"{r}: []" if isinstance(r, DecodeError) else r, SYSLEN_BAD_LENGTH]


def test_multi_syslen_splitter_equals_a_splitter_per_connection():
    d = RFC5424Decoder()
    rng = random.Random(99)
    lines = [as_bytes(ln) for ln in synth.rfc5424_lines(8 * 60, cfg=2)]
    streams = []
    for c in range(8):
        mine = lines[c * 60:(c + 1) * 60]
        if c == 1:
            mine[20] = b"not a syslog line"  # the decoder's error, with the payload
            mine[21] = b""
        if c == 4:
            mine[25] = mine[25][:30] + b"\xf0\x9f\x98" + mine[25][30:]  # an invalid payload: the connection's thread panics there
        s = wrap(mine, nl=c % 2 == 0)
        if c == 2:
            s = wrap(mine[:30]) + b"12x " + wrap(mine[30:])  # a bad length mid-stream
        if c == 3:
            s = s[:-40]  # closed inside a payload
        if c == 5:
            s += b"00"  # closed inside a length: "0" + a dropped byte = an empty message
        if c == 6:
            s += b"17"  # closed inside a length: "1" + a dropped byte, nothing follows
        streams.append(s)
    want = [sequential(d, s) for s in streams]
    ms = MultiSyslenSplitter(d, FlushPolicy(max_bytes=1 << 30, max_latency_ms=1e9))
    got, pos, over, flushes = [[] for _ in streams], [0] * 8, set(), 0
    while any(pos[c] < len(streams[c]) for c in range(8) if c not in over):
        for c in rng.sample(range(8), 8):
            if pos[c] >= len(streams[c]) or c in over:
                continue
            step = rng.randint(1, 2500)
            assert ms.push(c, streams[c][pos[c]:pos[c] + step]) == []
            pos[c] += step
            if pos[c] >= len(streams[c]):
                ms.close(c)
        for c, res in ms.flush():
            got[c] += res
            if res and isinstance(res[-1], DecodeError) and str(res[-1]) in (SYSLEN_BAD_LENGTH, SYSLEN_PANIC, SYSLEN_SHORT_READ):
                over.add(c)
        flushes += 1
    assert flushes >= 5 and ms.flush() == []
    for c in (2, 4):
        with pytest.raises(ValueError):
            ms.push(c, b"1 a")
    for c in range(8):
        have = [str(r) if isinstance(r, DecodeError) else r for r in got[c]]
        assert len(have) == len(want[c]), (c, len(have), len(want[c]))
        for i, (a, b) in enumerate(zip(have, want[c])):
            assert a == b, (c, i, a, b)
    assert want[2][-1] == SYSLEN_BAD_LENGTH and len(want[2]) == 31 and want[4][-1] == SYSLEN_PANIC and len(want[4]) == 26
    assert want[3][-1] == SYSLEN_SHORT_READ and want[6][-1] == SYSLEN_SHORT_READ and want[5][-2].endswith(": []")
    assert any(isinstance(x, str) and x.endswith(": [not a syslog line]") for x in want[1])
