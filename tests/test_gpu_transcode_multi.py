"""GPU: fg_transcode_multi_batch -- the chunks of many connections framed, decoded and encoded in one call -- through Pipeline.run_multi
and MultiTranscodingSplitter.  Slots and kinds are the models' (frame_multi_model, syslen_multi_model with the per-segment cut of
transcode_multi_model, capnp_frame_multi_model); the bytes are the oracle's encoding of every segment's FG_SLOT_FRAME payloads in
segment order (Cap'n Proto input: the reader's model and the oracle's encoders; the Cap'n Proto encoder: capnp_wire).  Every case first
checks ON THE MODEL that it holds what it is there for."""
from __future__ import annotations

import struct

import numpy as np
import pytest

import capnp_read_model as M
import capnp_wire as W
import oracle_binding as OB
from capnp_frame_multi_model import model as capnp_model
from flowgger_amd import (CapnpDecoder, CapnpEncoder, FlushPolicy, GelfDecoder, GelfEncoder, LTSVDecoder, MultiCapnpSplitter,
                          MultiStreamSplitter, MultiSyslenSplitter, MultiTranscodingSplitter, PassthroughEncoder, Pipeline, RFC3164Decoder,
                          RFC5424Decoder, RFC5424Encoder, synth, tzdb)
from flowgger_amd import _lib as L
from flowgger_amd.record import DecodeError, Record, parse_canonical
from frame_multi_model import model as lines_model
from syslen_multi_model import model as syslen_model
from transcode_multi_model import BAD_UTF8, CARRY, FRAME, UNREACHED, cut, cut_hazards

pytestmark = pytest.mark.gpu

NOW = 1438859724.638
LINE, NUL, SYSLEN, CAPNP = L.FG_FRAME_LINE, L.FG_FRAME_NUL, L.FG_FRAME_SYSLEN, L.FG_FRAME_CAPNP
GOOD = b"<13>1 2015-08-05T15:53:45Z host app 1 - - message"


@pytest.fixture(scope="module")
def orc():
    o = OB.Oracle()
    o.set_rfc3164(2026, tzdb.default_table())
    return o


def fmt_case(name):
    """-> (decoder, oracle config, lines, (encoder, what expected_stream takes for it))"""
    clean = lambda ls: [x.replace(b"\0", b" ").replace(b"\n", b" ") for x in ls]
    if name == "rfc5424":
        return RFC5424Decoder(), None, clean(synth.rfc5424_lines(56, cfg=2)), (PassthroughEncoder(None, merger="nul"), (OB.ENC_PASSTHROUGH, OB.MERGE_NUL))
    if name == "ltsv":
        return LTSVDecoder(synth.LTSV_CONFIG), synth.LTSV_CONFIG, clean(synth.ltsv_lines(56)), (RFC5424Encoder(None, merger="syslen"), (OB.ENC_RFC5424, OB.MERGE_SYSLEN))
    if name == "gelf":
        return GelfDecoder(), None, clean(synth.gelf_lines(56)), (GelfEncoder(None, merger="line"), (OB.ENC_GELF, OB.MERGE_LINE))
    return RFC3164Decoder({"rfc3164": {"current_year": 2026}}), None, clean(synth.rfc3164_lines(56)), (CapnpEncoder(None, merger=None), ("capnp", 0))


def expected_stream(orc, fmt, cfg, enc, bodies):
    """the oracle's decode + encode + merger of `bodies` -> (stream, size per body, decode status per body)"""
    data, offsets = synth.pack(bodies)
    if enc[0] == "capnp":
        blob, offs = orc.decode_batch(fmt, data, offsets, cfg)
        recs = [parse_canonical(blob[int(offs[i]):int(offs[i + 1])].tobytes(), now=NOW) for i in range(len(bodies))]
        parts = [b"" if isinstance(r, DecodeError) else W.frame(W.serialize(r, []), enc[1]) for r in recs]
        return b"".join(parts), [len(p) for p in parts], [int(isinstance(r, DecodeError)) for r in recs]
    blob, offs, st = orc.decode_encode_batch(fmt, enc[0], enc[1], data, offsets, cfg, now_ts=NOW)
    return blob.tobytes(), np.diff(offs.astype(np.int64)).tolist(), st.tolist()


def assert_slots(t, kind, bodies_of_frames, want):
    """t: TranscodedMulti; kind: the model's; want: expected_stream over the FRAME slots' bodies, in slot order.  No slot is left out."""
    stream, sizes, failed = want
    assert t.slot_kind.tolist() == list(kind)
    assert t.out.tobytes() == stream
    sz = iter(zip(sizes, failed))
    got = np.diff(t.out_offsets.astype(np.int64)).tolist()
    for i, k in enumerate(kind):
        if k != FRAME:
            assert got[i] == 0 and t.dec_status[i] == L.FG_ST_BAD_UTF8 and t.enc_status[i] == 1, i
        else:
            size, bad = next(sz)
            assert got[i] == size and (t.dec_status[i] != 0) == (bad == 1) and (t.enc_status[i] == 0) == (size > 0), (i, got[i], size, bad)
    assert int(t.out_offsets[0]) == 0 and int(t.out_offsets[-1]) == len(stream)


def bodies(raw, offsets, kind, framing):
    out = []
    for i, k in enumerate(kind):
        if k == FRAME:
            out.append(MultiStreamSplitter._unterminated(raw[int(offsets[i]):int(offsets[i + 1])], framing))
    return out


def starts_of(segs):
    return [0] + np.cumsum([len(s) for s in segs]).tolist()


# ---- LINE and NUL ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("framing", [LINE, NUL], ids=["line", "nul"])
@pytest.mark.parametrize("name", ["rfc5424", "ltsv", "gelf", "rfc3164"])
def test_eight_segments_in_eight_kib(orc, name, framing):
    dec, cfg, ln, (enc, oenc) = fmt_case(name)
    t_ = b"\n" if framing == LINE else b"\0"
    text = lambda a, b: b"".join(x + (b"\r\n" if framing == LINE and i % 3 == 0 else t_) for i, x in enumerate(ln[a:b]))
    segs = [text(0, 8), b"", text(8, 16) + ln[16], text(17, 24) + b"bad \xe2\x82 utf8" + t_ + text(24, 30) + ln[30][:40], b"no terminator, not final",
            text(31, 40) + b"this is no log line at all" + t_ + t_, text(40, 48) + ln[48], text(49, 56)]
    final = [0, 1, 1, 0, 0, 1, 0, 1]
    raw, starts = b"".join(segs), starts_of(segs)
    assert 2000 < len(raw) < 32768
    m = lines_model(orc, raw, starts, final, 0 if framing == LINE else 1)
    kind = m.kind.tolist()
    want = expected_stream(orc, dec.fmt, cfg, oenc, bodies(raw, m.offsets, kind, framing))
    assert kind.count(CARRY) == 3 and kind.count(BAD_UTF8) == 1 and sum(1 for s in want[1] if s) > 40 and sum(want[2]) >= 2
    t = Pipeline(dec, enc).run_multi(raw, starts, final, framing, now_ts=NOW)
    assert dec.last_host_path() == L.FG_PATH_FRAME_MULTI
    assert t.slot_offsets.tolist() == m.offsets.tolist() and t.seg_first.tolist() == m.seg_first.tolist()
    assert t.seg_consumed.tolist() == m.seg_consumed.tolist() and t.seg_stop is None
    assert_slots(t, kind, None, want)


def test_a_carry_of_100_kib_between_the_short_lines_of_two_neighbours(orc):
    """about 200 slots, so that the 64 lines of an encoder workgroup span segments -- and a never-encoded run of 100 KiB inside the input
    range such a workgroup covers"""
    dec = RFC5424Decoder()
    ln = [x.replace(b"\0", b" ") for x in synth.rfc5424_lines(200, cfg=2)]
    text = lambda a, b: b"".join(x + b"\n" for x in ln[a:b])
    segs = [text(0, 70) + b"no log line\n", text(70, 100) + b"<13>1 2015-08-05T15:53:45Z host app 1 - - " + b"C" * (100 << 10), text(100, 130) + b"\xff\n", text(130, 200)]
    final = [0, 0, 0, 1]
    raw, starts = b"".join(segs), starts_of(segs)
    m = lines_model(orc, raw, starts, final, 0)
    kind = m.kind.tolist()
    oenc = (OB.ENC_GELF, OB.MERGE_LINE)
    want = expected_stream(orc, dec.fmt, None, oenc, bodies(raw, m.offsets, kind, LINE))
    carry = kind.index(CARRY)
    assert kind.count(CARRY) == 1 and 64 < carry < 128 and int(m.offsets[carry + 1] - m.offsets[carry]) > 100 << 10 and len(kind) == 203
    assert kind.count(BAD_UTF8) == 1 and sum(want[2]) >= 1 and sum(1 for s in want[1] if s) > 150
    t = Pipeline(dec, GelfEncoder(None, merger="line")).run_multi(raw, starts, final, LINE, now_ts=NOW)
    assert t.slot_offsets.tolist() == m.offsets.tolist() and t.seg_first.tolist() == m.seg_first.tolist() and t.seg_consumed.tolist() == m.seg_consumed.tolist()
    assert_slots(t, kind, None, want)


# ---- SYSLEN ---------------------------------------------------------------------------------------------------------------------------
def syslen_check(orc, dec, raw, starts, path, bound=24):
    m = syslen_model(raw, starts, None if path == L.FG_PATH_FRAME_SYSLEN_MULTI_HOST else bound)
    kind = cut(m["bad"], m["seg_first"])
    want = expected_stream(orc, dec.fmt, None, (OB.ENC_GELF, OB.MERGE_LINE), [p for p, k in zip(m["payloads"], kind) if k == FRAME])
    t = Pipeline(dec, GelfEncoder(None, merger="line")).run_multi(raw, starts, None, SYSLEN, now_ts=NOW)
    assert dec.last_host_path() == path
    assert t.slot_offsets.tolist() == m["starts"] and t.seg_first.tolist() == m["seg_first"] and t.seg_consumed.tolist() == m["seg_consumed"]
    assert t.seg_stop.tolist() == m["seg_stop"]
    assert_slots(t, kind, None, want)
    return kind, want, m


@pytest.mark.parametrize("name,first,bad", cut_hazards(), ids=[c[0] for c in cut_hazards()])
def test_the_cut_hazards_end_to_end(orc, name, first, bad):
    dec = RFC5424Decoder()
    n = len(bad)
    four = name.startswith("3000")  # (one segment of four-byte frames between two of real lines)
    ok = [b"ab" if (four and 7 <= i < 3007) or i % 3 == 0 else GOOD for i in range(n)]
    frames = [b"%d %s" % (len(p), p) for p in (b"\xff\xfe" if b else o for b, o in zip(bad, ok))]
    segs = [b"".join(frames[a:b]) for a, b in zip(first, first[1:])]
    raw, starts = b"".join(segs), starts_of(segs)
    kind, want, m = syslen_check(orc, dec, raw, starts, L.FG_PATH_FRAME_SYSLEN_MULTI_DEVICE)
    assert m["n"] == n and kind == cut(bad, first)
    if sum(bad) and n > 8:
        assert sum(1 for s in want[1] if s) >= 1 and sum(want[2]) >= 1 and BAD_UTF8 in kind
    if four:
        assert kind.count(BAD_UTF8) == 1 and kind.count(UNREACHED) == 3000 - 71


def test_segments_that_stop_with_tail_and_bad_len_beside_a_cut_one(orc):
    wrap = lambda ms: b"".join(b"%d %s" % (len(x), x) for x in ms)
    segs = [wrap([GOOD, b"\xff", GOOD, GOOD]), wrap([GOOD, b"nonsense"]) + b"12", wrap([GOOD] * 3) + b" x", wrap([GOOD, b"\xc3"]) + b"700 short", b"",
            wrap([GOOD, GOOD])]
    kind, want, m = syslen_check(orc, RFC5424Decoder(), b"".join(segs), starts_of(segs), L.FG_PATH_FRAME_SYSLEN_MULTI_DEVICE)
    assert m["seg_stop"] == [L.FG_SYSLEN_CLEAN, L.FG_SYSLEN_TAIL, L.FG_SYSLEN_BAD_LEN, L.FG_SYSLEN_TAIL, L.FG_SYSLEN_CLEAN, L.FG_SYSLEN_CLEAN]
    assert kind[:4] == [FRAME, BAD_UTF8, UNREACHED, UNREACHED] and kind.count(BAD_UTF8) == 2 and sum(want[2]) == 1 and sum(1 for s in want[1] if s) == 8


def test_a_long_prefix_takes_the_host_hop_and_the_host_cut(orc):
    wrap = lambda ms: b"".join(b"%d %s" % (len(x), x) for x in ms)
    segs = [wrap([GOOD, b"\xff", GOOD, GOOD]), b"0" * 40 + wrap([GOOD, b"ab"]), wrap([b"\xfe", GOOD]), wrap([GOOD])]
    kind, want, m = syslen_check(orc, RFC5424Decoder(), b"".join(segs), starts_of(segs), L.FG_PATH_FRAME_SYSLEN_MULTI_HOST)
    assert kind == [FRAME, BAD_UTF8, UNREACHED, UNREACHED, FRAME, FRAME, BAD_UTF8, UNREACHED, FRAME] and sum(want[2]) == 1 and want[1].count(0) == 1


# ---- CAPNP ----------------------------------------------------------------------------------------------------------------------------
def capnp_messages(n):
    from test_capnp_in_cpu import simple
    out = [W.serialize(Record(ts=1.5 + i, hostname=f"host{i % 5}", appname="app", msg="m" * (i % 40), facility=i % 24, severity=i % 8)) for i in range(n)]
    out[n // 2] = simple(ts=float("nan"))  # handle_message fails on it
    return out


def capnp_expected(orc, msgs, enc):
    from test_gpu_capnp_in import canonical_of
    parts = []
    for msg in msgs:
        w = M.handle_message(msg)
        if w[0] != "ok":
            parts.append(b"")
        elif enc == "capnp":
            parts.append(W.frame(W.serialize(w[1], []), 1))
        else:
            parts.append(orc.encode(OB.ENC_GELF, canonical_of(w[1]), OB.MERGE_LINE, now_ts=NOW))
    return b"".join(parts), [len(p) for p in parts], [int(not p) for p in parts]


@pytest.mark.parametrize("enc", ["gelf", "capnp"])
def test_four_capnp_connections_with_carries_a_stop_and_a_failing_message(orc, enc):
    ms = capnp_messages(40)
    segs = [b"".join(ms[0:10]) + ms[10][:-8], b"".join(ms[10:25]) + ms[25][:16], b"".join(ms[25:30]) + struct.pack("<2I", 511, 0) + bytes(24),
            b"".join(ms[30:40]) + ms[0][:8]]
    raw, starts = b"".join(segs), starts_of(segs)
    m = capnp_model(raw, starts)
    kind, offs = m["kind"], m["offsets"]
    want = capnp_expected(orc, [raw[offs[i]:offs[i + 1]] for i, k in enumerate(kind) if k == FRAME], enc)
    assert kind.count(CARRY) == 4 and m["seg_stop"] == [L.FG_CAPNP_TAIL, L.FG_CAPNP_TAIL, L.FG_CAPNP_TOO_MANY_SEGMENTS, L.FG_CAPNP_TAIL]
    assert sum(want[2]) == 1 and sum(1 for s in want[1] if s) == 39
    dec = CapnpDecoder()
    encoder = GelfEncoder(None, merger="line") if enc == "gelf" else CapnpEncoder(None, merger="line")
    t = Pipeline(dec, encoder).run_multi(raw, starts, None, CAPNP, now_ts=NOW)
    assert dec.last_host_path() == L.FG_PATH_FRAME_CAPNP_MULTI_DEVICE
    assert t.slot_offsets.tolist() == offs and t.seg_first.tolist() == m["seg_first"] and t.seg_consumed.tolist() == m["seg_consumed"]
    assert t.seg_stop.tolist() == m["seg_stop"]
    assert_slots(t, kind, None, want)


# ---- equivalences ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("framing", [LINE, SYSLEN, CAPNP], ids=["line", "syslen", "capnp"])
def test_one_final_segment_is_transcode_batch_and_the_stream_is_the_siblings_rows_encoded(framing):
    ln = [x.replace(b"\0", b" ") for x in synth.rfc5424_lines(150, cfg=4, sd=True)] + [b"no log line"]
    if framing == LINE:
        dec, raw = RFC5424Decoder(), b"".join(x + b"\n" for x in ln) + b"<13>1 - h a 1 - - the tail"
    elif framing == SYSLEN:
        dec, raw = RFC5424Decoder(), b"".join(b"%d %s" % (len(x), x) for x in ln)
    else:
        dec, raw = CapnpDecoder(), b"".join(capnp_messages(150))
    pipe = Pipeline(dec, GelfEncoder({"output": {"gelf_extra": {"x": "y"}}}, merger="line"))
    one = pipe.run_stream(raw, framing, final=True, now_ts=NOW)
    t = pipe.run_multi(raw, [0, len(raw)], [1] if framing == LINE else None, framing, now_ts=NOW)
    assert t.n == one.n > 100 and t.out.tobytes() == one.out.tobytes() and np.array_equal(t.out_offsets, one.out_offsets)
    assert np.array_equal(t.meta, one.meta) and np.array_equal(t.enc_status, one.enc_status) and 0 < int((t.enc_status != 0).sum()) < 10
    assert np.array_equal(t.slot_offsets, one.frame_offsets[:len(t.slot_offsets)])
    # the sibling's slots and rows on a buffer of three segments; its FRAME slots through decode + encode as one packed batch
    if framing == LINE:  # (anywhere: the cut lines are a CARRY and a frame that fails)
        starts = [0, len(raw) // 3, 2 * len(raw) // 3, len(raw)]
    else:  # (between two frames: a connection's chunk starts with a length or a segment table)
        sizes = [len(b"%d %s" % (len(x), x)) for x in ln] if framing == SYSLEN else [len(x) for x in capnp_messages(150)]
        starts = [0, sum(sizes[:50]), sum(sizes[:100]), len(raw)]
    t = pipe.run_multi(raw, starts, [0, 1, 0] if framing == LINE else None, framing, now_ts=NOW)
    if framing == LINE:
        tab, offsets, kind, first, cons = dec.frame_decode_multi(raw, starts, [0, 1, 0], LINE)
        frames = bodies(raw, offsets, kind.tolist(), LINE)
    elif framing == SYSLEN:
        tab, offsets, first, cons, stop = dec.frame_decode_syslen_multi(raw, starts)
        kind = np.zeros(len(offsets), np.uint8)
        frames = []
        for a in offsets:
            sp = raw.index(b" ", int(a))
            frames.append(raw[sp + 1:sp + 1 + int(raw[int(a):sp])])
    else:
        tab, offsets, kind, first, cons, stop = dec.frame_decode_capnp_multi(raw, starts)
        frames = [raw[int(offsets[i]):int(offsets[i + 1])] for i, k in enumerate(kind) if k == FRAME]
    assert np.array_equal(t.slot_kind, kind) and np.array_equal(t.slot_offsets, offsets) and np.array_equal(t.seg_first, first)
    assert np.array_equal(t.seg_consumed, cons) and np.array_equal(t.dec_status, tab.status[:t.n])
    if framing == CAPNP:
        from test_capnp_in_cpu import pack_words
        packed = pipe.run_packed(*pack_words(frames), now_ts=NOW)
    else:
        packed = pipe.run_packed(*synth.pack(frames), now_ts=NOW)
    assert t.out.tobytes() == packed.out.tobytes() and packed.n == int((kind == FRAME).sum()) > 100


# ---- the splitter ---------------------------------------------------------------------------------------------------------------------
def encode_records(orc, items):
    from test_gpu_capnp_in import canonical_of
    return b"".join(orc.encode(OB.ENC_GELF, canonical_of(r), OB.MERGE_LINE, now_ts=NOW) for r in items if isinstance(r, Record))


def texts(items):
    return [(type(x).__name__, str(x)) for x in items if not isinstance(x, Record)]


@pytest.mark.parametrize("framing", [LINE, SYSLEN, CAPNP], ids=["line", "syslen", "capnp"])
def test_the_splitter_against_the_decode_side_splitter_on_identical_pushes(orc, framing):
    policy = lambda: FlushPolicy(max_bytes=1 << 30, max_latency_ms=1e9)  # (flushed by hand)
    ln = [x.replace(b"\0", b" ") for x in synth.rfc5424_lines(8 * 12, cfg=2)]
    if framing == LINE:
        dec = RFC5424Decoder()
        side = MultiStreamSplitter(dec, LINE, policy())
        streams = [b"".join(x + b"\n" for x in ln[12 * c:12 * c + 12]) for c in range(8)]
        streams[3] = streams[3][:200] + b"\xff" + streams[3][200:] + b"the last line has no terminator"
        streams[5] = b"no log line\n" + streams[5]
    elif framing == SYSLEN:
        dec = RFC5424Decoder()
        side = MultiSyslenSplitter(dec, policy())
        wrap = lambda ms: b"".join(b"%d %s" % (len(x), x) for x in ms)
        streams = [wrap(ln[12 * c:12 * c + 12]) for c in range(8)]
        streams[3] = wrap(ln[36:40] + [b"pa\xffnic"] + ln[40:48])
        streams[5] = wrap([b"no log line"] + ln[60:72])
        streams[6] = wrap(ln[72:80]) + b"x12 y" + wrap(ln[80:84])  # (a length that cannot be read ends the connection)
    else:
        dec = CapnpDecoder()
        side = MultiCapnpSplitter(dec, policy())
        ms = capnp_messages(96)
        streams = [b"".join(ms[12 * c:12 * c + 12]) for c in range(8)]
        streams[6] = b"".join(ms[72:80]) + struct.pack("<2I", 511, 0) + bytes(24)
    tr = MultiTranscodingSplitter(dec, GelfEncoder(None, merger="line"), framing, policy(), now_ts=NOW)
    cuts = [[0, len(s) // 3 + c, 2 * len(s) // 3 + 3 * c + 1, len(s)] for c, s in enumerate(streams)]  # (tails that complete a round later)
    out_bytes = n_err = n_rec = 0
    for rnd in range(3):
        for c, s in enumerate(streams):
            chunk = s[cuts[c][rnd]:cuts[c][rnd + 1]]
            ended = [isinstance(_raises(sp, c, chunk), ValueError) for sp in (side, tr)]
            assert ended[0] == ended[1], (rnd, c)
            if framing == SYSLEN and c == 3 and rnd == 2:
                assert ended == [True, True]  # (the connection that panicked: its later push raises)
        if rnd == 1:
            side.close(1)
            tr.close(1)
        want, (got, errs) = side.flush(), tr.flush()
        assert [c for c, _ in errs] == [c for c, _ in want]
        for (c, items), (_, e) in zip(want, errs):
            assert texts(e) == texts(items), (rnd, c)
            n_err += len(e)
            n_rec += len(items) - len(e)
        assert got == b"".join(encode_records(orc, items) for _, items in want), rnd
        out_bytes += len(got)
    assert out_bytes > 5000 and n_err >= 2 and n_rec > 60
    if framing != LINE:
        assert 6 in tr._over and 6 in side._over  # (the connection whose input ended it)


def _raises(sp, c, chunk):
    try:
        sp.push(c, chunk)
    except ValueError as e:
        return e
    return None
