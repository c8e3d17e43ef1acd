"""The streams of tests/ltsv_hazards.py -- a byte at every boundary of the LTSV kernel: the TAB window, the ':' window, the key and
suffix compares, the in-tile records, the register windows behind a value's end, the end of a long line's staged head and the rows
scanned behind it -- through the C ABI on the device: every launch option that selects another kernel or tile geometry, the host path,
the framed routes (fg_frame_device + fg_decode_frames_device, the fused fg_frame_decode_device, fg_frame_decode_batch from pinned
memory) and the transcoding pipeline, which USES the spans.  The oracle alone is the checker, and tests/test_ltsv_hazards_cpu.py has
pinned what it says: EVERY line of every stream must give the Record or the error it was built to give."""
from __future__ import annotations

from collections import Counter

import numpy as np
import pytest

import ltsv_hazards as H
from flowgger_amd import LTSVDecoder
from flowgger_amd import _lib as L
from gpu_util import assert_same, device_path, host_path_blob
from test_gpu_escape_hazards import frames_then_decode, pinned_batch
from test_gpu_round6 import expected_frames, run_device

pytestmark = pytest.mark.gpu

LTSV = 1
OPTS = [dict(), dict(lines_per_group=5, tile_cap=4096), dict(lines_per_group=64), dict(tile_cap=57344), dict(force_head=True),
        dict(force_head=True, tile_cap=6144, lines_per_group=5), dict(no_head=True)]
# the fused kernel stages whole lines in byte tiles planned for the everyday line length: the streams of long lines are declined
FUSED_AVG = 254
FUSED_STREAMS = ("tab-index", "tab-parts", "colon", "keys", "suffix", "suffix9", "records", "value-end")
LEDGER: Counter = Counter()  # (class, route) -> lines decoded and compared
_REF: dict = {}


def ident(opts: dict) -> str:
    return ",".join(f"{k}={v}" for k, v in opts.items()) or "default"


def report():
    for k in sorted(LEDGER):
        print(k, LEDGER[k])


def decoders(opts: dict = {}):
    """one decoder per configuration of the streams"""
    out = {}
    for cfg in (H.CONFIG, H.CONFIG9):
        dec = LTSVDecoder(cfg)
        dec.set_launch_opts(**opts)
        out[id(cfg)] = dec
    return out


def ring_ok(decs):
    for dec in decs.values():
        assert dec._ctx and L.lib().fg_ticket_ring_check(dec._ctx) == 0


def reference(oracle, s: H.Stream):
    """the oracle's Records of a stream's bare lines, computed once: (data, offsets, blob, blob offsets)"""
    key = (s.name, s.framing)
    if key not in _REF:
        lines = s.lines()
        offsets = np.zeros(len(lines) + 1, np.uint64)
        offsets[1:] = np.cumsum([len(x) for x in lines])
        data = np.frombuffer(b"".join(lines) + b"\0" * 64, np.uint8).copy()
        _REF[key] = (data, offsets) + tuple(oracle.decode_batch(LTSV, data, offsets, s.config))
    return _REF[key]


def same(oracle, s: H.Stream, blob, offs, ctx: str):
    """assert_same against the oracle; the first differing line with its class and what it aims at"""
    _, _, oblob, ooffs = reference(oracle, s)
    try:
        assert_same(blob, offs, oblob, ooffs, [x[:200] for x in s.lines()])
    except AssertionError as e:
        what = ""
        for i in range(min(len(offs), len(ooffs)) - 1):
            if blob[int(offs[i]):int(offs[i + 1])].tobytes() != oblob[int(ooffs[i]):int(ooffs[i + 1])].tobytes():
                h, a = s.ln[i], s.offsets[i]
                what = (f"class {h.cls}, aim {h.aim or 'helper'!r}, line offset {h.pos}, want {h.want}; the line starts at {a} "
                        f"(& 15 = {a & 15}), {len(h.line)} bytes; ")
                break
        raise AssertionError(f"{s.name} [{ctx}]: {what}{str(e)[:1500]}") from None
    LEDGER[(s.cls, ctx.split(" [")[0])] += len(s.ln)


@pytest.mark.parametrize("opts", OPTS, ids=ident)
def test_every_class_device_and_host_path(oracle, opts):
    """k_ltsv with whole lines and with heads only, at its tile geometries; the lines a tile hands back, from global memory"""
    decs = decoders(opts)
    for s in H.streams(H.NONE):
        dec = decs[id(s.config)]
        data = np.frombuffer(s.raw + b"\0" * 64, np.uint8).copy()
        offsets = np.array(s.offsets, np.uint64)
        tables, _, _ = device_path(dec, data, offsets, ent_cap=len(s.raw) // 4 + 65536)
        blob, offs = tables.to_host().serialize(dec.fmt, data, offsets, cfg=dec._cfg)
        same(oracle, s, blob, offs, f"device [{ident(opts)}]")
        (blob, offs), _ = host_path_blob(dec, data, offsets)
        same(oracle, s, blob, offs, f"host [{ident(opts)}]")
    ring_ok(decs)
    report()


@pytest.mark.parametrize("framing", [H.LINE, H.NUL], ids=["line", "nul"])
@pytest.mark.parametrize("opts", [dict(), dict(force_head=True), dict(no_head=True)], ids=ident)
def test_framed_routes(oracle, opts, framing):
    """the streams with a terminator behind every line: framed and decoded by separate kernels (the decoder strips), by the fused
    kernel and by one pinned fg_frame_decode_batch"""
    fr = L.FG_FRAME_LINE if framing == H.LINE else L.FG_FRAME_NUL
    decs = decoders(opts)
    paths = Counter()
    for s in H.streams(framing):
        dec = decs[id(s.config)]
        starts, ends, valid = expected_frames(oracle, s.raw, fr, True)
        assert [int(x) for x in starts] == s.offsets[:-1] and int(ends[-1]) == len(s.raw) and bool(valid.all())
        data = np.frombuffer(s.raw + b"\0" * 64, np.uint8)

        def check(tab, offs, ctx):
            offs = np.ascontiguousarray(offs[: len(s.ln) + 1], np.uint64)
            assert [int(x) for x in offs] == s.offsets, f"{s.name} {ctx}: frame offsets differ"
            assert not (tab.status[: len(s.ln)] == L.FG_ST_BAD_UTF8).any()
            blob, boffs = tab.serialize(dec.fmt, data, offs, 0, len(s.ln), cfg=dec._cfg)
            same(oracle, s, blob, boffs, ctx)

        tab, offs = frames_then_decode(dec, s.raw, fr, len(starts))
        check(tab, offs, f"frame + decode [{ident(opts)}]")
        if not opts and s.name in FUSED_STREAMS:
            tables, offs, n = run_device(dec, s.raw, fr, True, avg_line=FUSED_AVG, cap=len(starts) + 64)
            assert n == len(starts), f"{s.name} fused: {n} frames, the oracle has {len(starts)}"
            check(tables.to_host(), offs, "fused")
        tab, offs, n, used, path = pinned_batch(dec, s.raw, fr)
        assert n == len(starts) and used == len(s.raw)
        check(tab, offs, f"pinned batch [{ident(opts)}]")
        paths[path] += 1
    ring_ok(decs)
    print("fg_frame_decode_batch took FG_PATH", dict(paths))
    report()


@pytest.mark.parametrize("opts", [dict(), dict(force_head=True)], ids=ident)
def test_one_stream_per_class_through_the_pipeline(oracle, opts):
    """decode -> LTSV encode -> line merger in one call: the spans the decoder stored are what the encoder copies from"""
    import oracle_binding as OB
    from flowgger_amd import LTSVEncoder, Pipeline

    now_ts = 1438859724.638
    seen = set()
    decs = decoders(opts)
    for s in H.streams(H.NONE):
        if s.cls in seen:
            continue
        seen.add(s.cls)
        dec = decs[id(s.config)]
        data = np.frombuffer(s.raw + b"\0" * 64, np.uint8).copy()
        offsets = np.array(s.offsets, np.uint64)
        oblob, ooffs, ost = oracle.decode_encode_batch(LTSV, OB.ENC_LTSV, OB.MERGE_LINE, data, offsets, s.config, now_ts=now_ts)
        r = Pipeline(dec, LTSVEncoder(None, merger="line")).run_packed(data, offsets, now_ts=now_ts)
        assert r.n == len(s.ln) and r.consumed == len(s.raw)
        for i, h in enumerate(s.ln):
            got = r.out[int(r.out_offsets[i]):int(r.out_offsets[i + 1])].tobytes() if i + 1 < len(r.out_offsets) else None
            want = oblob[int(ooffs[i]):int(ooffs[i + 1])].tobytes()
            assert got == want, (f"{s.name} [{ident(opts)}] line {i}: class {h.cls}, aim {h.aim or 'helper'!r}, line offset {h.pos}, want {h.want}: "
                                 f"{h.line[:200]!r}\n  gpu    {None if got is None else got[:300]!r}\n  oracle {want[:300]!r}")
        assert np.array_equal(r.out_offsets, ooffs) and np.array_equal(np.minimum(r.enc_status, 2), ost)
        _, _, dblob, doffs = reference(oracle, s)
        assert np.array_equal(r.dec_status != 0, dblob[doffs[:-1].astype(np.int64)] != 0)
        LEDGER[(s.cls, "pipeline")] += len(s.ln)
    assert seen == set(H.CLASSES)
    ring_ok(decs)
    report()
