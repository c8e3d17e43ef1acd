"""The streams of tests/escape_hazards.py -- a run of backslashes and the quote behind it at every boundary across which the GELF fast
form and the structured-data walk of RFC5424 carry escape state -- through the C ABI on the device: every launch option that selects
another kernel or tile geometry, HEAD rows and the second look, the byte-wise fall-backs behind a tile bail, and the framed routes
(fg_frame_device + fg_decode_frames_device, the fused fg_frame_decode_device, fg_frame_decode_batch from pinned memory).  The oracle
alone is the checker: EVERY line of every stream must give its Record or its error, whichever form decoded it.  The same streams run
on the CPU emulation of the two fast forms in tests/test_escape_hazards_cpu.py, which also checks which lines they handle themselves."""
from __future__ import annotations

import ctypes as C
from collections import Counter

import numpy as np
import pytest

import escape_hazards as E
from flowgger_amd import GelfDecoder, RFC5424Decoder
from flowgger_amd import _lib as L
from flowgger_amd.tables import DeviceTables, HostTables
from gpu_util import assert_same, device_path
from test_gpu_round6 import check_rows, expected_frames, run_device

pytestmark = pytest.mark.gpu

DECODER = {E.GELF: GelfDecoder, E.SD: RFC5424Decoder}
GELF_OPTS = [dict(), dict(tile_cap=4096, lines_per_group=16), dict(tile_cap=24576, lines_per_group=64), dict(gelf_generic=True),
             dict(gelf_window_kib=2), dict(gelf_window_kib=6)]
SD_OPTS = [dict(), dict(sd_pairs=True), dict(sd_walk=True), dict(force_head=True), dict(force_head=True, tile_cap=6144), dict(no_head=True),
           dict(sd_pairs=True, tile_cap=4096)]
FUSED_OPTS = {E.GELF: [dict(), dict(gelf_generic=True)], E.SD: [dict(), dict(sd_pairs=True), dict(sd_walk=True)]}
# the line length the fused launches are planned for: that of each format's everyday corpus, whatever the stream's own average -- a
# stream of long RFC5424 lines would otherwise be declined (FG_ERR_UNSUPPORTED: its resident kernel stages heads only) and a line
# longer than the tile takes the stage-on steps and the forward scan
FUSED_AVG = {E.GELF: 300, E.SD: 254}
LEDGER: Counter = Counter()  # (format, class, route) -> lines decoded and compared
_REF: dict = {}


def ident(opts: dict) -> str:
    return ",".join(f"{k}={v}" for k, v in opts.items()) or "default"


def tally(s: E.Stream, route: str):
    LEDGER[(s.fmt, s.cls + (" (bail)" if s.bail else ""), route)] += len(s.hz)


def report(fmt: str):
    for k in sorted(k for k in LEDGER if k[0] == fmt):
        print(k, LEDGER[k])


def reference(oracle, dec, s: E.Stream):
    """the oracle's Records of a stream's bare lines, computed once"""
    if s.name not in _REF:
        data = np.frombuffer(s.raw + b"\0" * 64, np.uint8).copy()
        offsets = np.array(s.offsets, np.uint64)
        _REF[s.name] = (data, offsets) + tuple(oracle.decode_batch(dec.fmt, data, offsets, None))
    return _REF[s.name]


def bare_streams(oracle, fmt: str, opts: dict):
    dec = DECODER[fmt]()
    dec.set_launch_opts(**opts)
    for s in E.streams(fmt, E.NONE):
        data, offsets, oblob, ooffs = reference(oracle, dec, s)
        tables, _, _ = device_path(dec, data, offsets)
        blob, offs = tables.to_host().serialize(dec.fmt, data, offsets, cfg=dec._cfg)
        try:
            assert_same(blob, offs, oblob, ooffs, s.lines())
        except AssertionError as e:
            raise AssertionError(f"{s.name} [{ident(opts)}]: {str(e)[:1500]}") from None
        tally(s, "decode " + ident(opts))
    report(fmt)


@pytest.mark.parametrize("opts", GELF_OPTS, ids=ident)
def test_gelf_every_class(oracle, opts):
    """k_gelf at its constant and its run-time geometries, every register window, and k_gelf_general for whatever a tile hands back"""
    bare_streams(oracle, E.GELF, opts)


def test_gelf_batch_whose_average_line_is_longer_than_ten_kib(oracle):
    """what the `round-up` stream found: a GELF batch with an average line above ~10 KiB makes launch_geometry settle on one line per
    group; fg_launch_gelf's search for the lines per group that fit its LDS budget then halved that one to zero and the next
    launch_geometry divided by it (SIGFPE on the host).  Four lines of 12 KiB, alone."""
    from flowgger_amd import synth

    dec = GelfDecoder()
    lines = [b'{"host":"h%d","s":"' % i + b"y" * 12288 + b'\\\\","t":%d}' % i for i in range(4)]
    data, offsets = synth.pack(lines)
    oblob, ooffs = oracle.decode_batch(dec.fmt, data, offsets, None)
    tables, _, _ = device_path(dec, data, offsets)
    blob, offs = tables.to_host().serialize(dec.fmt, data, offsets, cfg=dec._cfg)
    assert_same(blob, offs, oblob, ooffs, lines)


@pytest.mark.parametrize("opts", SD_OPTS, ids=ident)
def test_rfc5424_every_class(oracle, opts):
    """the pair-parallel walk and the lane-per-line walker, whole lines and HEAD rows (with the second look behind the cut)"""
    bare_streams(oracle, E.SD, opts)


def frames_then_decode(dec, raw: bytes, framing: int, n_want: int):
    import torch

    dev = torch.device("cuda", dec.device)
    fill = 0x0A if framing == L.FG_FRAME_LINE else 0
    host = np.full(((len(raw) + 15) & ~15) + 32, fill, np.uint8)
    host[: len(raw)] = np.frombuffer(raw, np.uint8)
    d_bytes = torch.from_numpy(host).to(dev)[: len(raw)]
    d_off, d_bad, n = dec.frame_device(d_bytes, framing, cap_frames=n_want + 16)
    assert n == n_want
    tables = DeviceTables(n, len(raw) // 4 + 4096, dev)
    dec.decode_frames_device(d_bytes, d_off, n, tables, framing, d_bad)
    torch.cuda.synchronize(dev)
    return tables.to_host(), d_off[: n + 1].cpu().numpy().astype(np.uint64)


def pinned_batch(dec, raw: bytes, framing: int):
    lib = L.lib()
    p = C.c_void_p()
    L.check(lib.fg_alloc_pinned(len(raw) + 64, C.byref(p)), "fg_alloc_pinned")
    try:
        buf = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (len(raw) + 64,))
        buf[:] = 0x0A if framing == L.FG_FRAME_LINE else 0
        buf[: len(raw)] = np.frombuffer(raw, np.uint8)
        st = L.fg_tables()
        off = C.c_void_p()
        nf, used = C.c_uint64(), C.c_uint64()
        L.check(lib.fg_frame_decode_batch(dec._ctx, dec.fmt, framing, p, len(raw), 1, C.byref(st), C.byref(off), C.byref(nf), C.byref(used)),
                "fg_frame_decode_batch")
        n = int(nf.value)
        offs = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), (n + 1,)).copy()
        return HostTables.from_struct(st), offs, n, int(used.value), dec.last_host_path()
    finally:
        lib.fg_free_pinned(p)


@pytest.mark.parametrize("framing", [E.LINE, E.NUL], ids=["line", "nul"])
@pytest.mark.parametrize("fmt", [E.GELF, E.SD])
def test_framed_routes(oracle, fmt, framing):
    """the streams with a terminator behind every line: framed and decoded by separate kernels, by the fused kernels (which stage byte
    tiles that start anywhere: the `fine` stream is ordered so that every run meets every residue of their words all the same,
    escape_hazards.fused_residue) and by one pinned fg_frame_decode_batch"""
    dec = DECODER[fmt]()
    fr = L.FG_FRAME_LINE if framing == E.LINE else L.FG_FRAME_NUL
    paths = Counter()
    for s in E.streams(fmt, framing):
        starts, ends, valid = expected_frames(oracle, s.raw, fr, True)
        assert [int(x) for x in starts] == s.offsets[:-1] and bool(valid.all())

        def check(tab, offs, ctx):
            try:
                check_rows(oracle, dec.fmt, None, dec._cfg, s.raw, fr, starts, ends, valid, tab, offs)
            except AssertionError as e:
                raise AssertionError(f"{s.name} {ctx}: {str(e)[:1500]}") from None

        tab, offs = frames_then_decode(dec, s.raw, fr, len(starts))
        check(tab, offs, "frame + decode")
        tally(s, "frame + decode")
        for opts in FUSED_OPTS[fmt]:
            dec.set_launch_opts(**opts)
            tables, offs, n = run_device(dec, s.raw, fr, True, avg_line=FUSED_AVG[fmt], cap=len(starts) + 64)
            assert n == len(starts), f"{s.name} fused [{ident(opts)}]: {n} frames, the oracle has {len(starts)}"
            check(tables.to_host(), offs, f"fused [{ident(opts)}]")
            tally(s, "fused " + ident(opts))
        dec.set_launch_opts()
        tab, offs, n, used, path = pinned_batch(dec, s.raw, fr)
        assert n == len(starts) and used == len(s.raw)
        check(tab, offs, "pinned batch")
        tally(s, "pinned batch")
        paths[path] += 1
    print("fg_frame_decode_batch took FG_PATH", dict(paths))
    report(fmt)
