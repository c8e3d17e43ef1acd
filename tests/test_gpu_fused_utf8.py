"""The fused frame + decode kernels (flowgger_amd/csrc/fg_fused.hpp: fg_frame_decode_device, the one-launch form of
fg_frame_decode_batch) on streams that hold ONE UTF-8 hazard per staged range, at every boundary where stage A hands a predecessor
dword over (tests/utf8_hazards.py): frame count, every frame start, the UTF-8 verdict of every frame and the Record bytes of every
valid frame against the oracle, exactly.  The same streams are validated without a GPU by tests/test_utf8_hazards_cpu.py."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import utf8_hazards as H
from flowgger_amd import _lib as L
from flowgger_amd.tables import HostTables
from fuse_binding import FuseHost
from test_gpu_round6 import check_rows, expected_frames, make_decoder, run_device

pytestmark = pytest.mark.gpu

FRAMING = {H.LINE: L.FG_FRAME_LINE, H.NUL: L.FG_FRAME_NUL}


@pytest.fixture(scope="module")
def host():
    return FuseHost()


def expected(oracle, raw, framing, final):
    """the oracle's frames (fgo_frame), asserted equal to bytes.decode per frame"""
    starts, ends, valid = expected_frames(oracle, raw, FRAMING[framing], final)
    rs, re_, rv = H.reference_frames(raw, framing, final)
    assert np.array_equal(starts, rs) and np.array_equal(ends, re_) and np.array_equal(valid, rv)
    return starts, ends, valid


def launch_and_check(oracle, dec, cfg, fmt, raw, framing, final, avg_line, ctx, fill=None):
    starts, ends, valid = expected(oracle, raw, framing, final)
    tables, offs, n = run_device(dec, raw, FRAMING[framing], final, avg_line=avg_line, cap=len(starts) + 64, fill=fill)
    assert n == len(starts), f"{ctx}: {n} frames, the oracle has {len(starts)}"
    try:
        check_rows(oracle, fmt, cfg, dec._cfg, raw, FRAMING[framing], starts, ends, valid, tables.to_host(), offs)
    except AssertionError as e:
        raise AssertionError(f"{ctx}: {e}") from None


def describe(raw, made, starts, valid, st):
    """the placements whose frames' verdicts differ (for the failure message)"""
    out = []
    for p in made:
        i = int(np.searchsorted(starts, p.pos - p.cut, side="right")) - 1
        lo, hi = max(i - 1, 0), min(i + 3, len(valid))
        if not np.array_equal((st[lo:hi] == L.FG_ST_BAD_UTF8), valid[lo:hi] == 0):
            out.append(f"{p.cls}[{p.sub}] tile {p.tile} pos {p.pos} {p.kind.name} cut {p.cut}")
    return out


@pytest.mark.parametrize("framing", [H.LINE, H.NUL], ids=["line", "nul"])
@pytest.mark.parametrize("v", H.VARIANTS, ids=[v.name for v in H.VARIANTS])
def test_boundary_classes(oracle, host, v, framing):
    """every kernel variant (k_rfc5424_fused<16> and <12, pairs>, k_ltsv_fused<2>, k_gelf_fused<3, const> and <6>) x framing: the streams
    of utf8_hazards.boundary_streams, one per launch, each at the geometry it was built for -- pinned with set_launch_opts and avg_line,
    predicted with fg::fused_geometry (FuseHost.geometry).  The first row from buffer loads does not exist in RFC5424's and GELF's
    planned tiles (they fit the register windows): the `wide` stream pins a tile that has one; the constant 3 KiB GELF kernel has no
    other geometry and no such row.  About 20 launches and 6 to 17 MB of stream per case (the spacing of S + tile between placements is
    what makes them long, not the number of placements); measured on an MI355X: 0.2 to 0.4 s per case, the whole file 6 s."""
    dec, cfg = make_decoder(v.fmt)
    try:
        for name, g, raw, made, counts in H.boundary_streams(host, v, framing):
            dec.set_launch_opts(**g["opts"])
            ctx = f"{v.name} {name} S={g['S']} look={g['look']} tile={g['tile']} ext={g['ext']}"
            starts, ends, valid = expected(oracle, raw, framing, True)
            tables, offs, n = run_device(dec, raw, FRAMING[framing], True, avg_line=g["avg"], cap=len(starts) + 64)
            assert n == len(starts), f"{ctx}: {n} frames, the oracle has {len(starts)}"
            ht = tables.to_host()
            wrong = describe(raw, made, starts, valid, ht.status[:n]) if np.array_equal(offs[:n], starts) else []
            assert not wrong, f"{ctx}: verdicts differ at {len(wrong)} placements: {wrong[:12]}"
            check_rows(oracle, v.fmt, cfg, dec._cfg, raw, FRAMING[framing], starts, ends, valid, ht, offs)
    finally:
        dec.set_launch_opts()


@pytest.mark.parametrize("framing", [H.LINE, H.NUL], ids=["line", "nul"])
@pytest.mark.parametrize("v", [H.VARIANTS[0], H.VARIANTS[2], H.VARIANTS[4]], ids=["rfc5424", "ltsv", "gelf"])
def test_stream_end(oracle, host, v, framing):
    """streams of two to four tiles that end at every residue mod 16 with a cut or complete sequence, an ASCII byte or a terminator,
    final and not, the end reached inside the last tile's own range, inside the look-ahead of the tile before (two tiles hold it), by a
    staged-on row and by the tail scan; terminators, C3 or 80 behind the end up to the padded length and 16 bytes beyond.  With
    final = 0 the unterminated piece stays with the caller, and a sequence cut in it does not flag the frame before."""
    dec, cfg = make_decoder(v.fmt)
    fill, mk = H.fillers(v.fmt, framing, 200), H.Maker(v.fmt)
    g = H.geometry_of(host, v, H.SMALL)
    dec.set_launch_opts(**g["opts"])
    try:
        for way, residue, final, (ename, ending), garbage in H.end_cases(framing):
            raw = H.end_stream(fill, mk, g, framing, way, residue, ending)
            ctx = f"{v.name} end by {way}, residue {residue}, ends with {ename}, final={final}, {garbage} behind"
            launch_and_check(oracle, dec, cfg, v.fmt, raw, framing, final, g["avg"], ctx, fill=H.garbage_byte(garbage, framing))
    finally:
        dec.set_launch_opts()


@pytest.mark.parametrize("v", H.PLAIN, ids=[v.name for v in H.PLAIN])
def test_one_hazard_per_stream_tile(oracle, host, v):
    """geometry-blind: every line holds one valid multi-byte sequence, whose absolute position walks through all residues mod 1024; one
    line in about S + tile bytes holds a truncated one instead.  The library's own choice of kernel and geometry at three line lengths."""
    dec, cfg = make_decoder(v.fmt)
    mk = H.Maker(v.fmt)
    for avg in H.WALK_AVG:
        g = H.geometry_of(host, v, dict(avg=avg))
        raw, bad_at = H.walking_stream(mk, g, H.LINE)
        launch_and_check(oracle, dec, cfg, v.fmt, raw, H.LINE, True, avg, f"{v.name} avg_line {avg}: {len(bad_at)} truncated sequences")


@pytest.mark.parametrize("v", [H.PLAIN[0], H.PLAIN[2]], ids=["rfc5424", "gelf"])
def test_pinned_route(oracle, host, v):
    """the boundary streams from PINNED memory through fg_frame_decode_batch on a fresh decoder: it plans with its initial experience of
    200 bytes per line, link-bound (stage-on steps of 256 bytes, GELF's 48-line tiles); the route is asserted, so the separate framing
    pass cannot stand in"""
    lib = L.lib()
    g = H.geometry_of(host, v, dict(avg=200), link_bound=True)
    assert g["ext"] == 256
    fill, mk = H.fillers(v.fmt, H.LINE, 3000), H.Maker(v.fmt)
    raw, made, counts = H.build(fill, mk, g, H.planned_wants(g, H.LINE), H.LINE)
    red = H.cuts(H.reduced(H.LINE))
    assert H.covered(made, "row", red, H.rows_of(g, 1) - 1) and H.covered(made, "stage-on", red) and H.covered(made, "tail-scan", red, 4)
    assert H.covered(made, "stage-on", H.all_before(H.LINE), len(H.stage_steps(g)) - 1)
    assert (counts.get("window-edge", 0) > 0) == (v.fmt == H.GELF)  # (six rows of GELF's ten are in registers; RFC5424's tile fits its window)
    dec, cfg = make_decoder(v.fmt)
    p = C.c_void_p()
    L.check(lib.fg_alloc_pinned(len(raw) + 64, C.byref(p)), "fg_alloc_pinned")
    try:
        buf = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (len(raw) + 64,))
        buf[:] = 0x0A
        buf[: len(raw)] = np.frombuffer(raw, np.uint8)
        starts, ends, valid = expected(oracle, raw, H.LINE, True)
        st = L.fg_tables()
        off = C.c_void_p()
        nf, used = C.c_uint64(), C.c_uint64()
        L.check(lib.fg_frame_decode_batch(dec._ctx, v.fmt, L.FG_FRAME_LINE, p, len(raw), 1, C.byref(st), C.byref(off), C.byref(nf), C.byref(used)),
                "fg_frame_decode_batch")
        assert dec.last_host_path() == L.FG_PATH_FRAME_FUSED
        n = int(nf.value)
        assert n == len(starts) and int(used.value) == int(ends[-1])
        offs = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), (n + 1,)).copy()
        ht = HostTables.from_struct(st)
        wrong = describe(raw, made, starts, valid, ht.status[:n]) if np.array_equal(offs[:n], starts) else []
        assert not wrong, f"verdicts differ at {len(wrong)} placements: {wrong[:12]}"
        check_rows(oracle, v.fmt, cfg, dec._cfg, raw, L.FG_FRAME_LINE, starts, ends, valid, ht, offs)
    finally:
        lib.fg_free_pinned(p)


def test_stage_on_rows_shorter_than_a_kib(oracle, host):
    """the stream this file found a bug with: stage-on steps of 256 bytes (fused_ext, and every link-bound launch), a sequence cut by the
    END of a staged-on row.  The hand-over to the next row read lane 63, which holds nothing in a row of 16 chunks: the frame passed as
    valid.  One launch per step, so that nothing else in the stream can raise the tile's error bit."""
    v = H.VARIANTS[0]
    dec, cfg = make_decoder(v.fmt)
    fill, mk = H.fillers(v.fmt, H.LINE, 400), H.Maker(v.fmt)
    g = H.geometry_of(host, v, H.SMALL)
    assert g["ext"] == 256 and len(H.stage_steps(g)) == 5
    dec.set_launch_opts(**g["opts"])
    try:
        for k in H.reduced(H.LINE)[:3]:
            for step in range(4):
                raw, made, _ = H.build(fill, mk, g, [("stage-on", step, k, len(k.data))], H.LINE)
                launch_and_check(oracle, dec, cfg, v.fmt, raw, H.LINE, True, g["avg"], f"{k.name} before stage-on step {step}")
    finally:
        dec.set_launch_opts()


def test_framer_ignores_what_lies_behind_the_end(oracle):
    """the stream this file found a second bug with: a stream that ends with a complete sequence, a continuation byte behind its end in
    the same 16-byte chunk (the caller's memory: readable, and nothing more).  The framing scans judged position nbytes with that
    byte and flagged the last frame.  Every residue, 80 and BF behind the end, a cut sequence (which must stay flagged) as well."""
    import torch

    dec, _ = make_decoder(H.RFC5424)
    dev = torch.device("cuda", dec.device)
    try:
        for classic in (False, True):
            dec.set_launch_opts(frame_classic=classic)
            for r in range(16):
                for tail in ("é".encode(), "€".encode(), b"\xe2\x82", b"z"):
                    for garbage in (0x80, 0xBF):
                        raw = b"first\n" + b"a" * (26 + r - len(tail)) + tail
                        assert len(raw) % 16 == r
                        starts, ends, valid = expected(oracle, raw, H.LINE, True)
                        hostbuf = np.full(64, garbage, np.uint8)
                        hostbuf[: len(raw)] = np.frombuffer(raw, np.uint8)
                        d_offsets, d_bad, n = dec.frame_device(torch.from_numpy(hostbuf).to(dev)[: len(raw)], L.FG_FRAME_LINE)
                        assert n == 2 and d_bad[:2].cpu().numpy().tolist() == (1 - valid).tolist(), (classic, r, tail, garbage)
    finally:
        dec.set_launch_opts()


FRAMER = dict(S=16384, look=256, tile=17408, ext=1024, NB=99, avg=254)  # the separate framer's 16 KiB scan blocks


@pytest.mark.parametrize("framing", [H.LINE, H.NUL], ids=["line", "nul"])
def test_separate_framer_on_the_same_streams(oracle, host, framing):
    """fg_frame.hip (frame_device: the one-pass scan and FG_LO_FRAME_CLASSIC) on the boundary and stream-end streams, and on one built
    for its own 16 KiB scan blocks: every kind x cut at the block edges and at chunk boundaries.  Starts and verdicts against
    reference_frames.  (It judges every frame itself: nothing needs to be kept apart, and the placements are one block apart.)"""
    import torch

    v = H.VARIANTS[0]
    dec, _ = make_decoder(v.fmt)
    dev = torch.device("cuda", dec.device)
    fill, mk = H.fillers(v.fmt, framing, 3000), H.Maker(v.fmt)
    ks = H.kinds(framing)
    utf8 = H.cuts([k for k in ks if k.utf8])
    wants = H.cross("tile", 3, H.cuts([k for k in ks if not k.utf8])) + H.rotate("tile", 3, utf8) + H.rotate("chunk", 8, utf8)
    wanted = H.plan(FRAMER, wants, gap=2048)
    # its own rows: the hand-over of the last dword from one KiB row of a scan block to the next (block base + 1024 r, r = 1 .. 15)
    T = max(p.tile for p in wanted) + 2
    red = H.cuts(H.reduced(framing))
    for i in range(15 * 2):
        k, c = red[i % len(red)]
        wanted.append(H.Placement((T + 2 * i) * 16384 + 1024 * (i % 15 + 1), k, c, "row", tile=T + 2 * i, sub=i % 15 + 1))
    raw, made = H.place(fill, mk, wanted, framing, 2048, tail_fill=40000)
    assert len(made) == len(wanted) and {p.sub for p in made if p.cls == "row"} == set(range(1, 16))
    streams = [("scan blocks", raw, 0x0A)] + [(n, r, 0x80) for n, _, r, _, _ in H.boundary_streams(host, v, framing) if n in ("full", "block", "long-1")]
    g = H.geometry_of(host, v, H.SMALL)
    small_fill = H.fillers(v.fmt, framing, 200)
    for way, residue, final, (ename, ending), garbage in H.end_cases(framing):
        if final:
            streams.append((f"end by {way} residue {residue} {ename}", H.end_stream(small_fill, mk, g, framing, way, residue, ending), H.garbage_byte(garbage, framing)))
    try:
        for classic in (False, True):
            dec.set_launch_opts(frame_classic=classic)
            for name, data, garbage in streams:
                starts, ends, valid = expected(oracle, data, framing, True)
                hostbuf = np.full(((len(data) + 15) & ~15) + 32, garbage, np.uint8)
                hostbuf[: len(data)] = np.frombuffer(data, np.uint8)
                d_bytes = torch.from_numpy(hostbuf).to(dev)
                d_offsets, d_bad, n = dec.frame_device(d_bytes[: len(data)], FRAMING[framing], cap_frames=len(starts) + 16)
                ctx = f"{name} classic={classic}"
                assert n == len(starts), f"{ctx}: {n} frames, the reference has {len(starts)}"
                offs = d_offsets[: n + 1].cpu().numpy().astype(np.uint64)
                assert np.array_equal(offs[:n], starts) and int(offs[n]) == len(data), ctx
                bad = d_bad[:n].cpu().numpy()
                assert np.array_equal(bad, 1 - valid), f"{ctx}: first UTF-8 verdict mismatch at frame {int(np.flatnonzero(bad != 1 - valid)[0])}"
    finally:
        dec.set_launch_opts()
