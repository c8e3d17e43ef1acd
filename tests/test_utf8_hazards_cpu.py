"""The hazard streams of tests/utf8_hazards.py without a GPU: the streams meet their own conditions, Python's bytes.decode per frame
(reference_frames) equals the oracle's restatement of the splitters (fgo_frame) on every one of them, and so does the tile-level
framing code (flowgger_amd/csrc/fg_fuse.hpp on the CPU emulation of a wave, FuseHost.frame) at the geometry each stream was built
for.  This validates the inputs and the reference of tests/test_gpu_fused_utf8.py; the kernel loop itself only runs there."""
from __future__ import annotations

import numpy as np
import pytest

import utf8_hazards as H
from fuse_binding import FuseHost
from oracle_binding import Oracle


@pytest.fixture(scope="module")
def host():
    return FuseHost()


@pytest.fixture(scope="module")
def oracle():
    return Oracle()


def reference(oracle, raw: bytes, framing: int, final: bool):
    """reference_frames, asserted equal to the oracle's fgo_frame"""
    s, e, ok = H.reference_frames(raw, framing, True)
    os_, oe, ov = oracle.frame_arrays(np.frombuffer(raw + b"\0", np.uint8)[: len(raw)], "line" if framing == H.LINE else "nul")
    assert np.array_equal(s, os_) and np.array_equal(e, oe) and np.array_equal(ok, ov), "bytes.decode and the oracle disagree"
    return H.reference_frames(raw, framing, final)


def emulate(host, raw, framing, final, g, garbage):
    delim = 0x0A if framing == H.LINE else 0
    return host.frame(raw, delim, final, g["S"], g["look"], g["tile"], g["L"], H.garbage_byte(garbage, framing))


def same(got, want, ctx):
    gs, ge, gb = got[:3]
    ws, we, wv = want
    assert len(gs) == len(ws), f"{ctx}: {len(gs)} frames, the reference has {len(ws)}"
    assert np.array_equal(gs, ws) and np.array_equal(ge, we), ctx
    assert np.array_equal(gb, 1 - wv), f"{ctx}: UTF-8 verdicts differ at frame {int(np.flatnonzero(gb != 1 - wv)[0])}"


def test_kinds_are_what_they_claim():
    for framing in (H.LINE, H.NUL):
        t = H.term_of(framing)
        for k in H.kinds(framing):
            raw = b"ab" + k.data + b"cd" + t
            valid = H.reference_frames(raw, framing, True)[2]
            assert bool((valid == 0).any()) == k.bad, k
            assert k.utf8 == any(b >= 0x80 for b in k.data), k
        assert {k.name for k in H.reduced(framing)} == set(H.REDUCED)


def test_place_refuses_what_lies_too_close():
    fill, mk = H.fillers(H.RFC5424, H.LINE, 50), H.Maker(H.RFC5424)
    k = H.reduced(H.LINE)[0]
    raw, made = H.place(fill, mk, [H.Placement(5000, k, 1), H.Placement(9000, k, 0), H.Placement(40000, k, 2)], H.LINE, 8192)
    assert [p.pos for p in made] == [5000, 40000]
    assert raw[4999:5001] == k.data and raw[39998:40000] == k.data
    with pytest.raises(ValueError):  # (RFC5424's planned tile has no row beyond its register window)
        g = dict(S=14848, look=256, tile=16384, ext=1024, NB=16)
        H.plan(g, [("window-edge", 0, k, 0)])


def test_boundaries_of_the_planned_rfc5424_geometry(host):
    g = H.geometry_of(host, H.VARIANTS[0], None)
    assert (g["S"], g["look"], g["tile"], g["ext"], g["NB"]) == (14848, 256, 16384, 1024, 16)
    b = H.tile_boundaries(g, 2)
    w = 2 * 14848 - 16
    assert [t.pos for t in b["row"]] == [w + 1024 * r for r in range(1, 15)] and b["window-edge"] == []
    assert [t.pos for t in b["stage-on"]] == [w + 15120, w + 16144] and [t.pos for t in b["tail-scan"]] == [w + 16384 + 1024 * j for j in range(4)]
    assert [t.pos for t in b["tile"]] == [2 * 14848 - 1, 2 * 14848, 2 * 14848 + 1] and b["block"] == []
    assert [t.pos for t in H.tile_boundaries(g, 0)["row"]] == [1024 * r for r in range(1, 15)]  # (the first tile's window starts at the stream)
    assert H.tile_boundaries(g, 64)["block"] and all(len(v) for c, v in H.boundaries(g, 4 << 20).items() if c != "window-edge")


@pytest.mark.parametrize("framing", [H.LINE, H.NUL], ids=["line", "nul"])
@pytest.mark.parametrize("v", H.VARIANTS, ids=[v.name for v in H.VARIANTS])
def test_boundary_streams_on_the_emulation(host, oracle, v, framing):
    streams = H.boundary_streams(host, v, framing)
    total = 0
    for i, (name, g, raw, made, counts) in enumerate(streams):
        if not name.startswith("first"):
            print(f"{v.name} framing={framing} {name}: S={g['S']} look={g['look']} tile={g['tile']} ext={g['ext']} NB={g['NB']} "
                  f"{len(raw)} bytes, placements {dict(counts)}")
        total += len(raw)
        scans = 0
        for final, garbage in ((True, H.GARBAGE[i % 3]), (False, H.GARBAGE[(i + 1) % 3])):
            got = emulate(host, raw, framing, final, g, garbage)
            same(got, reference(oracle, raw, framing, final), f"{v.name} {name} final={final}")
            scans += got[5]
        if counts.get("tail-scan"):
            assert scans >= 1, f"{v.name} {name}: no tile needed the forward scan"
    names = [s[0] for s in streams]
    # (the first row from buffer loads: RFC5424's planned tiles fit their register windows -- 15 and 11 rows in 16 and 12 --, so does
    #  GELF's -- 3 in 3 and in 6; a pinned wider tile has such a row; the constant 3 KiB GELF kernel has no other geometry: empty there)
    edge = sum(c.get("window-edge", 0) for _, _, _, _, c in streams)
    assert (edge == 0) == (v.name == "gelf-const")
    assert "full" in names and "block" in names and total < (20 << 20)


@pytest.mark.parametrize("framing", [H.LINE, H.NUL], ids=["line", "nul"])
@pytest.mark.parametrize("v", [H.VARIANTS[0], H.VARIANTS[2], H.VARIANTS[4]], ids=["rfc5424", "ltsv", "gelf"])
def test_stream_ends_on_the_emulation(host, oracle, v, framing):
    fill, mk = H.fillers(v.fmt, framing, 200), H.Maker(v.fmt)
    g = H.geometry_of(host, v, H.SMALL)
    seen = set()
    for way, residue, final, (ename, ending), _ in H.end_cases(framing):
        raw = H.end_stream(fill, mk, g, framing, way, residue, ending)
        assert len(raw) % 16 == residue and 2 <= -(-len(raw) // g["S"]) <= 4
        scans = 0
        for garbage in H.GARBAGE:
            got = emulate(host, raw, framing, final, g, garbage)
            same(got, reference(oracle, raw, framing, final), f"{v.name} {way} residue {residue} ends with {ename} final={final} garbage={garbage}")
            scans += got[5]
            # (the emulation does not stage on: both ways whose last line outruns the look-ahead reach the end through the forward scan)
            assert way not in ("stage-on", "tail-scan") or got[5] >= 1, f"{way}: no tile needed the forward scan"
        seen.add((way, final, ename))
    assert len(seen) == len(H.WAYS) * 2 * len(H.endings(framing))


@pytest.mark.parametrize("v", H.PLAIN, ids=[v.name for v in H.PLAIN])
def test_walking_streams_on_the_emulation(host, oracle, v):
    mk = H.Maker(v.fmt)
    for avg in H.WALK_AVG:
        g = H.geometry_of(host, v, dict(avg=avg))
        raw, bad_at = H.walking_stream(mk, g, H.LINE)
        want = reference(oracle, raw, H.LINE, True)
        assert int((want[2] == 0).sum()) == len(bad_at) >= 10
        same(emulate(host, raw, H.LINE, True, g, 0xC3), want, f"{v.name} avg_line {avg}")
