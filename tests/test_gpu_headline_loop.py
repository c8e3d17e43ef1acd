"""GPU: the streaming loop of the RFC5424 headline kernel (fg_pipeline.hpp persistent_loop) after its memory waits moved.

The terminator strip reads the line's last bytes from the tile (from global memory only for the one line longer than the tile), the
next group's geometry is computed before the deferred row is stored, and the stores and the next window's loads go out back to back.
None of it may change a byte: every case below is compared with the oracle's canonical Records, byte for byte, as
tests/test_gpu_parity.py does."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from flowgger_amd import RFC5424Decoder, synth
from flowgger_amd import _lib as L
from flowgger_amd.tables import DeviceTables
from golden.reference_vectors import RFC5424
from gpu_util import assert_same

pytestmark = pytest.mark.gpu

OK = b"<13>1 2015-08-05T15:53:45Z h a p m - x"
BIG = b"<165>1 2003-10-11T22:14:15.003Z big.example.com app 77 ID9 - " + b"m" * 40960  # longer than any tile (40 KiB of message)
FRAMINGS = {"none": L.FG_FRAME_NONE, "line": L.FG_FRAME_LINE, "nul": L.FG_FRAME_NUL}
ROOT = Path(__file__).resolve().parent.parent
PLAN_SRC, PLAN_LIB = ROOT / "tests/native/plan_host.cpp", ROOT / "tests/native/libplan_host.so"
WAVE = 64  # lines a group holds at most


def planned_chunks(n, nbytes, cus, tile_cap=0, chunk_lines=0, static_chunks=False):
    """(chunk, chunks, blocks) of the short-line RFC5424 launch at ONE wave per CU, from the library's own host arithmetic
    (fg_plan_policy.hpp through tests/native/plan_host.cpp): the launch's geometry as fg_launch_rfc5424 asks for it, the grid that
    plan_launch (fg_pipeline.hpp) caps by the groups, then fg::plan_chunks.  One wave per CU only: there the grid
    does not depend on what the occupancy query answers.  The tests assert on it that a wave really runs the loop they are about --
    a batch this size that the plan cut into one group per wave would pass without ever reaching the prefetch."""
    deps = [PLAN_SRC, ROOT / "flowgger_amd/csrc/fg_plan_policy.hpp", ROOT / "include/fg_hip.h"]
    if not PLAN_LIB.exists() or PLAN_LIB.stat().st_mtime < max(d.stat().st_mtime for d in deps):
        subprocess.run(["g++", "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-o", str(PLAN_LIB), str(PLAN_SRC)], check=True)
    lib = C.CDLL(str(PLAN_LIB))
    u64, u32 = C.c_uint64, C.c_uint32
    lib.fgp_plan_chunks.argtypes = [u64, u64, u32, u64, u64, u32, u32, u32, u32, C.POINTER(u64)]
    lib.fgp_rfc5424_walk_geometry.argtypes = [u64, u64, u32, u32, C.POINTER(u64)]
    lib.fgp_pick_variant.argtypes = [u64, u32]
    avg = (nbytes + n - 1) // n
    assert lib.fgp_pick_variant(avg, 0) == 0  # the short-line whole-line kernel: k_rfc5424<20, false, false, false>
    geo = (u64 * 8)()
    lib.fgp_rfc5424_walk_geometry(n, avg, tile_cap, 0, geo)
    lines, groups, full, g, ticket_from, taper = (int(geo[k]) for k in (0, 3, 4, 5, 6, 7))
    assert lines == WAVE
    out = (u64 * 7)()
    lib.fgp_plan_chunks(n, min(cus, groups), lines, g, full, ticket_from, L.FG_LO_STATIC_CHUNKS if static_chunks else 0, chunk_lines, taper, out)
    return int(out[0]), int(out[1]), int(out[2])


def compute_units(dec):
    import torch

    return torch.cuda.get_device_properties(dec.device).multi_processor_count


def stripped(frame: bytes, framing: str) -> bytes:
    """What the decoder sees of a frame: BufRead::lines() strips "\\n", then one "\\r"; split(0) strips the NUL."""
    if framing == "line" and frame.endswith(b"\n"):
        frame = frame[:-1]
        if frame.endswith(b"\r"):
            frame = frame[:-1]
    elif framing == "nul" and frame.endswith(b"\0"):
        frame = frame[:-1]
    return frame


def strip_frames(framing: str):
    """4 000 cfg2 lines framed for `framing`, with the hand-placed frames the strip can go wrong on."""
    term = {"none": b"", "line": b"\n", "nul": b"\0"}[framing]
    base = synth.rfc5424_lines(4000, cfg=2)
    frames = [ln + (b"\r\n" if framing == "line" and i % 7 == 0 else term) for i, ln in enumerate(base)]
    frames[0] = OK + (b"\0" if framing == "nul" else b"\r\n")  # the first line carries a terminator
    frames[100] = term                                          # an empty line
    frames[101] = b"\r" + term                                  # a line that is only "\r"
    frames[102] = OK + b"\r\r\n"                                # "\r\r\n": one "\n" and ONE "\r" go
    frames[1000] = BIG + b"\r\n"                                # the oversize line, a group of its own, read from global memory
    frames[2500] = BIG + b"\0"
    frames[3998] = b"x" + term
    frames[3999] = term if term else b"-"                       # a 1-byte last line
    return frames


_cache = {}


def strip_case(framing, oracle):
    """(frames, device-ready arrays, the oracle's Records of the stripped frames): computed once per framing"""
    if framing not in _cache:
        frames = strip_frames(framing)
        data, offsets = synth.pack(frames)
        bodies = [stripped(f, framing) for f in frames]
        bdata, boffs = synth.pack(bodies)
        _cache[framing] = (frames, data, offsets, oracle.decode_batch(RFC5424, bdata, boffs))
    return _cache[framing]


def decode_frames(dec, data, offsets, framing, launches=1, tables=None):
    """decode_frames_device on HBM-resident frames (no UTF-8 verdicts: the strip and the loop are under test) -> DeviceTables"""
    import torch

    dev = torch.device("cuda", dec.device)
    n, nbytes = len(offsets) - 1, int(offsets[-1])
    d_bytes = torch.cat([torch.from_numpy(np.ascontiguousarray(data[:nbytes])), torch.zeros(32, dtype=torch.uint8)]).to(dev)
    d_offsets = torch.from_numpy(offsets.astype(np.int64)).to(dev)
    if tables is None:
        tables = DeviceTables(n, nbytes // 8 + 1024, dev)
    for _ in range(launches):
        dec.decode_frames_device(d_bytes[:nbytes], d_offsets, n, tables, FRAMINGS[framing])
    return tables, (d_bytes, d_offsets)


def check(tables, dec, data, offsets, want, lines):
    import torch

    torch.cuda.synchronize(torch.device("cuda", dec.device))
    blob, offs = tables.to_host().serialize(RFC5424, data, offsets)
    assert_same(blob, offs, want[0], want[1], lines)


@pytest.mark.parametrize("knobs", [{}, {"tile_cap": 2048}, {"waves_per_cu": 1}, {"static_chunks": True},
                                   {"tile_cap": 2048, "waves_per_cu": 1}, {"waves_per_cu": 1, "chunk_lines": 16}],
                         ids=lambda k: ",".join(f"{a}={b}" for a, b in k.items()) or "default")
@pytest.mark.parametrize("framing", ["none", "line", "nul"])
def test_strip_and_geometry(oracle, framing, knobs):
    """Every framing x launch shape: the last bytes come from the tile for the lines that lie there -- the first of a tile, the
    last, empty ones, one-byte ones -- and from global memory for the 40 KiB line, whose group holds nothing else.
    4 000 lines of 254 B are about as many 17 KiB groups as the plan starts waves, so under the first four shapes most waves run ONE
    group (tile_cap=2048: two or three).  The last two shapes make every wave go round the loop: a 2 KiB tile at one wave per CU is
    16 lines per wave in groups of at most seven; chunks of 16 lines at one wave per CU are several chunks per wave, a group each --
    so the oversize line's neighbours are prefetched behind it and stored in front of it by the same wave."""
    frames, data, offsets, want = strip_case(framing, oracle)
    dec = RFC5424Decoder()
    dec.set_launch_opts(**knobs)
    if knobs.get("waves_per_cu") and len(knobs) > 1:
        chunk, chunks, blocks = planned_chunks(len(frames), int(offsets[-1]), compute_units(dec), knobs.get("tile_cap", 0),
                                               knobs.get("chunk_lines", 0))
        if "chunk_lines" in knobs:
            assert chunk == 16 and chunks >= 2 * blocks, (chunk, chunks, blocks)  # several chunks per wave
        else:
            assert chunk * 192 > 2048 and chunk >= 12, (chunk, chunks, blocks)  # a wave's lines (>= 192 B each) are several tiles
    tables, keep = decode_frames(dec, data, offsets, framing)
    check(tables, dec, data, offsets, want, frames)


def short_lines(n):
    return [OK + b"y" * (i % 7) for i in range(n)]


def test_batches_of_one_group_per_wave(oracle):
    """Up to 513 short lines: the plan gives every wave ONE group of at most 64 lines (a batch this small is cut into one average
    group per wave), so the loop body runs once and every row leaves in the epilogue, nowhere else."""
    dec = RFC5424Decoder()
    for n in (1, 63, 64, 65, 255, 256, 257, 513):
        lines = short_lines(n)
        data, offsets = synth.pack(lines)
        tables, keep = decode_frames(dec, data, offsets, "none")
        check(tables, dec, data, offsets, oracle.decode_batch(RFC5424, data, offsets), lines)


@pytest.mark.parametrize("static_chunks", [False, True], ids=["tickets", "round-robin"])
@pytest.mark.parametrize("chunk_lines", [65, 129])
def test_group_and_chunk_edges(oracle, chunk_lines, static_chunks):
    """Chunks of 64 k + 1 short lines at one wave per CU, two chunks per wave and more: a chunk is k groups of 64 lines and a last
    group of ONE line.  A wave stores the deferred row of a full group while it prefetches the one-line window, then stores that row
    and prefetches across the change of chunk (drawn by ticket, or dealt round-robin).  The plan keeps a named chunk size only when
    the batch holds two such chunks per wave (fg_plan_policy.hpp), hence the batch of 2 x chunk x CUs lines and a ragged rest; 64
    lines of at most 44 B are 2.8 KiB, inside the smallest tile (4 KiB), so groups are cut by lines."""
    dec = RFC5424Decoder()
    dec.set_launch_opts(waves_per_cu=1, chunk_lines=chunk_lines, static_chunks=static_chunks)
    cus = compute_units(dec)
    lines = short_lines(cus * 2 * chunk_lines + 37)
    data, offsets = synth.pack(lines)
    chunk, chunks, blocks = planned_chunks(len(lines), int(offsets[-1]), cus, chunk_lines=chunk_lines, static_chunks=static_chunks)
    assert chunk == chunk_lines and chunk % WAVE == 1 and chunks >= 2 * blocks, (chunk, chunks, blocks)
    tables, keep = decode_frames(dec, data, offsets, "none")
    check(tables, dec, data, offsets, oracle.decode_batch(RFC5424, data, offsets), lines)


def test_a_batch_of_invalid_lines_only(oracle):
    """No line of the batch stays on the fast path: every group runs the byte-wise routes over the tile while the next group's
    window is in flight.  Chunks of 128 lines at one wave per CU: two groups to the chunk, two chunks per wave and more."""
    inv = [s.encode() for s in synth.rfc5424_invalid_lines()]
    dec = RFC5424Decoder()
    dec.set_launch_opts(waves_per_cu=1, chunk_lines=128)
    cus = compute_units(dec)
    lines = [inv[i % len(inv)] for i in range(cus * 256 + 5)]
    data, offsets = synth.pack(lines)
    chunk, chunks, blocks = planned_chunks(len(lines), int(offsets[-1]), cus, chunk_lines=128)
    assert chunk == 128 and chunks >= 2 * blocks, (chunk, chunks, blocks)
    tables, keep = decode_frames(dec, data, offsets, "none")
    check(tables, dec, data, offsets, oracle.decode_batch(RFC5424, data, offsets), lines)


def test_rows_of_back_to_back_launches(oracle):
    """The row stores are no longer waited for inside the loop: two launches back to back on one stream into the SAME tables and a
    third into fresh ones right behind them, nothing synchronised in between, then one launch on its own -- the three tables are
    equal, and they are the oracle's."""
    import torch

    frames, data, offsets, want = strip_case("line", oracle)
    dec = RFC5424Decoder()
    twice, keep_a = decode_frames(dec, data, offsets, "line", launches=2)
    fresh, keep_b = decode_frames(dec, data, offsets, "line")
    torch.cuda.synchronize(torch.device("cuda", dec.device))
    alone, keep_c = decode_frames(dec, data, offsets, "line")
    for tables in (twice, fresh, alone):
        check(tables, dec, data, offsets, want, frames)
    for name in ("meta", "ts", "hostname", "appname", "procid", "msgid", "msg", "full_msg", "ent_count"):
        assert bool((twice.column(name) == alone.column(name)).all()) and bool((fresh.column(name) == alone.column(name)).all()), name
