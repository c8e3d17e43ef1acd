"""The sliced raw-stream route of fg_frame_decode_batch (fg_host_pipeline.cpp frame_decode_sliced -> fg_launch_frame_slice) through
BOTH instantiations of the framing kernels: k_frame_onepass / k_frame_scan reading HBM behind a copy-engine upload, and their COPY
twins reading the caller's pinned chunk over the link and storing it to HBM on the way (FG_LO_FRAME_KERNEL_UPLOAD) -- one-pass and
classic (FG_LO_FRAME_CLASSIC), final and not.  Frame offsets, consumed bytes, the status of every row (bad UTF-8 among them) and the
canonical Record bytes must equal the one-piece route (FG_LO_TRANSCODE_ONE_PIECE: fg_launch_frame over the whole stream, which
tests/test_gpu_round5.py pins to the oracle's splitter) on the same bytes.

One stream just over 48 MiB, the smallest the route accepts; its slices are 8 MiB.  Placed on slice boundaries: a valid three-byte
sequence across 8 MiB, a sequence broken across 16 MiB (its error bit belongs to the first byte of the next slice and depends on the
last dword of the slice before), a delimiter as the last byte before 24 MiB and an empty frame as the first byte behind it; the
stream's length is no multiple of the 128 KiB tile (nor of 16) and it ends in an unterminated piece that a sequence is cut off in."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from flowgger_amd import RFC5424Decoder, synth
from flowgger_amd import _lib as L
from flowgger_amd.tables import HostTables

pytestmark = pytest.mark.gpu

MIB = 1 << 20
NBYTES = 49 * MIB + 12345


def build_stream() -> np.ndarray:
    block = np.frombuffer(b"".join(ln + b"\n" for ln in synth.rfc5424_lines(4000, cfg=2)), np.uint8)
    assert MIB // 2 < block.size < 2 * MIB and block.size // 4000 > 200  # (a fresh ctx sizes the sliced route's tables for lines of 160 bytes or more)
    raw = np.tile(block, NBYTES // block.size + 1)[:NBYTES].copy()
    assert raw.size % (128 << 10) != 0 and raw.size % 16 != 0
    for b in (8 * MIB, 16 * MIB, 24 * MIB):  # (a known neighbourhood: one long run of ASCII inside whatever line lies there)
        raw[b - 64: b + 64] = ord("x")
    raw[8 * MIB - 1: 8 * MIB + 2] = (0xE2, 0x82, 0xAC)
    raw[16 * MIB - 2: 16 * MIB] = (0xE2, 0x82)
    raw[24 * MIB - 1] = raw[24 * MIB] = 0x0A
    raw[-40:] = ord("t")
    raw[-2:] = (0xE2, 0x82)
    return raw


def run(dec, ptr: int, n: int, final: int):
    """fg_frame_decode_batch -> (offsets, consumed, HostTables, path)"""
    st, off, nf, used = L.fg_tables(), C.c_void_p(), C.c_uint64(), C.c_uint64()
    L.check(L.lib().fg_frame_decode_batch(dec._ctx, dec.fmt, L.FG_FRAME_LINE, C.c_void_p(ptr), n, final, C.byref(st), C.byref(off), C.byref(nf), C.byref(used)),
            "fg_frame_decode_batch")
    offs = np.ctypeslib.as_array(C.cast(off, C.POINTER(C.c_uint64)), (int(nf.value) + 1,)).copy()
    return offs, int(used.value), HostTables.from_struct(st), dec.last_host_path()


class Stream:
    def __init__(self):
        self.raw = build_stream()
        n = self.raw.size
        self.pageable = np.concatenate([self.raw, np.zeros(64, np.uint8)])
        self.pinned_ptr = C.c_void_p()
        L.check(L.lib().fg_alloc_pinned(n + 64, C.byref(self.pinned_ptr)), "fg_alloc_pinned")
        pinned = np.ctypeslib.as_array(C.cast(self.pinned_ptr, C.POINTER(C.c_uint8)), (n + 64,))
        pinned[:] = 0x0A  # (what lies behind the chunk is not the stream's)
        pinned[:n] = self.raw
        self.dec = RFC5424Decoder()
        # the reference: the one-piece route, computed once for each `final` and left alone
        self.dec.set_launch_opts(no_fused_framing=True, transcode_one_piece=True)
        self.ref = {}
        for final in (0, 1):
            offs, consumed, tab, path = run(self.dec, self.pageable.ctypes.data, n, final)
            assert path == L.FG_PATH_FRAME_ONE_PIECE
            self.ref[final] = (offs, consumed, tab.status[: offs.size - 1].copy(), self.records(tab, offs))

    def records(self, tab, offs):
        return tab.serialize(self.dec.fmt, self.pageable, np.ascontiguousarray(offs, np.uint64), cfg=self.dec._cfg)

    def close(self):
        self.dec.set_launch_opts()
        L.lib().fg_free_pinned(self.pinned_ptr)


@pytest.fixture(scope="module")
def stream():
    s = Stream()
    yield s
    s.close()


def test_the_reference_holds_what_the_stream_was_built_with(stream):
    offs, consumed, status, _ = stream.ref[1]
    bad = status == L.FG_ST_BAD_UTF8
    frame_of = lambda x: int(np.searchsorted(offs, x, side="right")) - 1
    assert not bad[frame_of(8 * MIB)] and bad[frame_of(16 * MIB)] and frame_of(16 * MIB) == frame_of(16 * MIB - 1)
    i = frame_of(24 * MIB)
    assert int(offs[i]) == 24 * MIB and int(offs[i + 1]) == 24 * MIB + 1  # (the empty frame)
    assert consumed == NBYTES and int(offs[-1]) == NBYTES and bad[-1]  # (final: the tail is a frame, cut off by the end)
    offs0, consumed0, status0, _ = stream.ref[0]
    assert offs0.size == offs.size - 1 and consumed0 == int(offs0[-1]) == int(offs[-2]) and not (status0[-1] == L.FG_ST_BAD_UTF8)


@pytest.mark.parametrize("final", [0, 1])
@pytest.mark.parametrize("classic", [False, True], ids=["onepass", "classic"])
@pytest.mark.parametrize("upload", [False, True], ids=["copy-engine", "kernel-upload"])
def test_sliced_route_equals_the_one_piece_route(stream, upload, classic, final):
    dec = stream.dec
    dec.set_launch_opts(no_fused_framing=True, frame_kernel_upload=upload, frame_classic=classic)
    ptr = stream.pinned_ptr.value if upload else stream.pageable.ctypes.data
    offs, consumed, tab, path = run(dec, ptr, NBYTES, final)
    assert path == L.FG_PATH_FRAME_SLICED
    want_offs, want_consumed, want_status, (want_blob, want_boffs) = stream.ref[final]
    assert offs.size == want_offs.size, f"{offs.size - 1} frames, the one-piece route has {want_offs.size - 1}"
    assert np.array_equal(offs, want_offs), f"frame offsets differ at {int(np.flatnonzero(offs != want_offs)[0])}"
    assert consumed == want_consumed
    status = tab.status[: offs.size - 1]
    assert np.array_equal(status, want_status), f"row status differs at frame {int(np.flatnonzero(status != want_status)[0])}"
    blob, boffs = stream.records(tab, offs)
    assert np.array_equal(boffs, want_boffs) and np.array_equal(blob, want_blob)
