"""ctypes binding of tests/native/libcapnp_frame_host.so: the Cap'n Proto stream framer's device logic
(flowgger_amd/csrc/fg_capnp_frame.hpp) compiled for the CPU over the fiber emulation of a wavefront, the sequential walk of
fg_capnp_next.hpp, the model both must reproduce (CapnpFramer.frame) and the streams the CPU and GPU suites share (test
infrastructure)."""
from __future__ import annotations

import ctypes as C
import struct
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent / "native"
ROOT = HERE.parent.parent
LIB = HERE / "libcapnp_frame_host.so"
CSRC = ROOT / "flowgger_amd" / "csrc"
SRC = [HERE / "capnp_frame_host.cpp", HERE / "fg_wave_emu.hpp", CSRC / "fg_capnp_frame.hpp", CSRC / "fg_capnp_next.hpp", CSRC / "fg_wave.hpp"]

CLEAN, TAIL, TOO_MANY_SEGMENTS, TOO_LARGE = range(4)
U64_MAX = (1 << 64) - 1
MAX_WORDS = 8 << 20


def build() -> Path:
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRC):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        f"-I{ROOT / 'include'}", f"-I{HERE}", f"-I{CSRC}", "-o", str(LIB), str(HERE / "capnp_frame_host.cpp")], check=True)
    return LIB


def model(buf: bytes):
    """CapnpFramer.frame as (offsets of the whole messages + consumed, consumed, stop): the stop is CLEAN when the chunk ends on a
    message boundary, TAIL when a table or a body runs past it, else what ended the connection"""
    from flowgger_amd import CapnpFramer, CapnpStreamError
    try:
        offs, consumed = CapnpFramer.frame(buf)
    except CapnpStreamError as e:
        return [int(x) for x in e.offsets], e.consumed, TOO_MANY_SEGMENTS if str(e).startswith("Too many") else TOO_LARGE
    return [int(x) for x in offs], consumed, CLEAN if consumed == len(buf) else TAIL


def msg(*sizes, fill=b"\0") -> bytes:
    """a message of len(sizes) segments of that many words each, the bodies filled with `fill` repeated"""
    n = len(sizes)
    table = struct.pack(f"<{n + 1}I", n - 1, *sizes)
    table += bytes(-len(table) % 8)
    body = 8 * sum(sizes)
    return table + (fill * (body // len(fill) + 1))[:body]


def node_heavy_stream(words: int = 6000) -> bytes:
    """one message whose body is false candidates, each the table of a single-segment message that ends on a word of its own far
    behind its tile: about one node per two words, beyond any node store sized to a fraction of the words"""
    body = b"".join(struct.pack("<2I", 0, 600 + k) for k in range(words))
    body += bytes(8 * (words + 700))
    return struct.pack("<2I", 0, len(body) // 8) + body + msg(3, fill=b"tail") + msg(0)


def shapes(tile_words: int):
    """name -> stream: the shapes both suites run (tile_words: the words of a tile of the device logic)"""
    t = tile_words
    small = msg(5, fill=b"abcdefgh")
    out = {
        "empty": b"",
        "one_8_byte_message": msg(0),
        "one_tile_long": msg(t - 1, fill=b"x"),
        "message_straddles_a_tile_end": msg(t - 40, fill=b"a") + msg(100, fill=b"b") + small,
        "table_straddles_a_tile_end": msg(t - 4, fill=b"a") + msg(*([3] * 9), fill=b"q") + small,
        "message_spans_three_tiles": small + msg(3 * t + 17, fill=b"long ") + small,
        "two_segments": msg(3, 4, fill=b"2") + small,
        "three_segments": msg(3, 0, 4, fill=b"3") + small,
        "511_segments": small + msg(*([1] * 511), fill=b"s") + small,
        "512_segments_behind_good": small + small + struct.pack("<2I", 511, 0) + bytes(4096),
        "sum_8mi_words_is_a_tail": small + struct.pack("<4I", 1, MAX_WORDS - 5, 5, 0) + bytes(64),
        "sum_8mi_plus_1_is_too_large": small + struct.pack("<4I", 1, MAX_WORDS - 5, 6, 0) + bytes(64),
        "tail_inside_the_table": small + msg(*([2] * 30), fill=b"t")[:64],
        "tail_inside_the_body": small + msg(200, fill=b"t")[:-8],
        "zero_text_bodies": b"".join(msg(k % 50 + 1) for k in range(300)),
        "small_integer_bodies": b"".join(msg(k % 70 + 1, fill=struct.pack("<8I", 0, 1, 2, 0, 1, 3, 0, 2)) for k in range(300)),
        "eight_byte_messages": msg(0) * 1500,
    }
    for k in range(1, 8):
        out[f"{k}_bytes"] = bytes(range(k))
        out[f"{k}_bytes_behind_a_message"] = small + bytes(k)
    return out


def fuzz_stream(rng, n_msgs: int) -> bytes:
    """random message sizes (most small, some past a tile, some multi-segment) with bodies of zero words, small integers and text"""
    fills = [b"\0", struct.pack("<2I", 0, 3), struct.pack("<4I", 1, 2, 0, 0), b"some text, ", struct.pack("<2I", 12, 1)]
    parts = []
    for _ in range(n_msgs):
        segs = 1 if rng.random() < 0.8 else int(rng.integers(2, 6))
        big = rng.random() < 0.05
        sizes = [int(rng.integers(0, 1500 if big else 60)) for _ in range(segs)]
        parts.append(msg(*sizes, fill=fills[int(rng.integers(0, len(fills)))]))
    return b"".join(parts)


class CapnpFrameHost:
    def __init__(self):
        self.lib = C.CDLL(str(build()))
        self.lib.fgcf_last_error.restype = C.c_char_p
        self.lib.fgcf_tile_words.restype = C.c_uint32
        self.lib.fgcf_node_cap.restype = C.c_uint32
        self.lib.fgcf_walk.restype = C.c_uint32
        self.tile_words = self.lib.fgcf_tile_words()

    def node_cap(self, nbytes: int) -> int:
        return int(self.lib.fgcf_node_cap(C.c_uint64(nbytes)))

    @staticmethod
    def _padded(buf: bytes):
        n = len(buf)
        data = np.zeros((n + 15) // 16 * 16 + 16, np.uint8)
        data[:n] = np.frombuffer(buf, np.uint8)
        return data

    def walk(self, buf: bytes):
        """the sequential walk of fg_capnp_next.hpp: (offsets + consumed, consumed, stop)"""
        data, n = self._padded(buf), len(buf)
        cap = n // 8 + 1
        offsets = np.full(cap + 1, U64_MAX, np.uint64)
        k, consumed = C.c_uint64(), C.c_uint64()
        st = self.lib.fgcf_walk(C.c_void_p(data.ctypes.data), C.c_uint64(n), C.c_void_p(offsets.ctypes.data), C.c_uint64(cap), C.byref(k), C.byref(consumed))
        return [int(x) for x in offsets[:k.value + 1]], int(consumed.value), int(st)

    def frame(self, buf: bytes, cap: int | None = None):
        """-> dict(declined, stop, n, consumed, offsets, nodes): the five stages, tile by tile"""
        data, n = self._padded(buf), len(buf)
        cap = n // 8 + 1 if cap is None else cap
        offsets = np.full(cap + 1, U64_MAX, np.uint64)
        hdr = np.zeros(16, np.uint32)
        rc = self.lib.fgcf_frame(C.c_void_p(data.ctypes.data), C.c_uint64(n), C.c_void_p(offsets.ctypes.data), C.c_uint64(cap), C.c_void_p(hdr.ctypes.data))
        if rc != 0:
            raise RuntimeError(self.lib.fgcf_last_error().decode())
        if hdr[0]:
            return {"declined": int(hdr[0]), "nodes": int(hdr[5])}
        assert hdr[4] == 1, "no node ended the chain"
        k = int(hdr[2])
        return {"declined": 0, "stop": int(hdr[1]), "n": k, "consumed": int(hdr[3]) * 8, "offsets": offsets[:min(k, cap) + 1], "nodes": int(hdr[5])}
