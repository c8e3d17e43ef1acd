"""What the Kafka message-set core (flowgger_amd/csrc/fg_kafka.hpp) is run through in the tests: the core on the wave emulation
(tests/native/kafka_host.cpp) behind a small class, and the case list.  The reference for every byte is tests/kafka_wire.py."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

import kafka_wire as kw

HERE = Path(__file__).resolve().parent / "native"
ROOT = HERE.parent.parent
CSRC = ROOT / "flowgger_amd" / "csrc"
LIB = HERE / "libkafka_host.so"
SRC = [HERE / "kafka_host.cpp", HERE / "kafka_driver.hpp", HERE / "fg_wave_emu.hpp", CSRC / "fg_kafka.hpp", CSRC / "fg_deflate.hpp", CSRC / "fg_inflate.hpp",
       CSRC / "fg_wave.hpp"]
ROW_MAX, PIECE = 4096, 16384  # fg::kafka::kRowMax, kPiece (KafkaHost checks them)


def build() -> Path:
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRC):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", f"-I{CSRC}", f"-I{HERE}", "-o", str(LIB),
                        str(HERE / "kafka_host.cpp")], check=True)
    return LIB


def aligned(nbytes: int, fill: int = 0) -> np.ndarray:
    """nbytes + 16 bytes of uint8 that start on a 64-byte boundary"""
    raw = np.full(nbytes + 16 + 64, fill, np.uint8)
    at = (-raw.ctypes.data) % 64
    return raw[at:at + nbytes + 16]


def pack(values):
    """-> (bytes as uint8 on a 64-byte boundary with 16 bytes of padding behind them, offsets[n + 1])"""
    off = np.zeros(len(values) + 1, np.uint64)
    off[1:] = np.cumsum([len(v) for v in values], dtype=np.uint64) if values else 0
    blob = aligned(int(off[-1]))
    blob[:int(off[-1])] = np.frombuffer(b"".join(values), np.uint8)
    return blob, off


def skip_array(skip, n):
    return None if skip is None else np.array([1 if s else 0 for s in skip], np.uint8).reshape(n)


class KafkaHost:
    """the core on the wave emulation (tests/native/kafka_host.cpp)"""

    def __init__(self):
        self.lib = L = C.CDLL(str(build()))
        L.fgk_overhead.restype = L.fgk_row_max.restype = L.fgk_piece.restype = C.c_uint32
        L.fgk_bound.restype = L.fgk_messageset.restype = L.fgk_wrap.restype = C.c_uint64
        L.fgk_bound.argtypes = [C.c_uint64] * 3
        L.fgk_messageset.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        L.fgk_wrap.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        L.fgk_cuts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
        L.fgk_cuts.restype = None
        assert (int(L.fgk_overhead()), int(L.fgk_row_max()), int(L.fgk_piece())) == (kw.OVERHEAD, ROW_MAX, PIECE)

    def bound(self, nbytes, n, n_members):
        return int(self.lib.fgk_bound(nbytes, n, n_members))

    def messageset_raw(self, blob, nbytes, off, skip):
        """-> (set as uint8 of exactly the total, set_offsets[n + 1]); None for refused offsets.  The buffer handed over holds exactly
        the total, with sentinel bytes behind it that must survive"""
        n = len(off) - 1
        sk = skip.ctypes.data if skip is not None else None
        so = np.zeros(n + 1, np.uint64)
        total = int(self.lib.fgk_messageset(blob.ctypes.data, nbytes, off.ctypes.data, sk, n, None, 0, so.ctypes.data))
        if total == 2**64 - 1:
            return None
        out = aligned(total + 16, 0xEE)
        so2 = np.zeros(n + 1, np.uint64)
        assert int(self.lib.fgk_messageset(blob.ctypes.data, nbytes, off.ctypes.data, sk, n, out.ctypes.data, total, so2.ctypes.data)) == total
        assert np.array_equal(so, so2) and (out[total:] == 0xEE).all(), "bytes written behind the set"
        return out[:total].copy(), so

    def messageset(self, values, skip=None):
        blob, off = pack(values)
        return self.messageset_raw(blob, int(off[-1]), off, skip_array(skip, len(values)))

    def wrap_raw(self, z, z_off):
        nm = len(z_off) - 1
        wo = np.zeros(nm + 1, np.uint64)
        total = int(self.lib.fgk_wrap(z.ctypes.data, z_off.ctypes.data, nm, None, 0, wo.ctypes.data))
        if total == 2**64 - 1:
            return None
        out = aligned(total + 16, 0xEE)
        wo2 = np.zeros(nm + 1, np.uint64)
        assert int(self.lib.fgk_wrap(z.ctypes.data, z_off.ctypes.data, nm, out.ctypes.data, total, wo2.ctypes.data)) == total
        assert np.array_equal(wo, wo2) and (out[total:] == 0xEE).all(), "bytes written behind the wrappers"
        return out[:total].copy(), wo

    def wrap(self, members):
        z, z_off = pack(members)
        return self.wrap_raw(z, z_off)

    def cuts(self, set_off, member_first):
        set_off, member_first = np.ascontiguousarray(set_off, np.uint64), np.ascontiguousarray(member_first, np.uint64)
        out = np.zeros(len(member_first), np.uint64)
        self.lib.fgk_cuts(set_off.ctypes.data, member_first.ctypes.data, len(set_off) - 1, len(member_first) - 1, out.ctypes.data)
        return out


# ---- the cases.  A value's copy is cut by its DESTINATION: up to 15 head bytes to a 16-byte boundary, quads, up to 15 tail bytes; a lane
# of a row takes ceil(quads / 16) quads, so the chunk grows where the quads pass a multiple of 16 -- value lengths 256 k .. 256 k + 15,
# whatever the head --, a row takes a value up to ROW_MAX and the wave (64 lanes, the chunk grows every 1024 bytes) a longer one.
def _around(points, reach=2, span=15):
    return sorted({n for p in points for n in range(max(0, p - reach), p + span + reach + 1)})


# (every row boundary: the chunk c = 1 .. 16, so every entry of the LDS power table is read; every wave boundary from the switch up to
#  c = 17, the first the wave computes for itself)
LENGTHS = sorted(set([0, 1] + list(range(2, 131)) + _around([256 * k for k in range(1, 17)]) + [255, 256, 257] + list(range(ROW_MAX - 17, ROW_MAX + 2))))
LENGTHS_LONG = sorted(set(_around([ROW_MAX], 2, 17) + _around([1024 * k for k in range(4, 18)]) + [65535, 65536, 65537]))
LONGEST = (1 << 20) + 3


def values_of(lengths, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in lengths]


def alignment_batch(align: int, lengths=LENGTHS):
    """row 0 is `align` bytes, so that the next value starts at source alignment `align` (the buffer itself starts on a boundary) and, when
    row 0 is skipped, at destination 26; every length follows, destinations at every alignment as the sizes add up"""
    return values_of([align] + list(lengths), 7000 + align)


SKIPS = ("null", "none", "first", "last", "middle", "all")


def skip_case(name: str, n: int):
    if name == "null":
        return None
    s = [False] * n
    if name == "first":
        s[0] = True
    elif name == "last":
        s[-1] = True
    elif name == "middle":
        for i in range(n // 3, min(n, n // 3 + 5)):
            s[i] = True
    elif name == "all":
        s = [True] * n
    return s


WRAP_LENGTHS = [1, 25, PIECE - 1, PIECE, PIECE + 1, 5 * PIECE + 7]


def wrap_members():
    """gzip members' bytes as far as the wrap cares (any bytes), an empty one between two others"""
    vals = values_of(WRAP_LENGTHS, 99)
    return vals[:2] + [b""] + vals[2:]


def expect_wrapped(members):
    return b"".join(kw.wrapper(m) for m in members if m)
