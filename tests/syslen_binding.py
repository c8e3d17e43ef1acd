"""ctypes binding of tests/native/libsyslen_host.so: the octet-counted framer's device logic (flowgger_amd/csrc/fg_syslen.hpp)
compiled for the CPU over the fiber emulation of a wavefront, plus the sequential walk it must reproduce (test infrastructure)."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent / "native"
ROOT = HERE.parent.parent
LIB = HERE / "libsyslen_host.so"
SRC = [HERE / "syslen_host.cpp", HERE / "fg_wave_emu.hpp", ROOT / "flowgger_amd" / "csrc" / "fg_syslen.hpp",
       ROOT / "flowgger_amd" / "csrc" / "fg_wave.hpp", ROOT / "flowgger_amd" / "csrc" / "fg_syslen_parse.hpp", ROOT / "flowgger_amd" / "csrc" / "fg_utf8.hpp"]

CLEAN, TAIL, BAD_LEN, LONG_PREFIX, VALID = range(5)
U64_MAX = (1 << 64) - 1


def build() -> Path:
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRC):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        f"-I{ROOT / 'include'}", f"-I{HERE}", f"-I{ROOT / 'flowgger_amd' / 'csrc'}", "-o", str(LIB),
                        str(HERE / "syslen_host.cpp")], check=True)
    return LIB


def read_msglen(buf: bytes, p: int, bound: int | None = None):
    """read_msglen of syslen_splitter.rs:17-25 at position p of a chunk, restated: -> (status, prefix length, payload length).
    The text before the first ' ' is usize::from_str: an optional '+', at least one ASCII digit, nothing else, below 2^64."""
    n = len(buf)
    if p >= n:
        return CLEAN, 0, 0
    sp = buf.find(b" ", p)
    end = n if sp < 0 else sp
    text = buf[p:end]
    body = text[1:] if text[:1] == b"+" else text
    bad = next((k for k, c in enumerate(body) if not 0x30 <= c <= 0x39), None)
    if bad is not None:  # a byte that is neither a digit nor the ' ': no length, wherever the ' ' is
        k = bad + (len(text) - len(body))
        if bound is None or k < bound:
            return BAD_LEN, 0, 0
        return LONG_PREFIX, 0, 0
    if bound is not None and len(text) >= bound:
        return LONG_PREFIX, 0, 0
    if sp < 0:
        return TAIL, 0, 0
    if not body or int(body) > U64_MAX:
        return BAD_LEN, len(text) + 1, 0
    ln = int(body)
    return (VALID if p + len(text) + 1 + ln <= n else TAIL), len(text) + 1, ln


def walk(buf: bytes, bound: int | None = None):
    """the sequential chain: -> (frame starts, prefix lengths, payload lengths, consumed, stop reason)"""
    pos, starts, plens, lens = 0, [], [], []
    while True:
        st, pl, ln = read_msglen(buf, pos, bound)
        if st != VALID:
            return starts, plens, lens, pos, st
        starts.append(pos)
        plens.append(pl)
        lens.append(ln)
        pos += pl + ln


def valid_utf8(b: bytes) -> bool:
    try:
        b.decode("utf-8")
        return True
    except UnicodeDecodeError:
        return False


class SyslenHost:
    def __init__(self):
        self.lib = C.CDLL(str(build()))
        self.lib.fgs_last_error.restype = C.c_char_p
        self.lib.fgs_tile.restype = C.c_uint32
        self.lib.fgs_max_prefix.restype = C.c_uint32
        self.tile = self.lib.fgs_tile()
        self.max_prefix = self.lib.fgs_max_prefix()

    def parse(self, buf: bytes, p: int, bound: int | None = None):
        out = (C.c_uint64 * 3)()
        self.lib.fgs_parse(buf, C.c_uint64(len(buf)), C.c_uint64(p), C.c_uint64(U64_MAX if bound is None else bound), out)
        return int(out[0]), int(out[1]), int(out[2])

    def utf8_bad(self, b: bytes) -> bool:
        return bool(self.lib.fgs_utf8_bad(b, C.c_uint64(len(b))))

    def frame(self, buf: bytes, cap: int | None = None):
        """-> dict(declined, stop, n, consumed, packed, offsets, starts, bad): the four stages, tile by tile"""
        n = len(buf)
        data = np.zeros((n + 15) // 16 * 16 + 16, np.uint8)
        data[:n] = np.frombuffer(buf, np.uint8)
        cap = n // 2 + 1 if cap is None else cap
        packed = np.full(data.size + 16, 0xEE, np.uint8)
        offsets = np.full(cap + 1, U64_MAX, np.uint64)
        starts = np.full(cap + 1, U64_MAX, np.uint64)
        bad = np.zeros(max(cap, 1), np.uint8)
        hdr = np.zeros(16, np.uint32)
        rc = self.lib.fgs_frame(C.c_void_p(data.ctypes.data), C.c_uint64(n), C.c_void_p(packed.ctypes.data), C.c_void_p(offsets.ctypes.data),
                                C.c_void_p(starts.ctypes.data), C.c_void_p(bad.ctypes.data), C.c_uint64(cap), C.c_void_p(hdr.ctypes.data))
        if rc != 0:
            raise RuntimeError(self.lib.fgs_last_error().decode())
        if hdr[0]:
            return {"declined": int(hdr[0])}
        assert hdr[5] == 1, "no node ended the chain"
        k = int(hdr[2])
        return {"declined": 0, "stop": int(hdr[1]), "n": k, "consumed": int(hdr[3]), "total": int(hdr[4]), "packed": packed,
                "offsets": offsets[:min(k, cap) + 1], "starts": starts[:min(k, cap) + 1], "bad": bad[:min(k, cap)]}
