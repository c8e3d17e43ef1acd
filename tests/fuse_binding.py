"""ctypes binding of tests/native/libfuse_host.so: flowgger_amd/csrc/fg_fuse.hpp (framing inside the decode kernels) compiled for the
CPU over the fiber emulation of a wavefront (test infrastructure)."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent / "native"
ROOT = HERE.parent.parent
LIB = HERE / "libfuse_host.so"
SRC = [HERE / "fuse_host.cpp", HERE / "fg_wave_emu.hpp", ROOT / "flowgger_amd" / "csrc" / "fg_fuse.hpp", ROOT / "flowgger_amd" / "csrc" / "fg_wave.hpp",
       ROOT / "flowgger_amd" / "csrc" / "fg_fused_plan.hpp", ROOT / "flowgger_amd" / "csrc" / "fg_utf8.hpp"]


def build() -> Path:
    if not LIB.exists() or any(s.exists() and s.stat().st_mtime > LIB.stat().st_mtime for s in SRC):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        f"-I{ROOT / 'include'}", f"-I{HERE}", f"-I{ROOT / 'flowgger_amd' / 'csrc'}", "-o", str(LIB), str(HERE / "fuse_host.cpp")],
                       check=True)
    return LIB


class FuseHost:
    def __init__(self):
        self.lib = C.CDLL(str(build()))
        self.lib.fgf_last_error.restype = C.c_char_p
        self.lib.fgf_frame.restype = C.c_long
        self.lib.fgf_plan.restype = C.c_uint32

    def plan(self, avg_len: int, lines: int, tile_cap: int):
        look = C.c_uint32()
        s = self.lib.fgf_plan(C.c_uint64(avg_len), C.c_uint32(lines), C.c_uint32(tile_cap), C.byref(look))
        return int(s), int(look.value)

    def geometry(self, fmt: int, avg_line: int, lines_per_group: int = 0, tile_cap: int = 0, fused_look: int = 0, fused_ext: int = 0,
                 flags: int = 0, link_bound: bool = False) -> dict:
        """fg::fused_geometry: what a fused launch of `fmt` looks like under these launch options"""
        out = (C.c_uint32 * 8)()
        self.lib.fgf_geometry(C.c_int(fmt), C.c_uint64(avg_line), C.c_uint32(lines_per_group), C.c_uint32(tile_cap), C.c_uint32(fused_look),
                              C.c_uint32(fused_ext), C.c_uint32(flags), C.c_int(1 if link_bound else 0), out)
        return dict(S=int(out[0]), look=int(out[1]), tile=int(out[2]), ext=int(out[3]), L=int(out[4]), variant=int(out[5]), ok=bool(out[6]))

    def frame(self, raw: bytes, delim: int, final: bool, S: int, look: int, tile_cap: int, lines: int = 64, garbage: int = 0x0A):
        """-> (starts, ends, bad, consumed, passes, scans); what lies behind the stream's end inside its last 16 bytes is `garbage`"""
        n = len(raw)
        padded = (n + 15) & ~15
        buf = np.full(max(padded, 16), garbage, np.uint8)
        buf[:n] = np.frombuffer(raw, np.uint8)
        cap = n + 2
        starts, ends = np.zeros(cap, np.uint64), np.zeros(cap, np.uint64)
        bad = np.zeros(cap, np.uint8)
        consumed, passes, scans = C.c_uint64(), C.c_uint64(), C.c_uint64()
        r = self.lib.fgf_frame(C.c_void_p(buf.ctypes.data), C.c_uint64(n), C.c_uint32(delim), C.c_int(1 if final else 0), C.c_uint32(S),
                               C.c_uint32(look), C.c_uint32(tile_cap), C.c_uint32(lines), C.c_void_p(starts.ctypes.data),
                               C.c_void_p(ends.ctypes.data), C.c_void_p(bad.ctypes.data), C.c_uint64(cap), C.byref(consumed), C.byref(passes),
                               C.byref(scans))
        if r < 0:
            raise RuntimeError(self.lib.fgf_last_error().decode())
        return starts[:r], ends[:r], bad[:r], int(consumed.value), int(passes.value), int(scans.value)

    def chunk_masks(self, chunk: bytes, pw: bytes, delim: int, rem: int) -> int:
        """fuse::chunk_masks of one 16-byte chunk behind the dword pw: delimiter mask | UTF-8 error mask << 16"""
        q = (C.c_uint32 * 4)(*np.frombuffer(chunk, "<u4"))
        self.lib.fgf_chunk_masks.restype = C.c_uint32
        return int(self.lib.fgf_chunk_masks(q, C.c_uint32(int.from_bytes(pw, "little")), C.c_uint32(delim), C.c_int32(rem)))

    def scalar_bad4(self, alphabet: bytes) -> np.ndarray:
        """the scalar rule's verdict (fg::utf8::payload_bad) on every four-byte string over the alphabet, in itertools.product order"""
        out = np.zeros(len(alphabet) ** 4, np.uint8)
        self.lib.fgf_scalar_bad4(C.c_char_p(alphabet), C.c_uint32(len(alphabet)), C.c_void_p(out.ctypes.data))
        return out

    def rule_sweep(self, alphabet: bytes, rems, delim: int):
        """fgf_rule_sweep -> (triples that differ, the first one (string index, phase, rem, got, want), (triples, error bits, delimiter bits))"""
        r = (C.c_int32 * len(rems))(*rems)
        first, stats = (C.c_int64 * 5)(), (C.c_uint64 * 3)()
        self.lib.fgf_rule_sweep.restype = C.c_uint64
        wrong = self.lib.fgf_rule_sweep(C.c_char_p(alphabet), C.c_uint32(len(alphabet)), r, C.c_uint32(len(rems)), C.c_uint32(delim), first, stats)
        return int(wrong), tuple(int(x) for x in first), tuple(int(x) for x in stats)
