"""ctypes binding of tests/native/libframe_multi_host.so: flowgger_amd/csrc/fg_frame_multi.hpp (the boundary logic of the segmented
framer) compiled for the CPU (test infrastructure)."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from frame_multi_model import Slots

HERE = Path(__file__).resolve().parent / "native"
ROOT = HERE.parent.parent
LIB = HERE / "libframe_multi_host.so"
SRC = [HERE / "frame_multi_host.cpp", ROOT / "flowgger_amd" / "csrc" / "fg_frame_multi.hpp", ROOT / "flowgger_amd" / "csrc" / "fg_utf8.hpp"]


def build() -> Path:
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRC):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wextra", f"-I{ROOT / 'flowgger_amd' / 'csrc'}",
                        "-o", str(LIB), str(SRC[0])], check=True)
    return LIB


class FrameMultiHost:
    def __init__(self):
        self.lib = C.CDLL(str(build()))
        self.lib.fgm_frame.restype = C.c_long

    def frame(self, raw: bytes, seg_starts, seg_final, framing: int, block: int = 0, reverse: bool = False):
        """-> (Slots, clamped starts, delimiters the patches added)"""
        n, K = len(raw), len(seg_starts) - 1
        buf = np.zeros(n + 16, np.uint8)
        buf[:n] = np.frombuffer(raw, np.uint8)
        starts = np.array(seg_starts, np.uint64)
        final = None if seg_final is None else np.array(seg_final, np.uint8)
        cap = n + 1
        offsets, kind = np.zeros(cap + 1, np.uint64), np.zeros(cap, np.uint8)
        first, cons, c = np.zeros(K + 1, np.uint64), np.zeros(max(K, 1), np.uint64), np.zeros(K + 1, np.uint64)
        added = C.c_uint64()
        vp = C.c_void_p
        r = self.lib.fgm_frame(vp(buf.ctypes.data), C.c_uint64(n), C.c_uint32(0x0A if framing == 0 else 0), vp(starts.ctypes.data),
                               vp(final.ctypes.data) if final is not None and K else None, C.c_uint64(K), C.c_uint64(block),
                               C.c_int(1 if reverse else 0), vp(offsets.ctypes.data), vp(kind.ctypes.data), C.c_uint64(cap),
                               vp(first.ctypes.data), vp(cons.ctypes.data), vp(c.ctypes.data), C.byref(added))
        assert r >= 0
        return Slots(offsets[:r + 1], kind[:r], first, cons[:K]), [int(x) for x in c], int(added.value)
