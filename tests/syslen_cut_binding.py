"""ctypes binding of tests/native/libsyslen_cut_host.so: the per-segment cut's device logic (flowgger_amd/csrc/fg_syslen_multi.hpp,
cut_find / cut_mark) compiled for the CPU over the fiber emulation of a wavefront (test infrastructure)."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent / "native"
ROOT = HERE.parent.parent
CSRC = ROOT / "flowgger_amd" / "csrc"
LIB = HERE / "libsyslen_cut_host.so"
SRC = [HERE / "syslen_cut_host.cpp", HERE / "fg_wave_emu.hpp", CSRC / "fg_syslen_multi.hpp", CSRC / "fg_syslen.hpp", CSRC / "fg_wave.hpp",
       CSRC / "fg_syslen_parse.hpp", CSRC / "fg_frame_multi.hpp", CSRC / "fg_utf8.hpp"]
GUARD = 0xEE
WORD_GUARD = 0xEEEEEEEE


def build() -> Path:
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRC):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        f"-I{ROOT / 'include'}", f"-I{HERE}", f"-I{CSRC}", "-o", str(LIB), str(HERE / "syslen_cut_host.cpp")], check=True)
    return LIB


class SyslenCutHost:
    def __init__(self):
        self.lib = C.CDLL(str(build()))
        self.lib.fgsc_last_error.restype = C.c_char_p
        self.lib.fgsc_mark.restype = C.c_uint32
        self.mark = self.lib.fgsc_mark()

    def cut(self, bad, seg_first, reverse: bool = False):
        """-> the n verdicts after both passes.  The arrays have guard entries behind what the passes may touch; they are checked here."""
        n, k = len(bad), len(seg_first) - 1
        b = np.full(n + 8, GUARD, np.uint8)
        b[:n] = bad
        first = np.asarray(seg_first, np.uint64)
        words = np.full(k + 1 + 2, WORD_GUARD, np.uint32)
        vp = lambda a: C.c_void_p(a.ctypes.data)
        rc = self.lib.fgsc_cut(vp(b), C.c_uint64(n), vp(first), C.c_uint64(k), vp(words), C.c_int(int(reverse)))
        if rc != 0:
            raise RuntimeError(self.lib.fgsc_last_error().decode())
        assert (b[n:] == GUARD).all() and (words[k + 1:] == WORD_GUARD).all()
        return b[:n].copy()
