"""ctypes binding of tests/native/libsyslen_multi_host.so: the segmented octet-counted framer's device logic
(flowgger_amd/csrc/fg_syslen_multi.hpp) compiled for the CPU over the fiber emulation of a wavefront (test infrastructure)."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent / "native"
ROOT = HERE.parent.parent
CSRC = ROOT / "flowgger_amd" / "csrc"
LIB = HERE / "libsyslen_multi_host.so"
SRC = [HERE / "syslen_multi_host.cpp", HERE / "fg_wave_emu.hpp", CSRC / "fg_syslen_multi.hpp", CSRC / "fg_syslen.hpp", CSRC / "fg_wave.hpp",
       CSRC / "fg_syslen_parse.hpp", CSRC / "fg_frame_multi.hpp", CSRC / "fg_utf8.hpp"]
GUARD = 0xEE
U64_GUARD = 0xEEEEEEEEEEEEEEEE


def build() -> Path:
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRC):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        f"-I{ROOT / 'include'}", f"-I{HERE}", f"-I{CSRC}", "-o", str(LIB), str(HERE / "syslen_multi_host.cpp")], check=True)
    return LIB


class SyslenMultiHost:
    def __init__(self):
        self.lib = C.CDLL(str(build()))
        self.lib.fgsm_last_error.restype = C.c_char_p
        for f in (self.lib.fgsm_tile, self.lib.fgsm_max_prefix, self.lib.fgsm_inbox):
            f.restype = C.c_uint32
        self.tile = self.lib.fgsm_tile()
        self.max_prefix = self.lib.fgsm_max_prefix()
        self.inbox = self.lib.fgsm_inbox()

    def frame(self, buf: bytes, seg_starts, cap: int | None = None):
        """-> dict(declined, n, total, packed, offsets, starts, bad, seg_first, seg_consumed, seg_stop, overflow): the stages, tile by
        tile.  Every output array has guard entries behind what the call may write; they are checked here."""
        n = len(buf)
        k = len(seg_starts) - 1
        data = np.zeros((n + 15) // 16 * 16 + 16, np.uint8)
        data[:n] = np.frombuffer(buf, np.uint8)
        cap = n // 2 + 1 if cap is None else cap
        raw = np.asarray(seg_starts, np.uint64)
        packed = np.full(n + 64, GUARD, np.uint8)
        offsets = np.full(cap + 1 + 4, U64_GUARD, np.uint64)
        starts = np.full(cap + 4, U64_GUARD, np.uint64)
        bad = np.zeros(cap + 4, np.uint8)
        bad[cap:] = GUARD
        seg_first = np.full(k + 1 + 4, U64_GUARD, np.uint64)
        seg_consumed = np.full(k + 4, U64_GUARD, np.uint64)
        seg_stop = np.full(k + 4, GUARD, np.uint8)
        hdr = np.zeros(16, np.uint32)
        vp = lambda a: C.c_void_p(a.ctypes.data)
        rc = self.lib.fgsm_frame(vp(data), C.c_uint64(n), vp(raw), C.c_uint64(k), vp(packed), vp(offsets), vp(starts), vp(bad), C.c_uint64(cap),
                                 vp(seg_first), vp(seg_consumed), vp(seg_stop), vp(hdr))
        if rc != 0:
            raise RuntimeError(self.lib.fgsm_last_error().decode())
        assert (offsets[cap + 1:] == U64_GUARD).all() and (starts[cap:] == U64_GUARD).all() and (bad[cap:] == GUARD).all()
        assert (seg_first[k + 1:] == U64_GUARD).all() and (seg_consumed[k:] == U64_GUARD).all() and (seg_stop[k:] == GUARD).all()
        if hdr[0]:
            return {"declined": int(hdr[0])}
        assert hdr[5] == 1, "the scan did not run"
        nf, total = int(hdr[2]), int(hdr[4])
        assert (packed[total:] == GUARD).all()
        if nf > cap:  # the need is reported, no output is written
            assert (seg_first == U64_GUARD).all() and (seg_consumed == U64_GUARD).all() and (seg_stop == GUARD).all()
            assert (offsets == U64_GUARD).all() and (starts == U64_GUARD).all() and (packed == GUARD).all()
            return {"declined": 0, "n": nf, "overflow": True}
        assert (starts[nf:] == U64_GUARD).all()
        return {"declined": 0, "overflow": False, "n": nf, "total": total, "packed": packed, "offsets": offsets[:nf + 1], "starts": starts[:nf],
                "bad": bad[:nf], "seg_first": seg_first[:k + 1], "seg_consumed": seg_consumed[:k], "seg_stop": seg_stop[:k]}
