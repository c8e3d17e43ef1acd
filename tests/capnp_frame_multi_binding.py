"""ctypes binding of tests/native/libcapnp_frame_multi_host.so: the segmented Cap'n Proto framer's device logic
(flowgger_amd/csrc/fg_capnp_frame_multi.hpp) compiled for the CPU over the fiber emulation of a wavefront (test infrastructure)."""
from __future__ import annotations

import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent / "native"
ROOT = HERE.parent.parent
CSRC = ROOT / "flowgger_amd" / "csrc"
LIB = HERE / "libcapnp_frame_multi_host.so"
SRC = [HERE / "capnp_frame_multi_host.cpp", HERE / "fg_wave_emu.hpp", CSRC / "fg_capnp_frame_multi.hpp", CSRC / "fg_capnp_frame.hpp",
       CSRC / "fg_capnp_next.hpp", CSRC / "fg_wave.hpp", CSRC / "fg_frame_multi.hpp", CSRC / "fg_utf8.hpp"]
GUARD = 0xEE
U64_GUARD = 0xEEEEEEEEEEEEEEEE


def build() -> Path:
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRC):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        f"-I{ROOT / 'include'}", f"-I{HERE}", f"-I{CSRC}", "-o", str(LIB), str(HERE / "capnp_frame_multi_host.cpp")], check=True)
    return LIB


class CapnpFrameMultiHost:
    def __init__(self):
        self.lib = C.CDLL(str(build()))
        self.lib.fgcm_last_error.restype = C.c_char_p
        self.lib.fgcm_tile_words.restype = C.c_uint32
        self.lib.fgcm_node_cap.restype = C.c_uint32
        self.tile_words = self.lib.fgcm_tile_words()

    def node_cap(self, nbytes: int, n_segs: int) -> int:
        return int(self.lib.fgcm_node_cap(C.c_uint64(nbytes), C.c_uint64(n_segs)))

    def frame(self, buf: bytes, seg_starts, cap: int | None = None):
        """-> dict(declined, n, offsets, kind, seg_first, seg_consumed, seg_stop, overflow): the stages, tile by tile.  Every output array
        has guard entries behind what the call may write; they are checked here."""
        n = len(buf)
        k = len(seg_starts) - 1
        data = np.zeros((n + 15) // 16 * 16 + 16, np.uint8)
        data[:n] = np.frombuffer(buf, np.uint8)
        cap = n // 8 + k if cap is None else cap
        raw = np.asarray(seg_starts, np.uint64)
        offsets = np.full(cap + 1 + 4, U64_GUARD, np.uint64)
        kind = np.full(cap + 4, GUARD, np.uint8)
        seg_first = np.full(k + 1 + 4, U64_GUARD, np.uint64)
        seg_consumed = np.full(k + 4, U64_GUARD, np.uint64)
        seg_stop = np.full(k + 4, GUARD, np.uint8)
        hdr = np.zeros(16, np.uint32)
        vp = lambda a: C.c_void_p(a.ctypes.data)
        rc = self.lib.fgcm_frame(vp(data), C.c_uint64(n), vp(raw), C.c_uint64(k), vp(offsets), vp(kind), C.c_uint64(cap), vp(seg_first),
                                 vp(seg_consumed), vp(seg_stop), vp(hdr))
        if rc != 0:
            raise RuntimeError(self.lib.fgcm_last_error().decode())
        assert (offsets[cap + 1:] == U64_GUARD).all() and (kind[cap:] == GUARD).all()
        assert (seg_first[k + 1:] == U64_GUARD).all() and (seg_consumed[k:] == U64_GUARD).all() and (seg_stop[k:] == GUARD).all()
        untouched = ((offsets == U64_GUARD).all() and (kind == GUARD).all() and (seg_first == U64_GUARD).all()
                     and (seg_consumed == U64_GUARD).all() and (seg_stop == GUARD).all())
        if hdr[0]:
            assert untouched, "a declined launch wrote to an output"
            return {"declined": int(hdr[0]), "nodes": int(hdr[5])}
        assert hdr[4] == 1, "the scan did not run"
        ns = int(hdr[2])
        if ns > cap:  # the need is reported, no output is written
            assert untouched, "an overflowing launch wrote to an output"
            return {"declined": 0, "n": ns, "overflow": True}
        assert (offsets[ns + 1:] == U64_GUARD).all() and (kind[ns:] == GUARD).all()
        return {"declined": 0, "overflow": False, "n": ns, "offsets": offsets[:ns + 1], "kind": kind[:ns], "seg_first": seg_first[:k + 1],
                "seg_consumed": seg_consumed[:k], "seg_stop": seg_stop[:k], "nodes": int(hdr[5])}
