"""What the output compressor (flowgger_amd/csrc/fg_deflate.hpp) is held against: the member policies as a Python model, the case
list, and the checks.  The oracle everywhere is Python's zlib: every member inflates on its own, as a gzip member, to exactly its
input, with nothing left over (which settles CRC-32 and ISIZE too)."""
from __future__ import annotations

import ctypes as C
import subprocess
import zlib
from pathlib import Path

import numpy as np

from flowgger_amd import synth

HERE = Path(__file__).resolve().parent / "native"
ROOT = HERE.parent.parent
CSRC = ROOT / "flowgger_amd" / "csrc"
LIB = HERE / "libdeflate_host.so"
SRC = [HERE / "deflate_host.cpp", HERE / "deflate_driver.hpp", HERE / "fg_wave_emu.hpp", CSRC / "fg_deflate.hpp", CSRC / "fg_inflate.hpp",
       CSRC / "fg_wave.hpp"]
HEADER = bytes([0x1F, 0x8B, 8, 0, 0, 0, 0, 0, 0, 0xFF])
LENGTHS_SMALL = [0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 257, 258, 259, 260, 261]
PHRASE = b"the quick brown fox jumps over the lazy dog, 0123456789 times"


def build() -> Path:
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRC):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", f"-I{CSRC}", f"-I{HERE}", "-o", str(LIB),
                        str(HERE / "deflate_host.cpp")], check=True)
    return LIB


def pack_members(members):
    """-> (bytes as uint8 with 16 bytes of padding behind them, cuts[n + 1])"""
    cuts = np.zeros(len(members) + 1, np.uint64)
    cuts[1:] = np.cumsum([len(m) for m in members], dtype=np.uint64) if members else 0
    blob = np.zeros(int(cuts[-1]) + 16, np.uint8)
    blob[:int(cuts[-1])] = np.frombuffer(b"".join(members), np.uint8)
    return blob, cuts


class DeflateHost:
    """the core on the wave emulation (tests/native/deflate_host.cpp)"""

    def __init__(self):
        self.lib = C.CDLL(str(build()))
        self.lib.fgd_block_bytes.restype = C.c_uint32
        self.lib.fgd_bound.restype = C.c_uint64
        self.lib.fgd_deflate.restype = C.c_uint64
        self.lib.fgd_members.restype = C.c_uint64
        self.block = int(self.lib.fgd_block_bytes())

    def bound(self, nbytes, n_members):
        return int(self.lib.fgd_bound(C.c_uint64(nbytes), C.c_uint64(n_members)))

    def deflate_raw(self, blob, nbytes, cuts):
        """-> (z as uint8 of exactly the total, z_offsets[n + 1]); None for refused cuts"""
        vp = lambda a: C.c_void_p(a.ctypes.data)
        n = len(cuts) - 1
        zoffs = np.zeros(n + 1, np.uint64)
        args = [vp(blob), C.c_uint64(nbytes), vp(cuts), C.c_uint64(n)]
        total = int(self.lib.fgd_deflate(*args, None, C.c_uint64(0), vp(zoffs)))
        if total == 2**64 - 1:
            return None
        z = np.zeros(max(total, 1), np.uint8)
        zoffs2 = np.zeros(n + 1, np.uint64)
        assert int(self.lib.fgd_deflate(*args, vp(z), C.c_uint64(total), vp(zoffs2))) == total and np.array_equal(zoffs, zoffs2)
        return z[:total], zoffs

    def deflate(self, members):
        blob, cuts = pack_members(members)
        return self.deflate_raw(blob, int(cuts[-1]), cuts)

    def members(self, off, coalesce, member_bytes):
        off = np.ascontiguousarray(off, np.uint64)
        n = len(off) - 1
        first, cuts = np.zeros(n + 2, np.uint64), np.zeros(n + 2, np.uint64)
        nm = int(self.lib.fgd_members(C.c_void_p(off.ctypes.data), C.c_uint64(n), C.c_uint64(coalesce), C.c_uint64(member_bytes),
                                      C.c_void_p(first.ctypes.data), C.c_void_p(cuts.ctypes.data)))
        return first[:nm + 1], cuts[:nm + 1]


# ---- the member policies (fg_hip.h: fg_compress_cfg)
def model_members(off, coalesce, member_bytes, block):
    """-> (member_first[n_members + 1], cuts[n_members + 1]) for out_offsets `off`"""
    off = [int(x) for x in off]
    n = len(off) - 1
    if coalesce >= 1:
        first = list(range(0, n, coalesce))
    else:
        b = member_bytes or block
        first = [i for i in range(n) if i == 0 or off[i] // b > off[i - 1] // b]
    first.append(n)
    return np.array(first, np.uint64), np.array([off[i] for i in first], np.uint64)


# ---- the checks
def split(z, zoffs):
    z = bytes(z)
    return [z[int(zoffs[k]):int(zoffs[k + 1])] for k in range(len(zoffs) - 1)]


def check_members(members, z, zoffs, block, what=""):
    """every member alone against zlib, the frame, the per-member size bound; returns the deflate bytes (frames excluded)"""
    assert len(zoffs) == len(members) + 1 and int(zoffs[0]) == 0 and int(zoffs[-1]) == len(z), what
    body = 0
    for k, (raw, zm) in enumerate(zip(members, split(z, zoffs))):
        tag = f"{what} member {k} ({len(raw)} bytes)"
        if not raw:
            assert zm == b"", tag
            continue
        assert zm[:10] == HEADER, tag
        d = zlib.decompressobj(31)
        got = d.decompress(zm)
        assert got == raw and d.eof and d.unused_data == b"", tag
        assert len(zm) <= len(raw) + 18 + 12 * (-(-len(raw) // block)), tag
        body += len(zm) - 18
    return body


# ---- the cases
def contents(n: int, block: int):
    """(name, n bytes) for every content of the length-by-content list"""
    rng = np.random.default_rng(1000 + n)
    rep = lambda unit: (unit * (n // len(unit) + 1))[:n]
    out = [("one_byte", b"a" * n), ("one_byte_hi", b"\xe9" * n)]
    out += [(f"period{k}", rep(bytes(range(65, 65 + k)) if k < 200 else bytes((7 * i + 3) % 251 for i in range(k)))) for k in (2, 3, 4, 257)]
    out.append(("all_bytes", rep(bytes(range(256)))))
    out.append(("random", rng.integers(0, 256, n, dtype=np.uint8).tobytes()))
    out.append(("gelf", rep(b"\n".join(_gelf()[:200]))))
    # (the filler is one long run: it goes out as distance-1 matches, publishes a single hash slot and so leaves the phrase's slots
    #  of the window at 0 alone -- the planted match is found and reaches the output)
    filler = b"~" * n
    far = bytearray(filler)  # the phrase at 0 and again at the end of the first block: the longest distance a block allows
    if n >= 2 * len(PHRASE):
        far[:len(PHRASE)] = PHRASE
        at = min(n, block) - len(PHRASE)
        far[at:at + len(PHRASE)] = PHRASE
    out.append(("phrase_far", bytes(far)))
    cross = bytearray(filler)  # the phrase early, and again across the block boundary at every offset -2 .. +2
    if n > block + len(PHRASE):
        cross[:len(PHRASE)] = PHRASE
        at = block - len(PHRASE) // 2 + (n % 5) - 2
        cross[at:at + len(PHRASE)] = PHRASE
    out.append(("phrase_cross", bytes(cross)))
    return out


_GELF = None


def _gelf():
    global _GELF
    if _GELF is None:
        _GELF = synth.gelf_lines(4000)
    return _GELF


def lengths(block: int):
    return LENGTHS_SMALL + [block - 1, block, block + 1, 2 * block - 1, 2 * block, 2 * block + 1]


def case_members(block: int):
    """the length-by-content list as one batch of members: (names, members)"""
    names, members = [], []
    for n in lengths(block):
        for name, data in contents(n, block):
            assert len(data) == n
            names.append(f"{name}/{n}")
            members.append(data)
    return names, members


def cross_cases(block: int):
    """members of B + 200 bytes, a run but for the phrase at 0 and a second copy that starts at each offset from one phrase short of
    B - 2 up to B + 2: every way the copy can lie across (or just touch) the block boundary"""
    out = []
    for at in range(block - 2 - len(PHRASE) + 1, block + 3):  # every overlap of the boundary, and the copies that just touch it
        buf = bytearray(b"~" * (block + 200))
        buf[:len(PHRASE)] = PHRASE
        buf[at:at + len(PHRASE)] = PHRASE
        out.append(bytes(buf))
    return out


def equal_members(count: int = 40):
    text = b"\n".join(_gelf()[:12])
    return [text] * count


def fuzz_members(count: int, block: int, seed: int = 5):
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        n = int(rng.integers(0, 3 * block + 1)) if k % 4 == 0 else int(rng.integers(0, 600))
        if k == 0:
            n = 3 * block
        buf = bytearray()
        while len(buf) < n:
            kind, span = int(rng.integers(0, 3)), int(rng.integers(1, 400))
            if kind == 0 or not buf:
                buf += rng.integers(0, 256, span, dtype=np.uint8).tobytes()
            elif kind == 1:
                a = int(rng.integers(0, len(buf)))
                piece = bytes(buf[a:a + span])
                buf += piece * int(rng.integers(1, 4))
            else:
                buf += bytes([int(rng.integers(0, 256))]) * span
        out.append(bytes(buf[:n]))
    return out
