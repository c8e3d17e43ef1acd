"""FG_DEFLATE_DYNAMIC on the wave emulation (tests/native/deflate_dyn_host.cpp): the compressor in either mode with the per-block report
of compress_block_dyn, the code builder alone, and the named shapes the CPU and the GPU tests share.  The cases and the checks are
tests/deflate_model.py's."""
from __future__ import annotations

import ctypes as C
import subprocess

import numpy as np

import deflate_model as dm

LIB = dm.HERE / "libdeflate_dyn_host.so"
SRC = [dm.HERE / "deflate_dyn_host.cpp", dm.HERE / "deflate_dyn_driver.hpp"] + dm.SRC[1:]
FIXED, DYNAMIC = 0, 1
LIM_LIT, LIM_DIST, LIM_CL = 1, 2, 4  # compress_block_dyn's *info; the block's BTYPE is info >> 4
LIMITED_SEED = 0  # limited_block(): the first seed of the search whose block had its literal/length code limited


def build():
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRC):
        subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", f"-I{dm.CSRC}", f"-I{dm.HERE}", "-o", str(LIB), str(SRC[0])],
                       check=True)
    return LIB


class DynHost:
    def __init__(self):
        self.lib = C.CDLL(str(build()))
        self.lib.fgd_block_bytes.restype = C.c_uint32
        self.lib.fgd_bound.restype = self.lib.fgd_deflate_mode.restype = C.c_uint64
        self.lib.fgd_build_lengths.restype = C.c_uint32
        self.block = int(self.lib.fgd_block_bytes())

    def deflate(self, members, mode=DYNAMIC):
        """-> (z, z_offsets[n + 1], info per block)"""
        vp = lambda a: C.c_void_p(a.ctypes.data)
        blob, cuts = dm.pack_members(members)
        n, nbytes = len(members), int(cuts[-1])
        nb = sum(-(-len(m) // self.block) for m in members)
        zoffs, info = np.zeros(n + 1, np.uint64), np.zeros(nb + 1, np.uint32)
        args = [vp(blob), C.c_uint64(nbytes), vp(cuts), C.c_uint64(n), C.c_int(mode)]
        total = int(self.lib.fgd_deflate_mode(*args, None, C.c_uint64(0), vp(zoffs), None))
        z = np.zeros(max(total, 1), np.uint8)
        assert int(self.lib.fgd_deflate_mode(*args, vp(z), C.c_uint64(total), vp(zoffs), vp(info))) == total
        return z[:total], zoffs, info[:nb]

    def lengths(self, freq, limit):
        """-> (lengths, cost, limited) of the wave's code builder"""
        f = np.ascontiguousarray(freq, np.uint32)
        out, lim = np.zeros(len(f), np.uint32), C.c_uint32(0)
        cost = int(self.lib.fgd_build_lengths(C.c_void_p(f.ctypes.data), C.c_uint32(len(f)), C.c_uint32(limit), C.c_void_p(out.ctypes.data), C.byref(lim)))
        return out.tolist(), cost, bool(lim.value)


def btype(zm: bytes) -> int:
    """of the first block of a gzip member"""
    return (zm[10] >> 1) & 3


def de_bruijn_256() -> bytes:
    """order 4 over four byte values: 256 bytes in which no four bytes occur twice (read as a line, not a cycle: the last three 4-grams
    of the cycle are not there at all)"""
    k, n = 4, 4
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    out = bytes(b"acgt"[x] for x in seq)
    assert len(out) == 256 and len({out[i:i + 4] for i in range(253)}) == 253
    return out


def fib_block(seed: int) -> bytes:
    """A block of 16 371 literals whose Huffman code is 17 levels deep.  The counts: 1, 2, then each the sum of the two before it plus one,
    fourteen values up to 986 (with the end-of-block symbol's 1 in front, every merge takes the chain so far and the next value: a chain
    as deep as it has values; the plain Fibonacci numbers tie at every level and the tree comes out half as deep), and fourteen more
    values with 986 each for four more levels.  The order: drawn by what is left of each count, seeded, but never completing four bytes
    that occurred before -- no 4-gram twice means the parse finds no match at all (a run of five holds one twice).  A draw that has no
    such choice left takes any byte; hence the search."""
    counts = [1, 2]
    while len(counts) < 14:
        counts.append(counts[-1] + counts[-2] + 1)
    left = np.array(counts + [counts[-1]] * 14, np.int64)
    rng = np.random.default_rng(seed)
    out, seen = [], set()
    for _ in range(int(left.sum())):
        order = rng.permutation(len(left))
        order = order[np.argsort(-(left[order] * rng.random(len(left))), kind="stable")]  # (more left: more likely in front)
        k = next((int(j) for j in order if left[j] and tuple(out[-3:] + [int(j)]) not in seen), None)
        if k is None:
            k = int(next(j for j in order if left[j]))
        if len(out) >= 3:
            seen.add(tuple(out[-3:] + [k]))
        out.append(k)
        left[k] -= 1
    return bytes(33 + 3 * k for k in out)


def limited_block(host: DynHost, seeds=range(LIMITED_SEED, LIMITED_SEED + 64)):
    """the seeded search: the first fib_block whose literal/length code the limiter shortened -> (seed, block)"""
    for seed in seeds:
        blk = fib_block(seed)
        if host.deflate([blk])[2][0] & LIM_LIT:
            return seed, blk
    return None, None


def gelf_message() -> bytes:
    return dm._gelf()[7] + b"\n"


def named_shapes(B: int):
    """(name, member) of the shapes that must come out dynamic; 'limited' is fib_block(LIMITED_SEED)"""
    db = de_bruijn_256()
    return [("one_byte", b"a" * B), ("de_bruijn", db), ("de_bruijn_blocks", (db * (2 * B // 256 + 1))[:2 * B + 1]), ("limited", fib_block(LIMITED_SEED)),
            ("gelf_message", gelf_message())]


def all_cases(B: int, fuzz: int = 64):
    """(names, members): deflate_model's case list, the copies across the block boundary, the equal members, a seeded fuzz and the named shapes"""
    names, members = dm.case_members(B)
    for tag, more in (("cross", dm.cross_cases(B)), ("equal", dm.equal_members()), ("fuzz", dm.fuzz_members(fuzz, B))):
        names = names + [f"{tag}/{k}" for k in range(len(more))]
        members = members + more
    shapes = named_shapes(B)
    return names + [f"shape/{n}" for n, _ in shapes], members + [m for _, m in shapes]


def emulate(host: DynHost, members, mode: int, workers: int = 16):
    """the members' gzip forms from the emulation, one list entry each (the batch is dealt to `workers` threads: members share nothing)"""
    from concurrent.futures import ThreadPoolExecutor

    chunks = [members[k::workers] for k in range(workers)]
    with ThreadPoolExecutor(max_workers=workers) as pool:
        parts = [dm.split(z, zo) for z, zo, _ in pool.map(lambda c: host.deflate(c, mode), chunks)]
    return [parts[i % workers][i // workers] for i in range(len(members))]
