"""The one-walk form of the UDP input's inflate core (flowgger_amd/csrc/fg_inflate.hpp: stage_datagram, stage_capacity) compiled for
the CPU and run in the device's order -- stage every datagram, scan, write_datagram for the spilled rows, copy the others -- against the
model of tests/udp_model.py.  Exact on offsets, bytes, drop and status, at every stage capacity where a piece of the stream straddles
the stage's end; and the number of spilled datagrams under the policy is what the model's sizes say it is."""
import ctypes as C
import functools
import struct
import subprocess
import zlib

import numpy as np
import pytest

import udp_model as um

LIB = um.HERE / "libinflate_once_host.so"
SRC = [um.HERE / "inflate_once_host.cpp", um.ROOT / "flowgger_amd" / "csrc" / "fg_inflate.hpp", um.ROOT / "flowgger_amd" / "csrc" / "fg_utf8.hpp"]
STAGE_K, STAGE_C = 4, 64  # the issue's policy: w = min(max_inflated + 1, round_up_16(K * len + C)) for a gated datagram, 0 for a bare one


def policy_w(d: bytes, max_inflated: int) -> int:
    if um.gate(d) == um.RAW:
        return 0
    return min(max_inflated + 1, (STAGE_K * len(d) + STAGE_C + 15) // 16 * 16)


class OnceHost:
    def __init__(self):
        if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRC):
            subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fPIC", "-shared", "-Wall", f"-I{um.ROOT / 'flowgger_amd' / 'csrc'}", "-o", str(LIB),
                            str(SRC[0])], check=True)
        self.lib = C.CDLL(str(LIB))
        self.lib.fgo_unpack_batch.restype = C.c_uint64
        self.lib.fgo_stage_capacity.restype = C.c_uint32

    def unpack(self, datagrams, max_inflated, w=None):
        """-> (offsets[n + 1], packed, drop[n], status[n], spilled datagrams); w: the stage capacity per datagram (None: the policy)"""
        blob, offs = um.pack(datagrams)
        n = len(datagrams)
        data = np.zeros(blob.size + 16, np.uint8)
        data[:blob.size] = blob
        out_offs = np.zeros(n + 1, np.uint64)
        drop, status = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
        spilled = C.c_uint64(0)
        vp = lambda a: C.c_void_p(a.ctypes.data)
        wa = None if w is None else np.asarray(w, np.uint32)
        args = [vp(data), vp(offs), C.c_uint64(n), C.c_uint32(max_inflated), None if wa is None else vp(wa)]
        tail = [vp(out_offs), vp(drop), vp(status), C.byref(spilled)]
        total = self.lib.fgo_unpack_batch(*args, None, C.c_uint64(0), *tail)
        assert total != 2 ** 64 - 1, "a row that did not spill lies beyond its stage"
        packed = np.zeros(total + 16, np.uint8)
        assert self.lib.fgo_unpack_batch(*args, vp(packed), C.c_uint64(total), *tail) == total
        return out_offs, packed, drop[:n], status[:n], int(spilled.value)


@pytest.fixture(scope="module")
def host():
    return OnceHost()


CORPUS_NAMES = ["case list"] + [f"hand-built streams, cap {cap}" for cap in um.HAND_CAPS] + ["truncations", "mutation pool", "random code sets"]
CORPUS_IDS = [c.replace(" ", "_").replace(",", "") for c in CORPUS_NAMES]
FORCED = ("0", "1", "2", "257", "258", "259", "size-1", "size", "size+1", "max+1")


@functools.lru_cache(maxsize=None)
def corpus(name):
    """-> (datagrams, max_inflated, the model's slot size of every datagram): the issue's list, each built once"""
    if name == "case list":
        grams, cap = [d for _, d in um.case_list()], um.DEFAULT_MAX
    elif name.startswith("hand-built"):
        cap = int(name.rsplit(" ", 1)[1])
        grams = [d for _, d, _ in um.hand_streams(cap)]
    elif name == "truncations":
        grams, cap = um.truncations(), um.DEFAULT_MAX
    elif name == "mutation pool":
        grams, cap = um.mutation_pool(5000), um.DEFAULT_MAX
    else:
        good, flipped = um.random_code_set_pool()
        grams, cap = good[:400] + flipped[:400], um.DEFAULT_MAX
    return grams, cap, [len(s) for s in um.expect(grams, cap)[2]]


@pytest.mark.parametrize("forced", FORCED)
@pytest.mark.parametrize("name", CORPUS_NAMES, ids=CORPUS_IDS)
def test_forced_stage_capacity(host, name, forced):
    """every stage the same relation to its datagram's size: a length-258 match or a distance-1 run straddles its end somewhere"""
    grams, cap, sizes = corpus(name)
    w = [{"size-1": max(s - 1, 0), "size": s, "size+1": s + 1, "max+1": cap + 1}.get(forced, None) for s in sizes]
    w = [int(forced) if x is None else x for x in w]
    offs, packed, drop, status, spilled = host.unpack(grams, cap, w)
    um.check_batch(grams, cap, offs, packed, drop, status, f"{name}, w = {forced}")
    # what spills is decided by the sizes alone: a gated datagram whose slot is larger than its stage
    assert spilled == sum(1 for d, s, wi in zip(grams, sizes, w) if um.gate(d) != um.RAW and s > wi), f"{name}, w = {forced}"


@pytest.mark.parametrize("name", CORPUS_NAMES, ids=CORPUS_IDS)
def test_policy_spill_count(host, name):
    grams, cap, sizes = corpus(name)
    for d in grams[:200]:
        assert host.lib.fgo_stage_capacity(d + bytes(16), C.c_uint64(len(d)), C.c_uint32(cap)) == policy_w(d, cap)
    fit = sum(1 for d, s in zip(grams, sizes) if s <= policy_w(d, cap) or um.gate(d) == um.RAW)
    offs, packed, drop, status, spilled = host.unpack(grams, cap)
    um.check_batch(grams, cap, offs, packed, drop, status, f"{name}, policy")
    assert (len(grams) - spilled, spilled) == (fit, len(grams) - fit), name


def test_policy_corner_cases(host):
    """the rows the issue names: a stream whose checksum alone disagrees keeps its bytes staged or spilled, and the complete row of
    exactly max_inflated + 1 bytes fits a stage of that size"""
    cap = 300
    bad_fit = bytearray(zlib.compress(um.JSON_LINE))
    bad_fit[-1] ^= 1
    bad_spill = bytearray(zlib.compress(b"z" * 20_000))
    bad_spill[-1] ^= 1
    exact = zlib.compress(b"q" * (cap + 1), 0)  # (stored: as long as what it holds, so the policy gives it the whole cap)
    grams = [bytes(bad_fit), bytes(bad_spill), exact]
    for c in (um.DEFAULT_MAX, cap):
        offs, packed, drop, status, spilled = host.unpack(grams, c)
        um.check_batch(grams, c, offs, packed, drop, status, f"corner cases, cap {c}")
        sizes = [len(s) for s in um.expect(grams, c)[2]]
        assert spilled == sum(1 for d, s in zip(grams, sizes) if s > policy_w(d, c))
    assert um.model(bytes(bad_fit))[0] == um.BAD_ZLIB and len(um.model(bytes(bad_fit))[1]) == len(um.JSON_LINE) <= policy_w(bytes(bad_fit), um.DEFAULT_MAX)
    assert um.model(bytes(bad_spill))[0] == um.BAD_ZLIB and len(um.model(bytes(bad_spill))[1]) == 20_000 > policy_w(bytes(bad_spill), um.DEFAULT_MAX)
    assert um.model(exact, cap) == (um.TOO_LARGE, b"q" * (cap + 1), False) and policy_w(exact, cap) == cap + 1


def test_sanitized_standalone_run_once(tmp_path):
    """the staged walk in a stand-alone program under AddressSanitizer and UBSan, over the hand-built streams at every cap and the
    flipped code sets, under the policy and with every stage forced to 0, 1, 258 and 259 bytes: each stage is an allocation of exactly
    its capacity.  The program checks its own sanity and that the capacity never changes the total; the answers are the other tests'."""
    root = um.ROOT
    exe = tmp_path / "inflate_once_sanitized"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                    f"-I{root / 'flowgger_amd' / 'csrc'}", str(root / "tests/native/inflate_once_host.cpp"),
                    str(root / "tests/native/inflate_once_sanitized_main.cpp"), "-o", str(exe)], check=True)
    good, flipped = um.random_code_set_pool()
    for k, cap in enumerate(um.HAND_CAPS):
        grams = [d for _, d, _ in um.hand_streams(cap)] + (flipped if k == 0 else flipped[:300])
        f = tmp_path / f"grams_{cap}.bin"
        f.write_bytes(b"".join(struct.pack("<I", len(g)) + g for g in grams))
        r = subprocess.run([str(exe), str(f), str(cap), "0", "1", "258", "259"], capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "" and r.stdout.split()[:2] == ["OK", str(len(grams))], r.stdout + r.stderr
        sizes = [len(s) for s in um.expect(grams, cap)[2]]
        assert int(r.stdout.split()[2]) == sum(sizes)
        assert int(r.stdout.split()[3]) == sum(1 for d, s in zip(grams, sizes) if s > policy_w(d, cap))
