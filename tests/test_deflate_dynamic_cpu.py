"""FG_DEFLATE_DYNAMIC on the CPU: fg_deflate.hpp's second mode (compress_block_dyn and the wave's code builder) on the wave emulation
(tests/native/deflate_dyn_host.cpp) -- the builder alone against a plain Huffman build, every block against Python's zlib and against
the fixed mode of the same input, the shapes whose alphabets are degenerate, and the ratio against what zlib gains from the same step."""
import heapq
import math
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

import deflate_dyn_model as ddm
import deflate_model as dm

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def host():
    return ddm.DynHost()


@pytest.fixture(scope="module")
def B(host):
    return host.block


# ---- the code builder alone
def huffman(freq):
    """a plain Huffman build: (cost, depth)"""
    heap = [(f, 0, i) for i, f in enumerate(freq) if f]
    heapq.heapify(heap)
    cost, n = 0, len(freq)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1, n))
        n += 1
    return cost, heap[0][1]


def fib(n):
    out = [1, 1]
    while len(out) < n:
        out.append(out[-1] + out[-2])
    return out[:n]


def histograms():
    """(name, freq, limit)"""
    out = [("one", [0, 0, 9, 0], 15), ("one_of_286", [0] * 285 + [3], 15), ("two", [4, 0, 0, 1], 15), ("two_equal", [0, 7, 7], 7),
           ("three", [1, 0, 2, 0, 50], 15), ("three_equal", [5, 5, 5], 7), ("all_286_equal", [57] * 286, 15), ("none", [0] * 30, 15)]
    for n in range(17, 25):  # deeper than 15 unlimited: sum(fib(24)) = 75 024 counts are more than a block has, the builder takes them
        out.append((f"fib{n}", fib(n), 15))
        out.append((f"fib{n}_scattered", [f for x in fib(n)[::-1] for f in (x, 0, 0)], 15))
    for n in range(10, 20):
        out.append((f"fib{n}_limit7", fib(n) + [0] * (19 - n), 7))
    rng = np.random.default_rng(77)
    for k in range(200):
        n = (286, 30, 19)[k % 3]
        used = int(rng.integers(1, n + 1))
        f = np.zeros(n, np.int64)
        idx = rng.permutation(n)[:used]
        w = rng.random(used) ** int(rng.integers(1, 9))  # (from flat to very skewed)
        f[idx] = np.maximum(1, (w / w.sum() * int(rng.integers(used, 16385 - used))).astype(np.int64)) if used < 16000 else 1
        assert f.sum() <= 16384
        out.append((f"random{k}", f.tolist(), 15 if n != 19 else 7))
    return out


def test_code_builder(host):
    limited_seen = 0
    for name, freq, limit in histograms():
        lens, cost, limited = host.lengths(freq, limit)
        used = sum(1 for f in freq if f)
        assert all((l == 0) == (f == 0) for l, f in zip(lens, freq)), name
        assert max(lens, default=0) <= limit, name
        assert cost == sum(f * l for f, l in zip(freq, lens)), name
        kraft = sum(2 ** (limit - l) for l in lens if l)
        if used >= 2:
            assert kraft == 2 ** limit, name
            hcost, hdepth = huffman(freq)
            assert cost >= hcost, name
            if hdepth <= limit:
                assert cost == hcost and not limited, name
            else:
                assert limited, name
            assert cost <= math.ceil(math.log2(used)) * sum(freq), name
        elif used == 1:
            assert sorted(lens)[-1] == 1 and sum(lens) == 1 and not limited, name
        limited_seen += limited
    assert limited_seen >= 20  # (the Fibonacci histograms beyond the limits)
    assert huffman(fib(17))[1] == 16 and huffman(fib(10))[1] == 9


# ---- blocks
@pytest.fixture(scope="module")
def cases(host, B):
    names, members = ddm.all_cases(B, fuzz=400)
    return names, members, ddm.emulate(host, members, ddm.DYNAMIC), ddm.emulate(host, members, ddm.FIXED)


def glue(zs):
    return np.frombuffer(b"".join(zs), np.uint8), np.concatenate([[0], np.cumsum([len(z) for z in zs])]).astype(np.uint64)


def test_every_case_in_dynamic_mode(host, B, cases):
    names, members, dyn, fixed = cases
    assert len(members) == 23 * 11 + len(dm.PHRASE) + 4 + 40 + 400 + 5
    dm.check_members(members, *glue(dyn), B, "dynamic")
    assert sum(map(len, dyn)) <= host.lib.fgd_bound(sum(map(len, members)), len(members))
    # the fixed mode of the new driver is the old driver's
    old = dm.DeflateHost()
    z, zoffs = old.deflate(members[:23 * 11])
    assert dm.split(z, zoffs) == fixed[:23 * 11]
    for name, raw, zd, zf in zip(names, members, dyn, fixed):
        assert len(zd) <= len(zf), name
        if not raw:
            continue
        if len(raw) <= B and ddm.btype(zd) != 2:
            assert zd == zf, name
        if name.startswith("random/"):
            assert zd == zf and (len(raw) < 64 or zd[10] & 6 == 0), name
        if name.startswith("gelf/") and len(raw) >= B - 1:  # (text by the block: what the mode is for, see the ratio test)
            assert ddm.btype(zd) == 2 and len(zd) < 0.9 * len(zf), name
    # a second run, in other batches: the same bytes
    again = ddm.emulate(host, members[:120], ddm.DYNAMIC, workers=7)
    assert again == dyn[:120]


def test_named_shapes(host, B):
    seed, blk = ddm.limited_block(host)
    assert seed == ddm.LIMITED_SEED  # (the search's result is committed: named_shapes() builds the block from it)
    shapes = ddm.named_shapes(B)
    assert [n for n, _ in shapes] == ["one_byte", "de_bruijn", "de_bruijn_blocks", "limited", "gelf_message"] and dict(shapes)["limited"] == blk
    members = [m for _, m in shapes]
    z, zoffs, info = host.deflate(members)
    dm.check_members(members, z, zoffs, B, "named shapes")
    zf, zfoffs, _ = host.deflate(members, ddm.FIXED)
    nblk = [-(-len(m) // B) for m in members]
    first = np.concatenate([[0], np.cumsum(nblk)])
    for k, ((name, raw), zm, fm) in enumerate(zip(shapes, dm.split(z, zoffs), dm.split(zf, zfoffs))):
        assert ddm.btype(zm) == 2 and int(info[first[k]]) >> 4 == 2 and len(zm) < len(fm), name
    by = {n: (zm, info[first[k]:first[k + 1]]) for k, ((n, _), zm) in enumerate(zip(shapes, dm.split(z, zoffs)))}
    # one literal, end-of-block and length 258 (and the remainder's length): a few bits a token.  63 matches of 258 and a tail
    assert len(by["one_byte"][0]) < 18 + 40
    # 256 literals over four values and end-of-block: two bits a literal and a header
    assert len(by["de_bruijn"][0]) < 18 + 64 + 30
    assert [int(i) >> 4 for i in by["de_bruijn_blocks"][1]] == [2, 2, 1]  # (the last block is one byte)
    assert int(by["limited"][1][0]) & ddm.LIM_LIT
    assert 24 <= len(by["gelf_message"][0]) < len(dict(shapes)["gelf_message"])


# ---- the ratio
def zlib_sizes(pieces):
    f = d = 0
    for p in pieces:
        c = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
        f += len(c.compress(p) + c.flush())
        c = zlib.compressobj(1, zlib.DEFLATED, -15, 8)
        d += len(c.compress(p) + c.flush())
    return f, d


def test_ratio_against_zlib_dynamic(host, B):
    """ours_dyn <= ours_fixed * (1 + D / F) / 2 -- half of what zlib level 1 gains by the same step, over the same pieces -- for the members
    of member_bytes = 65536 (F, D over every 16 KiB block of every member alone) and for one message per member"""
    msgs = [x + b"\n" for x in dm._gelf()]
    off = np.concatenate([[0], np.cumsum([len(m) for m in msgs])]).astype(np.uint64)
    _, cuts = dm.model_members(off, 0, 65536, B)
    raw = b"".join(msgs)
    big = [raw[int(cuts[k]):int(cuts[k + 1])] for k in range(len(cuts) - 1)]
    assert len(big) >= 15 and max(map(len, big)) <= 65536 + 400
    for what, members, pieces in (("member_bytes 65536", big, [m[a:a + B] for m in big for a in range(0, len(m), B)]), ("one message", msgs, msgs)):
        dyn, fixed = ddm.emulate(host, members, ddm.DYNAMIC), ddm.emulate(host, members, ddm.FIXED)
        ours_dyn = dm.check_members(members, *glue(dyn), B, what)
        ours_fixed = dm.check_members(members, *glue(fixed), B, what)
        F, D = zlib_sizes(pieces)
        R = sum(map(len, members))
        print(f"{what}: raw {R}; ours fixed {ours_fixed / R:.4f} dynamic {ours_dyn / R:.4f} (dynamic / fixed {ours_dyn / ours_fixed:.4f}); "
              f"zlib F {F / R:.4f} D {D / R:.4f} (D / F {D / F:.4f})")
        assert 0.75 < D / F < 0.87, what  # (the corpus is the one the cap was derived for: 0.809 and 0.8125)
        assert ours_dyn <= ours_fixed * (1 + D / F) / 2, what


def test_sanitized_standalone_run(tmp_path):
    """compress_block_dyn and build_lengths in a stand-alone program under AddressSanitizer and UBSan (tests/native/deflate_dyn_san_main.cpp):
    inputs, slots and outputs that end with their last byte.  Nothing loaded into Python is sanitized."""
    exe = tmp_path / "deflate_dyn_san"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fno-omit-frame-pointer", f"-I{ROOT / 'flowgger_amd' / 'csrc'}",
           f"-I{ROOT / 'tests' / 'native'}", str(ROOT / "tests/native/deflate_dyn_san_main.cpp"), "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd[:1] + san + cmd[1:], capture_output=True).returncode != 0:
        subprocess.run(cmd, check=True)  # (no sanitizer runtime on this machine: the plain build still runs every case)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.split()[:1] == ["ok"] and "ERROR" not in r.stderr, r.stdout + r.stderr
