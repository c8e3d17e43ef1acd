"""CPU: the compression of the transcode entry points (fg_set_output_compression, fg_last_compressed, fg_deflate_device: the host side in
flowgger_amd/csrc/fg_capi.cpp and fg_host_pipeline.cpp) on the fake runtime of test_host_pipeline_cpu.py, built with host loops over
fg_deflate.hpp in the place of the kernels of fg_deflate.hip (tests/native/host_pipeline_fake_deflate.cpp).  The compressor is the real
core, so the members are held against zlib and the cuts against the model of tests/deflate_model.py; the decode and the encoder behind
them are the fakes of host_pipeline_fake.cpp (an Ok row's message is its payload, one '#' per '=' and a newline)."""
import ctypes as C
import subprocess
import zlib

import numpy as np
import pytest

import deflate_model as dm
import test_host_pipeline_cpu as H
import udp_model as um
from flowgger_amd import _lib as L
from test_host_pipeline_cpu import Ctx

u64, vp = C.c_uint64, C.c_void_p
LIB = H.HERE / "libhost_pipeline_fake_deflate.so"
CSRC = H.ROOT / "flowgger_amd/csrc"
SRC = [H.HERE / "host_pipeline_fake_deflate.cpp", H.HERE / "host_pipeline_fake_udp.cpp", H.HERE / "deflate_driver.hpp", H.HERE / "fg_wave_emu.hpp",
       CSRC / "fg_deflate.hpp", CSRC / "fg_inflate.hpp", CSRC / "fg_wave.hpp", CSRC / "fg_utf8.hpp"] + H.SRC
LINE = L.FG_FRAME_LINE
POLICIES = [(1, 0), (7, 0), (4096, 0), (0, 0), (0, 4096)]


@pytest.fixture(scope="module")
def fake():
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRC):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-Wno-unused-variable", f"-I{H.HERE / 'fakehip'}", f"-I{H.ROOT / 'include'}", f"-I{CSRC}", f"-I{H.HERE}", "-o", str(LIB), str(SRC[0])],
                       check=True)
    lib = C.CDLL(str(LIB))
    lib.fg_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    lib.fg_destroy.argtypes = [vp]
    lib.fg_destroy.restype = None
    lib.fg_last_hip_error.argtypes = [vp]
    lib.fg_transcode_batch.argtypes = [vp, C.c_int, C.c_int, C.POINTER(L.fg_encode_cfg), vp, u64, vp, u64, C.c_int, C.POINTER(L.fg_transcoded)]
    lib.fg_transcode_multi_batch.argtypes = [vp, C.c_int, C.c_int, C.POINTER(L.fg_encode_cfg), vp, u64, vp, vp, u64, C.POINTER(L.fg_transcoded_multi)]
    lib.fg_udp_transcode_batch.argtypes = [vp, C.c_int, C.POINTER(L.fg_encode_cfg), vp, u64, vp, u64, u64, C.POINTER(L.fg_transcoded), C.POINTER(vp)]
    lib.fg_set_output_compression.argtypes = [vp, C.POINTER(L.fg_compress_cfg)]
    lib.fg_last_compressed.argtypes = [vp, C.POINTER(L.fg_compressed)]
    lib.fg_deflate_device.argtypes = [vp, vp, u64, vp, u64, vp, u64, vp, C.POINTER(u64), vp]
    lib.fg_deflate_block_bytes.restype = C.c_uint32
    lib.fgf_fail_call_after.argtypes = [C.c_longlong]
    lib.fgf_calls.restype = lib.fgf_in_flight.restype = C.c_ulonglong
    lib.fgf_deflate_caps.argtypes = [vp, C.POINTER(C.c_ulonglong)]
    return lib


def _arr(p, dt, cnt):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (cnt * np.dtype(dt).itemsize,)).view(dt).copy() if cnt and p else np.zeros(0, dt)


def _ecfg():
    ecfg = L.fg_encode_cfg()
    ecfg.encoder, ecfg.merger = L.FG_ENC_GELF, L.FG_MERGE_LINE
    return ecfg


def set_compression(lib, ctx, codec, coalesce=1, member_bytes=0):
    cfg = L.fg_compress_cfg(codec, coalesce, member_bytes)
    assert lib.fg_set_output_compression(ctx.h, C.byref(cfg)) == 0


def compressed(lib, ctx):
    c = L.fg_compressed()
    assert lib.fg_last_compressed(ctx.h, C.byref(c)) == 0
    nm = int(c.n_members)
    return {"z": _arr(c.z, np.uint8, int(c.z_bytes)), "z_offsets": _arr(c.z_offsets, np.uint64, nm + 1 if nm else 0),
            "member_first": _arr(c.member_first, np.uint64, nm + 1 if nm else 0), "n_members": nm, "raw_bytes": int(c.raw_bytes), "null": not c.z}


def lines_of(count, seed=5):
    ln = [x for x in H.corpus(count + 40, np.random.default_rng(seed)) if x and max(x) < 0x80 and b"\n" not in x and b"\0" not in x][:count]
    assert len(ln) == count
    ln[3] = ln[17] = ln[18] = b""  # (rows that fail the fake decode: empty messages inside the members)
    return ln


def fake_messages(lines):
    return [(x + b"#" * x.count(b"=") + b"\n") if x else b"" for x in lines]


def run_packed(lib, ctx, lines):
    blob, offs = um.pack(lines)
    buf = np.zeros(blob.size + 32, np.uint8)
    buf[:blob.size] = blob
    ecfg, out = _ecfg(), L.fg_transcoded()
    rc = lib.fg_transcode_batch(ctx.h, 0, L.FG_FRAME_NONE, C.byref(ecfg), buf.ctypes.data, blob.size, offs.ctypes.data, len(lines), 1, C.byref(out))
    return rc, out, len(lines)


def run_multi(lib, ctx, lines):
    segs = [b"".join(x + b"\n" for x in lines[k::3]) for k in range(3)]
    raw = np.frombuffer(b"".join(segs), np.uint8).copy()
    starts = np.cumsum([0] + [len(s) for s in segs]).astype(np.uint64)
    ecfg, out = _ecfg(), L.fg_transcoded_multi()
    rc = lib.fg_transcode_multi_batch(ctx.h, 0, LINE, C.byref(ecfg), raw.ctypes.data, raw.size, starts.ctypes.data, None, 3, C.byref(out))
    return rc, out, int(out.n)


def run_udp(lib, ctx, lines):
    grams = [zlib.compress(x) if i % 2 and x else x for i, x in enumerate(lines)]
    blob, offs = um.pack(grams)
    buf = np.zeros(blob.size + 32, np.uint8)
    buf[:blob.size] = blob
    ecfg, out, ust = _ecfg(), L.fg_transcoded(), vp()
    rc = lib.fg_udp_transcode_batch(ctx.h, 0, C.byref(ecfg), buf.ctypes.data, blob.size, offs.ctypes.data, len(grams), 0, C.byref(out), C.byref(ust))
    return rc, out, len(grams)


ENTRIES = {"packed": run_packed, "multi": run_multi, "udp": run_udp}


def result(out, n):
    return {"out": None if not out.out else _arr(out.out, np.uint8, int(out.out_bytes)).tobytes(), "out_bytes": int(out.out_bytes),
            "out_offsets": _arr(out.out_offsets, np.uint64, n + 1), "meta": _arr(out.meta, np.uint32, n), "enc_status": _arr(out.enc_status, np.uint8, n)}


def counters(lib, reset=True):
    cnt = (C.c_ulonglong * 3)()
    lib.fgf_counters(cnt, int(reset))
    return [int(x) for x in cnt]  # copies, H2D bytes, D2H bytes


def launches(lib, reset=True):
    a = (C.c_ulonglong * 5)()
    lib.fgf_deflate_launches(a, int(reset))
    return [int(x) for x in a]


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_unset_and_none_are_what_they_were(fake, entry):
    """a ctx that never heard of compression, one told FG_COMP_NONE, one told NULL after gzip: the same bytes, offsets and runtime calls,
    none of the compressor's launches, no members reported"""
    lines = lines_of(300)
    seen = []
    for how in ("unset", "none", "null_after_gzip"):
        c = Ctx(fake)
        if how == "none":
            set_compression(fake, c, L.FG_COMP_NONE, 9, 9)
        if how == "null_after_gzip":
            set_compression(fake, c, L.FG_COMP_GZIP, 7)
            assert fake.fg_set_output_compression(c.h, None) == 0
        assert ENTRIES[entry](fake, c, lines)[0] == 0  # (the ctx's buffers exist from here on)
        counters(fake)
        launches(fake)
        c0 = fake.fgf_calls()
        rc, out, n = ENTRIES[entry](fake, c, lines)
        assert rc == 0 and fake.fgf_in_flight() == 0
        r = result(out, n)
        seen.append((r["out"], r["out_offsets"].tolist(), r["meta"].tolist(), r["enc_status"].tolist(), int(fake.fgf_calls() - c0), counters(fake)))
        assert launches(fake) == [0] * 5
        z = compressed(fake, c)
        assert z["n_members"] == 0 and z["null"] and z["raw_bytes"] == 0
        c.close()
    assert seen[0] == seen[1] == seen[2]
    if entry != "multi":
        assert seen[0][0] == b"".join(fake_messages(lines))


@pytest.mark.parametrize("coalesce,member_bytes", POLICIES)
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_gzip_members_in_the_place_of_the_stream(fake, entry, coalesce, member_bytes):
    B = int(fake.fg_deflate_block_bytes())
    lines = lines_of(300)
    c = Ctx(fake)
    rc, out, n = ENTRIES[entry](fake, c, lines)
    assert rc == 0
    plain = result(out, n)
    counters(fake)
    assert ENTRIES[entry](fake, c, lines)[0] == 0
    plain_cnt = counters(fake)
    set_compression(fake, c, L.FG_COMP_GZIP, coalesce, member_bytes)
    assert ENTRIES[entry](fake, c, lines)[0] == 0  # (the compressor's buffers exist from here on)
    counters(fake)
    launches(fake)
    rc, out, n2 = ENTRIES[entry](fake, c, lines)
    assert rc == 0 and fake.fgf_in_flight() == 0 and n2 == n
    gz_cnt = counters(fake)
    assert launches(fake) == [1] * 5
    got = result(out, n)
    assert got["out"] is None and got["out_bytes"] == len(plain["out"]) > 10_000
    for k in ("out_offsets", "meta", "enc_status"):
        assert np.array_equal(got[k], plain[k]), k
    z = compressed(fake, c)
    first, cuts = dm.model_members(plain["out_offsets"], coalesce, member_bytes, B)
    assert np.array_equal(z["member_first"], first) and z["n_members"] == len(first) - 1 and z["raw_bytes"] == len(plain["out"])
    raw = [plain["out"][int(cuts[k]):int(cuts[k + 1])] for k in range(len(cuts) - 1)]
    dm.check_members(raw, z["z"], z["z_offsets"], B, f"{entry} {coalesce} {member_bytes}")
    assert b"".join(zlib.decompress(m, 31) for m in dm.split(z["z"], z["z_offsets"]) if m) == plain["out"]
    # the plain stream does not cross the link: what comes down is the plain call's bytes less the stream, plus the members, their two
    # lists and the few words the compress stage reads (the member count, the error word, the block count, the total: 28 bytes)
    assert gz_cnt[1] == plain_cnt[1]
    assert gz_cnt[2] == plain_cnt[2] - len(plain["out"]) + len(z["z"]) + 16 * (z["n_members"] + 1) + 28
    # ... and back to no compression on the same ctx
    set_compression(fake, c, L.FG_COMP_NONE)
    rc, out, n = ENTRIES[entry](fake, c, lines)
    assert rc == 0 and result(out, n)["out"] == plain["out"] and compressed(fake, c)["n_members"] == 0
    c.close()


def test_nothing_but_dropped_lines_and_an_empty_batch(fake):
    c = Ctx(fake)
    set_compression(fake, c, L.FG_COMP_GZIP, 2)
    rc, out, n = run_packed(fake, c, [b"", b"", b""])
    assert rc == 0 and int(out.out_bytes) == 0 and not out.out
    z = compressed(fake, c)
    assert z["n_members"] == 2 and z["z"].size == 0 and z["z_offsets"].tolist() == [0, 0, 0] and z["member_first"].tolist() == [0, 2, 3]
    rc, out, n = run_packed(fake, c, [b"a=1"])
    assert rc == 0 and compressed(fake, c)["n_members"] == 1
    rc, out, n = run_udp(fake, c, [])
    assert rc == 0 and compressed(fake, c)["n_members"] == 0  # (no call reports the members of the one before it)
    c.close()


def test_argument_errors(fake):
    c = Ctx(fake)
    good = L.fg_compress_cfg(L.FG_COMP_GZIP, 1, 0)
    assert fake.fg_set_output_compression(None, C.byref(good)) == L.FG_ERR_ARG
    assert fake.fg_set_output_compression(c.h, C.byref(L.fg_compress_cfg(2, 1, 0))) == L.FG_ERR_ARG
    assert fake.fg_set_output_compression(c.h, C.byref(L.fg_compress_cfg(-1, 1, 0))) == L.FG_ERR_ARG
    z = L.fg_compressed()
    assert fake.fg_last_compressed(None, C.byref(z)) == L.FG_ERR_ARG and fake.fg_last_compressed(c.h, None) == L.FG_ERR_ARG
    # fg_deflate_device (host arrays play the device)
    members = [b"k=v " * 100, b"", bytes(range(256)) * 3]
    blob, cuts = dm.pack_members(members)
    nbytes, n = int(cuts[-1]), len(members)
    zoff, total = np.zeros(n + 1, np.uint64), u64()
    head = (blob.ctypes.data, nbytes, cuts.ctypes.data, n)
    tail = (zoff.ctypes.data, C.byref(total), vp(-1))
    assert fake.fg_deflate_device(None, *head, None, 0, *tail) == L.FG_ERR_ARG
    assert fake.fg_deflate_device(c.h, None, nbytes, cuts.ctypes.data, n, None, 0, *tail) == L.FG_ERR_ARG
    assert fake.fg_deflate_device(c.h, blob.ctypes.data, nbytes, None, n, None, 0, *tail) == L.FG_ERR_ARG
    assert fake.fg_deflate_device(c.h, *head, None, 0, None, C.byref(total), vp(-1)) == L.FG_ERR_ARG
    assert fake.fg_deflate_device(c.h, *head, None, 0, zoff.ctypes.data, None, vp(-1)) == L.FG_ERR_ARG
    for bad in ([0, 500, 400, nbytes], [0, 400, nbytes + 1], [5, 4]):
        b = np.array(bad, np.uint64)
        assert fake.fg_deflate_device(c.h, blob.ctypes.data, nbytes, b.ctypes.data, len(bad) - 1, None, 0, *tail) == L.FG_ERR_ARG, bad
    assert fake.fg_deflate_device(c.h, *head, None, 0, *tail) == 0 and fake.fgf_in_flight() == 0
    need = int(total.value)
    out = np.full(need + 8, 0xEE, np.uint8)
    assert fake.fg_deflate_device(c.h, *head, out.ctypes.data, need - 1, *tail) == L.FG_ERR_ENT_OVERFLOW and int(total.value) == need and (out == 0xEE).all()
    assert fake.fg_deflate_device(c.h, *head, out.ctypes.data, need, *tail) == 0 and (out[need:] == 0xEE).all()
    dm.check_members(members, out[:need], zoff, int(fake.fg_deflate_block_bytes()), "fg_deflate_device")
    zoff[:] = 9
    assert fake.fg_deflate_device(c.h, *head[:3], 0, None, 0, *tail) == 0 and int(zoff[0]) == 0 and int(total.value) == 0
    c.close()


def test_scratch_grows_and_is_reused(fake):
    c = Ctx(fake)
    set_compression(fake, c, L.FG_COMP_GZIP, 0, 4096)
    caps = (C.c_ulonglong * 4)()
    seen = []
    rng = np.random.default_rng(2)
    big = [bytes(rng.integers(97, 123, 2000, dtype=np.uint8)) for _ in range(1500)]  # (3 MB that compress little: beyond the first buffers)
    for lines in (lines_of(50), lines_of(300), big, lines_of(300), lines_of(50)):
        rc, out, n = run_packed(fake, c, lines)
        assert rc == 0
        z = compressed(fake, c)
        assert b"".join(zlib.decompress(m, 31) for m in dm.split(z["z"], z["z_offsets"]) if m) == b"".join(fake_messages(lines))
        fake.fgf_deflate_caps(c.h, caps)
        seen.append([int(x) for x in caps])
    assert seen[0] == seen[1] and all(a < b for a, b in zip(seen[1][:3], seen[2][:3])) and seen[2] == seen[3] == seen[4]
    c.close()


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_a_failed_runtime_call_at_every_index_leaves_nothing_in_flight_and_the_ctx_usable(fake, entry):
    lines = lines_of(120)
    c = Ctx(fake)
    set_compression(fake, c, L.FG_COMP_GZIP, 0, 4096)
    assert ENTRIES[entry](fake, c, lines)[0] == 0  # (the ctx's buffers exist from here on)
    c0 = fake.fgf_calls()
    rc, out, n = ENTRIES[entry](fake, c, lines)
    calls = int(fake.fgf_calls() - c0)
    first = compressed(fake, c)
    assert rc == 0 and calls >= 25 and first["n_members"] >= 3
    bad = []
    for i in range(1, calls + 1):
        fake.fgf_fail_call_after(i)
        rc, _, _ = ENTRIES[entry](fake, c, lines)
        fake.fgf_fail_call_after(-1)
        why = []
        if rc != L.FG_ERR_HIP:
            why.append(f"rc {rc}")
        if abs(fake.fg_last_hip_error(c.h)) != fake.fgf_last_injected():
            why.append(f"fg_last_hip_error {fake.fg_last_hip_error(c.h)}, injected {fake.fgf_last_injected()}")
        if fake.fgf_in_flight() != 0:
            why.append(f"{fake.fgf_in_flight()} operations in flight")
        rc, out, n = ENTRIES[entry](fake, c, lines)
        again = compressed(fake, c)
        if rc != 0 or not np.array_equal(again["z"], first["z"]) or not np.array_equal(again["member_first"], first["member_first"]):
            why.append(f"the call after it: rc {rc} or another result")
        if why:
            bad.append((i, why))
    c.close()
    assert not bad, f"{len(bad)} of {calls} call indices: {bad}"
