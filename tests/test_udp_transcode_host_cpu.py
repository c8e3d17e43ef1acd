"""CPU: fg_udp_transcode_batch (flowgger_amd/csrc/fg_host_pipeline.cpp) on the fake runtime of test_host_pipeline_cpu.py, built with
host loops over fg_inflate.hpp in the place of the one-walk UDP kernels (tests/native/host_pipeline_fake_udp.cpp).  The unpack is the
real core, so which datagram is dropped and why is held against the model of tests/udp_model.py; the decode and the encoder behind
it are the fakes of host_pipeline_fake.cpp (an Ok row's message is its payload, one '#' per '=' and a newline; an empty payload
fails to decode), so the stream is held against that rule applied to the model's payloads -- what the real decoders and encoders
make of them is the GPU suite's (tests/test_gpu_udp_transcode.py, against the oracle)."""
import ctypes as C
import gzip
import subprocess
import zlib

import numpy as np
import pytest

import test_host_pipeline_cpu as H
import udp_model as um
from flowgger_amd import _lib as L
from test_host_pipeline_cpu import Ctx
from test_inflate_once_cpu import policy_w

u64, vp = C.c_uint64, C.c_void_p
LIB = H.HERE / "libhost_pipeline_fake_udp.so"
SRC = [H.HERE / "host_pipeline_fake_udp.cpp", H.ROOT / "flowgger_amd/csrc/fg_inflate.hpp", H.ROOT / "flowgger_amd/csrc/fg_utf8.hpp"] + H.SRC


@pytest.fixture(scope="module")
def fake():
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRC):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-Wno-unused-variable", f"-I{H.HERE / 'fakehip'}", f"-I{H.ROOT / 'include'}", "-o", str(LIB), str(SRC[0])], check=True)
    lib = C.CDLL(str(LIB))
    lib.fg_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    lib.fg_destroy.argtypes = [vp]
    lib.fg_destroy.restype = None
    lib.fg_last_host_path.argtypes = lib.fg_last_hip_error.argtypes = lib.fg_udp_last_spilled.argtypes = [vp]
    lib.fg_udp_last_spilled.restype = u64
    lib.fg_transcode_batch.argtypes = [vp, C.c_int, C.c_int, C.POINTER(L.fg_encode_cfg), vp, u64, vp, u64, C.c_int, C.POINTER(L.fg_transcoded)]
    lib.fg_udp_transcode_batch.argtypes = [vp, C.c_int, C.POINTER(L.fg_encode_cfg), vp, u64, vp, u64, u64, C.POINTER(L.fg_transcoded), C.POINTER(vp)]
    lib.fgf_fail_call_after.argtypes = [C.c_longlong]
    lib.fgf_calls.restype = lib.fgf_in_flight.restype = lib.fgf_packed_cap.restype = C.c_ulonglong
    lib.fgf_packed_cap.argtypes = [vp]
    return lib


def _arr(p, dt, cnt):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (cnt * np.dtype(dt).itemsize,)).view(dt).copy() if cnt and p else np.zeros(0, dt)


def _ecfg():
    ecfg = L.fg_encode_cfg()
    ecfg.encoder, ecfg.merger = L.FG_ENC_GELF, L.FG_MERGE_LINE
    return ecfg


def launches(lib, reset=False):
    a = (C.c_ulonglong * 3)()
    lib.fgf_udp_launches(a, int(reset))
    return list(a)


def run(lib, ctx, grams, max_inflated=0, fmt=0, offsets=None, nbytes=None, null=()):
    """-> (rc, dict of copies); FG_OK only with nothing left in flight"""
    blob, offs = um.pack(grams)
    if offsets is not None:
        offs = np.asarray(offsets, np.uint64)
    buf = np.zeros(blob.size + 32, np.uint8)
    buf[:blob.size] = blob
    ecfg, out, ust = _ecfg(), L.fg_transcoded(), vp()
    n = len(offs) - 1
    rc = lib.fg_udp_transcode_batch(None if "ctx" in null else ctx.h, fmt, None if "cfg" in null else C.byref(ecfg), None if "bytes" in null else buf.ctypes.data,
                                    blob.size if nbytes is None else nbytes, None if "offsets" in null else offs.ctypes.data, n, max_inflated,
                                    None if "out" in null else C.byref(out), None if "status" in null else C.byref(ust))
    if rc != 0:
        return rc, None
    assert lib.fgf_in_flight() == 0, f"FG_OK with {lib.fgf_in_flight()} operations in flight"
    assert int(out.n) == n and int(out.consumed) == blob.size and not out.frame_offsets
    return 0, {"out": _arr(out.out, np.uint8, int(out.out_bytes)).tobytes(), "out_offsets": _arr(out.out_offsets, np.uint64, n + 1 if n else 0).tolist(),
               "meta": _arr(out.meta, np.uint32, n), "enc_status": _arr(out.enc_status, np.uint8, n).tolist(), "udp_status": _arr(ust, np.uint8, n).tolist()}


def expected(grams, max_inflated=um.DEFAULT_MAX):
    """the model's verdicts, and the fake decode + encode over the model's payloads"""
    st, kept, slots = um.expect(grams, max_inflated)
    msgs = [(p + b"#" * p.count(b"=") + b"\n") if k and p else b"" for k, p in zip(kept, slots)]
    dec = [L.FG_ST_BAD_UTF8 if not k else 0 if p else 1 for k, p in zip(kept, slots)]
    return st.tolist(), dec, msgs


def mixed():
    """about 40 datagrams: bare, zlib, gzip, every drop reason, an empty payload, streams that outgrow their stage"""
    ln = [x for x in H.corpus(30, np.random.default_rng(11)) if x and max(x) < 0x80]
    assert len(ln) >= 20
    cases = dict(um.case_list())
    grams = []
    for i, x in enumerate(ln[:24]):
        grams.append(x if i % 3 == 0 else zlib.compress(x, (0, 1, 6, 9)[i % 4]) if i % 3 == 1 else gzip.compress(x, mtime=0))
    grams += [cases[k] for k in ("raw_bad_utf8", "zlib_bad_utf8", "gzip_cut_utf8", "zlib_bad_adler", "gz_bad_crc32", "gz_isize_cut", "ref_gzip_trunc5",
                                 "empty", "zlib_trailing", "gz_all4")]
    grams += [zlib.compress(b""), zlib.compress(b"k=v " * 5000), gzip.compress(b"a=b " * 3000, mtime=0), zlib.compress(b"q" * 400_000)]
    bad = bytearray(zlib.compress(b"z=1 " * 5000))
    bad[-1] ^= 1
    grams.append(bytes(bad))
    return grams


def spills(grams, max_inflated=um.DEFAULT_MAX):
    """from the model's sizes and the policy alone: the datagrams whose slot is larger than their stage"""
    return sum(1 for d, s in zip(grams, um.expect(grams, max_inflated)[2]) if len(s) > policy_w(d, max_inflated) and um.gate(d) != um.RAW)


def same(r, grams, max_inflated=um.DEFAULT_MAX):
    st, dec, msgs = expected(grams, max_inflated)
    assert r["udp_status"] == st
    assert (r["meta"] & 0xFF).tolist() == dec
    assert r["enc_status"] == [0 if m else 1 for m in msgs]
    assert r["out"] == b"".join(msgs) and r["out_offsets"] == [0] + np.cumsum([len(m) for m in msgs]).tolist()


def test_mixed_datagrams(fake):
    grams = mixed()
    st = um.expect(grams)[0].tolist()
    assert len(grams) >= 38 and set(st) == set(range(7)), sorted(set(st))  # (every fg_udp_status is in the batch)
    c = Ctx(fake)
    launches(fake, reset=True)
    rc, r = run(fake, c, grams)
    assert rc == 0
    same(r, grams)
    assert launches(fake) == [1, 1, 1] and fake.fg_udp_last_spilled(c.h) == spills(grams) >= 3  # (k=v, a=b, the wrong checksum at least)
    assert sum(1 for m in expected(grams)[2] if m) > 25
    # the same ctx takes a packed batch right after, and datagrams again (the buffers are shared)
    lines = [g for g in grams if um.gate(g) == um.RAW and um.model(g)[2] and g]
    blob, offs = um.pack(lines)
    buf = np.zeros(blob.size + 32, np.uint8)
    buf[:blob.size] = blob
    ecfg, out = _ecfg(), L.fg_transcoded()
    assert fake.fg_transcode_batch(c.h, 0, L.FG_FRAME_NONE, C.byref(ecfg), buf.ctypes.data, blob.size, offs.ctypes.data, len(lines), 1, C.byref(out)) == 0
    assert _arr(out.out, np.uint8, int(out.out_bytes)).tobytes() == b"".join(x + b"#" * x.count(b"=") + b"\n" for x in lines)
    rc, r = run(fake, c, grams[::-1])
    assert rc == 0
    same(r, grams[::-1])
    c.close()


def test_small_cap_and_no_kept_datagram(fake):
    c = Ctx(fake)
    grams = mixed()
    rc, r = run(fake, c, grams, 300)
    assert rc == 0
    same(r, grams, 300)
    none = [b"\xff", zlib.compress(b"abc")[:-1], b"\xc3"]
    rc, r = run(fake, c, none)
    assert rc == 0 and r["out"] == b"" and r["out_offsets"] == [0, 0, 0, 0] and r["udp_status"] == [um.BAD_UTF8, um.BAD_ZLIB, um.BAD_UTF8]
    assert r["enc_status"] == [1, 1, 1] and (r["meta"] & 0xFF).tolist() == [L.FG_ST_BAD_UTF8] * 3
    rc, r = run(fake, c, [zlib.compress(b"one=1")])
    assert rc == 0 and r["out"] == b"one=1#\n"
    c.close()


def test_no_datagrams(fake):
    c = Ctx(fake)
    calls = fake.fgf_calls()
    rc, r = run(fake, c, [])
    assert rc == 0 and r["out"] == b"" and r["udp_status"] == [] and fake.fgf_calls() == calls
    c.close()


def test_argument_errors(fake):
    c = Ctx(fake)
    g = [b"<1>a", zlib.compress(b"<2>b")]
    n = sum(map(len, g))
    assert run(fake, c, g)[0] == 0
    for null in ("ctx", "cfg", "bytes", "offsets", "out", "status"):
        assert run(fake, c, g, null=(null,))[0] == L.FG_ERR_ARG, null
    assert run(fake, c, g, fmt=L.FG_CAPNP)[0] == L.FG_ERR_ARG and run(fake, c, g, fmt=9)[0] == L.FG_ERR_ARG
    for offs in ([1, 4, n], [0, 4, n - 1], [0, n, 4], [0, 4, n + 1]):
        assert run(fake, c, g, offsets=offs)[0] == L.FG_ERR_ARG, offs
    assert run(fake, c, g, max_inflated=0x7FFFFFF1)[0] == L.FG_ERR_ARG
    assert run(fake, c, g, max_inflated=0x7FFFFFF0)[0] == 0
    c.close()


def test_a_packed_buffer_one_byte_too_small_is_grown_and_the_walk_is_not_repeated(fake):
    c = Ctx(fake)
    assert run(fake, c, [b"a=1"])[0] == 0
    cap = int(fake.fgf_packed_cap(c.h))
    assert cap >= 1 << 20
    big = [zlib.compress(bytes([65 + k]) * 3 + b"=v " * 6000) for k in range(8)]  # 18 003 bytes each, all spilled
    for delta in (0, 1):
        total = cap - 16 + delta  # (the buffer holds the payloads rounded up to 16, and 16 bytes of pad)
        rest = total - 8 * 18_003
        grams = big[:4] + [b"x" * 1000] * (rest // 1000 - 1) + big[4:] + [b"y" * (rest - (rest // 1000 - 1) * 1000)]
        assert sum(len(s) for s in um.expect(grams)[2]) == total
        before = int(fake.fgf_packed_cap(c.h))
        launches(fake, reset=True)
        rc, r = run(fake, c, grams)
        assert rc == 0
        same(r, grams)
        assert (int(fake.fgf_packed_cap(c.h)) > before) == bool(delta)
        assert launches(fake) == [1, 1, 1] and fake.fg_udp_last_spilled(c.h) == spills(grams) == 8  # (one walk, whatever the buffer was)
    c.close()


def test_a_failed_runtime_call_at_every_index_leaves_nothing_in_flight_and_the_ctx_usable(fake):
    grams = mixed()
    c = Ctx(fake)
    assert run(fake, c, grams)[0] == 0  # (the ctx's buffers exist from here on)
    c0 = fake.fgf_calls()
    rc, first = run(fake, c, grams)
    calls = int(fake.fgf_calls() - c0)
    assert rc == 0 and calls >= 12
    bad = []
    for i in range(1, calls + 1):
        fake.fgf_fail_call_after(i)
        rc, _ = run(fake, c, grams)
        fake.fgf_fail_call_after(-1)
        why = []
        if rc != L.FG_ERR_HIP:
            why.append(f"rc {rc}")
        if abs(fake.fg_last_hip_error(c.h)) != fake.fgf_last_injected():
            why.append(f"fg_last_hip_error {fake.fg_last_hip_error(c.h)}, injected {fake.fgf_last_injected()}")
        if fake.fgf_in_flight() != 0:
            why.append(f"{fake.fgf_in_flight()} operations in flight")
        rc, again = run(fake, c, grams)
        if rc != 0 or any(np.asarray(again[k] != first[k]).any() for k in first):
            why.append(f"the call after it: rc {rc} or another result")
        if why:
            bad.append((i, why))
    c.close()
    assert not bad, f"{len(bad)} of {calls} call indices: {bad}"
