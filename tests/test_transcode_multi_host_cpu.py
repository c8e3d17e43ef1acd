"""CPU: fg_transcode_multi_batch (flowgger_amd/csrc/fg_host_pipeline.cpp) on the fake runtime of test_host_pipeline_cpu.py, built with
the fake FG_CAPNP decode launcher (tests/native/host_pipeline_fake_transcode_multi.cpp).  LINE and NUL run the fake segmented framer;
SYSLEN and CAPNP have none and take their host hop, which is where the host-side cut is proven.  The lists must be the models', and
`out` the concatenation of what fg_transcode_batch on the same fake returns segment by segment (SYSLEN: up to the first row that is
not UTF-8).  The fake decode fails on an empty frame only, so a Cap'n Proto message cannot fail to decode here: that case is the GPU
suite's."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import capnp_frame_binding as B
import oracle_binding
import test_host_pipeline_cpu as H
from capnp_frame_multi_model import model as capnp_model
from flowgger_amd import _lib as L
from frame_multi_model import model as lines_model
from syslen_multi_model import model as syslen_model
from test_host_pipeline_cpu import Ctx
from transcode_multi_model import BAD_UTF8, CARRY, FRAME, UNREACHED, cut

u64, vp = C.c_uint64, C.c_void_p
LIB = H.HERE / "libhost_pipeline_fake_transcode_multi.so"
SRC = [H.HERE / "host_pipeline_fake_transcode_multi.cpp", H.HERE / "host_pipeline_fake_capnp.cpp", H.ROOT / "flowgger_amd/csrc/fg_capnp_next.hpp"] + H.SRC
LINE, NUL, SYSLEN, CAPNP = L.FG_FRAME_LINE, L.FG_FRAME_NUL, L.FG_FRAME_SYSLEN, L.FG_FRAME_CAPNP
PATHS = {LINE: L.FG_PATH_FRAME_MULTI, NUL: L.FG_PATH_FRAME_MULTI, SYSLEN: L.FG_PATH_FRAME_SYSLEN_MULTI_HOST, CAPNP: L.FG_PATH_FRAME_CAPNP_MULTI_HOST}


@pytest.fixture(scope="module")
def fake():
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRC):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-Wno-unused-variable", f"-I{H.HERE / 'fakehip'}", f"-I{H.ROOT / 'include'}", "-o", str(LIB),
                        str(H.HERE / "host_pipeline_fake_transcode_multi.cpp")], check=True)
    lib = C.CDLL(str(LIB))
    lib.fg_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    lib.fg_destroy.argtypes = [vp]
    lib.fg_destroy.restype = None
    lib.fg_last_host_path.argtypes = lib.fg_last_hip_error.argtypes = lib.fg_last_syslen_stop.argtypes = lib.fg_last_capnp_stop.argtypes = [vp]
    lib.fg_transcode_batch.argtypes = [vp, C.c_int, C.c_int, C.POINTER(L.fg_encode_cfg), vp, u64, vp, u64, C.c_int, C.POINTER(L.fg_transcoded)]
    lib.fg_transcode_multi_batch.argtypes = [vp, C.c_int, C.c_int, C.POINTER(L.fg_encode_cfg), vp, u64, vp, vp, u64, C.POINTER(L.fg_transcoded_multi)]
    lib.fgf_fail_call_after.argtypes = [C.c_longlong]
    lib.fgf_calls.restype = lib.fgf_in_flight.restype = lib.fgf_tout_cap.restype = C.c_ulonglong
    lib.fgf_tout_cap.argtypes = [vp]
    return lib


@pytest.fixture(scope="module")
def oracle():
    return oracle_binding.Oracle()


def _arr(p, dt, cnt):
    return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), (cnt * np.dtype(dt).itemsize,)).view(dt).copy() if cnt and p else np.zeros(0, dt)


def _ecfg():
    ecfg = L.fg_encode_cfg()
    ecfg.encoder, ecfg.merger = L.FG_ENC_GELF, L.FG_MERGE_LINE
    return ecfg


def multi(lib, ctx, framing, raw, starts, final=None, fmt=None):
    """-> (rc, dict of copies); FG_OK only with nothing left in flight"""
    fmt = (L.FG_CAPNP if framing == CAPNP else 0) if fmt is None else fmt
    buf = np.frombuffer(raw + bytes(32), np.uint8)
    s = np.asarray(starts, np.uint64)
    fin = None if final is None else np.asarray(final, np.uint8)
    k = len(starts) - 1
    ecfg, out = _ecfg(), L.fg_transcoded_multi()
    rc = lib.fg_transcode_multi_batch(ctx.h, fmt, framing, C.byref(ecfg), buf.ctypes.data, len(raw), s.ctypes.data,
                                      None if fin is None else fin.ctypes.data, k, C.byref(out))
    if rc != 0:
        return rc, None
    assert lib.fgf_in_flight() == 0, f"FG_OK with {lib.fgf_in_flight()} operations in flight"
    n = int(out.n)
    return 0, {"n": n, "out": _arr(out.out, np.uint8, int(out.out_bytes)).tobytes(), "out_offsets": _arr(out.out_offsets, np.uint64, n + 1).tolist(),
               "meta": _arr(out.meta, np.uint32, n), "enc_status": _arr(out.enc_status, np.uint8, n).tolist(),
               "slot_offsets": _arr(out.slot_offsets, np.uint64, n if framing == SYSLEN else n + 1).tolist(),
               "kind": _arr(out.slot_kind, np.uint8, n).tolist(), "seg_first": _arr(out.seg_first, np.uint64, k + 1).tolist(),
               "seg_consumed": _arr(out.seg_consumed, np.uint64, k).tolist(),
               "seg_stop": _arr(out.seg_stop, np.uint8, k).tolist() if out.seg_stop else None, "path": lib.fg_last_host_path(ctx.h)}


def single(lib, ctx, framing, seg, final):
    """fg_transcode_batch on one segment -> (out bytes, dec status per row)"""
    buf = np.frombuffer(seg + bytes(32), np.uint8)
    ecfg, out = _ecfg(), L.fg_transcoded()
    assert lib.fg_transcode_batch(ctx.h, L.FG_CAPNP if framing == CAPNP else 0, framing, C.byref(ecfg), buf.ctypes.data, len(seg), None, 0, int(final),
                                  C.byref(out)) == 0
    n = int(out.n)
    offs, st = _arr(out.out_offsets, np.uint64, n + 1), _arr(out.meta, np.uint32, n) & 0xFF
    blob = _arr(out.out, np.uint8, int(out.out_bytes)).tobytes()
    if framing == SYSLEN and (st == L.FG_ST_BAD_UTF8).any():  # the connection ends at its first payload that is not UTF-8
        blob = blob[:int(offs[int(np.argmax(st == L.FG_ST_BAD_UTF8))])]
    return blob


def starts_of(segs):
    return [0] + np.cumsum([len(s) for s in segs]).tolist()


def wrap(msgs):
    return b"".join(b"%d %s" % (len(m), m) for m in msgs)


def case(framing, oracle):
    """-> (raw, seg_starts, seg_final, model dict with kind / slot_offsets / seg_*): every hazard in one buffer.  A frame with a byte
    >= 0xF8 is what the fake framer flags, and no UTF-8 either; an empty frame is what the fake decode fails on."""
    ln = [x for x in H.corpus(120, np.random.default_rng(5)) if x]
    if framing in (LINE, NUL):
        t = b"\n" if framing == LINE else b"\0"
        text = lambda a, b: b"".join(x + t for x in ln[a:b])
        segs = [text(0, 30), b"", text(30, 40) + b"<1>tail a=1", t + text(40, 50) + b"bad \xff\xfe" + t + text(50, 60) + b"<2>cut off b=", b"z",
                text(60, 70) + (b"crlf a=1\r\n" if framing == LINE else b"") + t, text(70, 100)]
        final = [0, 0, 1, 0, 0, 1, 0]
        raw, starts = b"".join(segs), starts_of(segs)
        m = lines_model(oracle, raw, starts, final, 0 if framing == LINE else 1)
        want = {"kind": m.kind.tolist(), "slot_offsets": m.offsets.tolist(), "seg_first": m.seg_first.tolist(), "seg_consumed": m.seg_consumed.tolist(),
                "seg_stop": None}
        empties = sum(raw[a:b] == t for a, b, k in zip(want["slot_offsets"], want["slot_offsets"][1:], want["kind"]) if k == FRAME)
        assert want["kind"].count(CARRY) == 2 and want["kind"].count(BAD_UTF8) == 1 and empties >= 2 and want["kind"].count(FRAME) > 90
        return raw, starts, final, want
    if framing == SYSLEN:
        bad = b"x\xff\xfe"
        segs = [wrap(ln[0:10] + [b""] + ln[10:20]), b"", wrap(ln[20:25] + [bad] + ln[25:30] + [bad, b""]), wrap([bad] + ln[30:33]), wrap(ln[33:40] + [b""]) + b"12",
                wrap(ln[40:45]) + b" x", wrap(ln[45:60] + [bad]), b"", wrap([b"a=1", bad, b"b=2", b"c=3"]), b"1 a" + b"0" * 40 + b"2 bc" + b"3 de"]
        raw, starts = b"".join(segs), starts_of(segs)
        m = syslen_model(raw, starts, None)
        kind = cut(m["bad"], m["seg_first"])
        assert kind.count(BAD_UTF8) == 4 and kind.count(UNREACHED) == 7 + 3 + 2 and m["payloads"].count(b"") == 3 and kind.count(FRAME) > 50
        assert kind[m["seg_first"][8]:m["seg_first"][9]] == [FRAME, BAD_UTF8, UNREACHED, UNREACHED] and set(m["seg_stop"]) == {0, 1, 2}
        return raw, starts, None, {"kind": kind, "slot_offsets": m["starts"], "seg_first": m["seg_first"], "seg_consumed": m["seg_consumed"],
                                   "seg_stop": m["seg_stop"]}
    body = lambda k: B.msg(k % 9 + 1, fill=b"k%d=v " % k)
    segs = [b"".join(body(k) for k in range(20)), b"", body(1) + body(2)[:-8], B.msg(0) * 5 + struct.pack("<2I", 511, 0) + bytes(24),
            b"".join(body(k) for k in range(20, 50)), body(7) + b"abc"]
    raw, starts = b"".join(segs), starts_of(segs)
    m = capnp_model(raw, starts)
    assert m["kind"].count(CARRY) == 3 and m["kind"].count(FRAME) > 50 and 2 in m["seg_stop"]
    return raw, starts, None, {"kind": m["kind"], "slot_offsets": m["offsets"], "seg_first": m["seg_first"], "seg_consumed": m["seg_consumed"],
                               "seg_stop": m["seg_stop"]}


def same(r, want):
    for key in ("kind", "slot_offsets", "seg_first", "seg_consumed", "seg_stop"):
        assert r[key] == want[key], key
    assert r["n"] == len(want["kind"])


@pytest.mark.parametrize("framing", [LINE, NUL, SYSLEN, CAPNP], ids=["line", "nul", "syslen", "capnp"])
def test_the_lists_are_the_models_and_the_stream_is_the_segments_streams(fake, oracle, framing):
    raw, starts, final, want = case(framing, oracle)
    c, ref = Ctx(fake), Ctx(fake)
    stops = fake.fg_last_syslen_stop(c.h), fake.fg_last_capnp_stop(c.h)
    rc, r = multi(fake, c, framing, raw, starts, final)
    assert rc == 0 and r["path"] == PATHS[framing]
    assert (fake.fg_last_syslen_stop(c.h), fake.fg_last_capnp_stop(c.h)) == stops
    same(r, want)
    pieces = [single(fake, ref, framing, raw[a:b], final[k] if final else 0) for k, (a, b) in enumerate(zip(starts, starts[1:]))]
    assert r["out"] == b"".join(pieces) and len(r["out"]) > len(raw) // 2
    # every slot: a skipped row produces nothing, and the stream is the messages back to back
    st = r["meta"] & 0xFF
    for i, k in enumerate(r["kind"]):
        size = r["out_offsets"][i + 1] - r["out_offsets"][i]
        if k != FRAME:
            assert st[i] == L.FG_ST_BAD_UTF8 and r["enc_status"][i] == 1 and size == 0, i
        else:
            assert (size > 0) == (st[i] == 0) == (r["enc_status"][i] == 0), i
    assert r["out_offsets"][0] == 0 and r["out_offsets"][-1] == len(r["out"])
    if framing != CAPNP:
        assert sum(1 for i, k in enumerate(r["kind"]) if k == FRAME and st[i] != 0) >= 2  # (frames that fail to decode)
    # per segment: its slots' messages are its own stream
    for k, piece in enumerate(pieces):
        a, b = r["seg_first"][k], r["seg_first"][k + 1]
        assert r["out"][r["out_offsets"][a]:r["out_offsets"][b]] == piece, k
    c.close()
    ref.close()


@pytest.mark.parametrize("framing", [LINE, SYSLEN, CAPNP], ids=["line", "syslen", "capnp"])
def test_no_segments_and_segments_without_bytes(fake, framing):
    c = Ctx(fake)
    for starts in ([0], [0, 0, 0, 0]):
        rc, r = multi(fake, c, framing, b"", starts, [1, 0, 0][:len(starts) - 1] if framing == LINE else None)
        assert rc == 0 and r["n"] == 0 and r["out"] == b"" and r["out_offsets"] == [0] and r["seg_first"] == [0] * len(starts)
        assert r["seg_consumed"] == [0] * (len(starts) - 1) and r["kind"] == []
    c.close()


def test_an_output_buffer_one_byte_too_small_is_grown_and_the_encode_runs_again(fake):
    c = Ctx(fake)
    rc, r = multi(fake, c, LINE, b"<1>a\n", [0, 5], [0])
    cap = int(fake.fgf_tout_cap(c.h))
    assert rc == 0 and r["out"] == b"<1>a\n\n" and cap >= 4096
    # the fake encoder writes a slot and one byte more: `rows` slots of 1024 bytes, and a last one that makes the stream cap + delta
    for delta in (0, 1):
        rows = cap // 1025 - 1
        rest = cap + delta - rows * 1025
        lines = [b"x" * 1023 + b"\n"] * rows + [b"y" * (rest - 2) + b"\n"]
        segs = [b"".join(lines[:7]), b"".join(lines[7:])]
        before = int(fake.fgf_tout_cap(c.h))
        rc, r = multi(fake, c, LINE, b"".join(segs), starts_of(segs), [0, 0])
        assert rc == 0 and len(r["out"]) == cap + delta and r["n"] == rows + 1 and r["out"] == b"".join(x + b"\n" for x in lines)
        assert (int(fake.fgf_tout_cap(c.h)) > before) == bool(delta)
    c.close()


@pytest.mark.parametrize("framing", [LINE, SYSLEN, CAPNP], ids=["line", "syslen", "capnp"])
def test_a_failed_runtime_call_at_every_index_leaves_nothing_in_flight_and_the_ctx_usable(fake, oracle, framing):
    raw, starts, final, want = case(framing, oracle)
    c = Ctx(fake)
    rc, first = multi(fake, c, framing, raw, starts, final)  # (the ctx's buffers exist from here on)
    assert rc == 0
    c0 = fake.fgf_calls()
    rc, first = multi(fake, c, framing, raw, starts, final)
    calls = int(fake.fgf_calls() - c0)
    assert rc == 0 and calls >= 12
    bad = []
    for i in range(1, calls + 1):
        fake.fgf_fail_call_after(i)
        rc, _ = multi(fake, c, framing, raw, starts, final)
        fake.fgf_fail_call_after(-1)
        why = []
        if rc != L.FG_ERR_HIP:
            why.append(f"rc {rc}")
        if abs(fake.fg_last_hip_error(c.h)) != fake.fgf_last_injected():
            why.append(f"fg_last_hip_error {fake.fg_last_hip_error(c.h)}, injected {fake.fgf_last_injected()}")
        if fake.fgf_in_flight() != 0:
            why.append(f"{fake.fgf_in_flight()} operations in flight")
        if fake.fg_last_host_path(c.h) != 0:
            why.append("a host path is reported")
        rc, again = multi(fake, c, framing, raw, starts, final)
        if rc != 0 or any(np.asarray(again[k] != first[k]).any() for k in first):
            why.append(f"the call after it: rc {rc} or another result")
        if why:
            bad.append((i, why))
    c.close()
    assert not bad, f"{len(bad)} of {calls} call indices: {bad}"


def test_argument_errors(fake):
    c = Ctx(fake)
    raw = b"<1>a\n<2>b\n"
    ok = lambda *a, **k: multi(fake, c, *a, **k)[0]
    assert ok(LINE, raw, [0, 5, 10], [0, 1]) == 0
    assert ok(L.FG_FRAME_NONE, raw, [0, 10]) == L.FG_ERR_ARG                      # a packed batch is fg_transcode_batch's
    assert ok(7, raw, [0, 10]) == L.FG_ERR_ARG
    assert ok(LINE, raw, [0, 10], fmt=L.FG_CAPNP) == L.FG_ERR_ARG                 # a bad framing / format pair, either way
    assert ok(SYSLEN, raw, [0, 10], fmt=L.FG_CAPNP) == L.FG_ERR_ARG
    m = B.msg(1) * 4
    assert ok(CAPNP, m, [0, len(m)], fmt=0) == L.FG_ERR_ARG
    assert ok(SYSLEN, b"4 <1>a", [0, 6], [1]) == L.FG_ERR_ARG                     # seg_final is LINE's and NUL's
    assert ok(CAPNP, m, [0, len(m)], [0]) == L.FG_ERR_ARG
    for framing in (LINE, NUL, SYSLEN):                                           # lists that do not tile the buffer
        for starts in ([1, 10], [0, 9], [0, 7, 3, 10], [0, 11]):
            assert ok(framing, raw, starts) == L.FG_ERR_ARG
    for starts in ([0, 12, len(m)], [0, 16, 17, len(m)], [8, len(m)], [0, len(m) + 8]):  # a Cap'n Proto start off a word
        assert ok(CAPNP, m, starts) == L.FG_ERR_ARG
    assert ok(CAPNP, m, [0, 16, len(m)]) == 0 and ok(SYSLEN, b"4 <1>a", [0, 6]) == 0
    c.close()
