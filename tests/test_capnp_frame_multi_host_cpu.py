"""CPU: fg_frame_decode_capnp_multi_batch (flowgger_amd/csrc/fg_host_pipeline.cpp) on the fake runtime of test_host_pipeline_cpu.py, with
a fake FG_CAPNP decode launcher beside the others (tests/native/host_pipeline_fake_capnp.cpp).  The fake has no framer, so the device
entry answers FG_ERR_UNSUPPORTED and the call walks every segment on the host: the slots and the segments must be the model's, and the
rows of the FRAME slots those of one device call on the same messages."""
import ctypes as C
import struct
import subprocess

import numpy as np
import pytest

import capnp_frame_binding as B
import test_host_pipeline_cpu as H
from capnp_frame_binding import CLEAN, TAIL, TOO_LARGE, TOO_MANY_SEGMENTS
from capnp_frame_multi_model import CARRY, FRAME, model
from flowgger_amd import _lib as L
from test_host_pipeline_cpu import Ctx, device_reference, snapshot

u64, vp = C.c_uint64, C.c_void_p
LIB = H.HERE / "libhost_pipeline_fake_capnp.so"
SRC = [H.HERE / "host_pipeline_fake_capnp.cpp", H.ROOT / "flowgger_amd/csrc/fg_capnp_next.hpp"] + H.SRC


@pytest.fixture(scope="module")
def fake():
    if not LIB.exists() or any(s.stat().st_mtime > LIB.stat().st_mtime for s in SRC):
        subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas",
                        "-Wno-unused-variable", f"-I{H.HERE / 'fakehip'}", f"-I{H.ROOT / 'include'}", "-o", str(LIB),
                        str(H.HERE / "host_pipeline_fake_capnp.cpp")], check=True)
    lib = C.CDLL(str(LIB))
    lib.fg_create.argtypes = [C.c_int, vp, C.POINTER(vp)]
    lib.fg_destroy.argtypes = [vp]
    lib.fg_destroy.restype = None
    lib.fg_tables_layout.argtypes = [u64, u64, C.POINTER(u64)]
    lib.fg_decode_batch_device.argtypes = [vp, C.c_int, vp, u64, vp, u64, C.POINTER(L.fg_tables), vp]
    lib.fg_last_host_path.argtypes = [vp]
    lib.fg_frame_decode_capnp_multi_batch.argtypes = [vp, vp, u64, vp, u64, C.POINTER(L.fg_tables), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                                      C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    return lib


def call(lib, ctx, raw, starts):
    buf = np.frombuffer(raw + bytes(32), np.uint8)
    s = np.asarray(starts, np.uint64)
    st = L.fg_tables()
    off, kind, first, cons, stop, n = vp(), vp(), vp(), vp(), vp(), u64()
    rc = lib.fg_frame_decode_capnp_multi_batch(ctx.h, buf.ctypes.data, len(raw), s.ctypes.data, len(starts) - 1, C.byref(st), C.byref(off),
                                               C.byref(kind), C.byref(first), C.byref(cons), C.byref(stop), C.byref(n))
    if rc != 0:
        return rc, None
    k, ns = len(starts) - 1, int(n.value)
    arr = lambda p, t, cnt: np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), (cnt,)).copy() if cnt else np.zeros(0, t)
    return 0, {"n": ns, "tables": st, "offsets": arr(off, C.c_uint64, ns + 1), "kind": arr(kind, C.c_uint8, ns),
               "seg_first": arr(first, C.c_uint64, k + 1), "seg_consumed": arr(cons, C.c_uint64, k), "seg_stop": arr(stop, C.c_uint8, k),
               "path": lib.fg_last_host_path(ctx.h)}


def segments():
    """bodies hold '=' signs, which the fake decode turns into entries"""
    body = lambda k: B.msg(k % 9 + 1, fill=b"k%d=v " % k)
    segs = [b"".join(body(k) for k in range(60)), b"", body(1) + body(2)[:-8], B.msg(0) * 5 + struct.pack("<2I", 511, 0) + bytes(24),
            body(3) + struct.pack("<4I", 1, B.MAX_WORDS - 5, 6, 0) + bytes(16), b"".join(body(k) for k in range(60, 200)), body(7) + b"abc"]
    starts = [0]
    for s in segs:
        starts.append(starts[-1] + len(s))
    return b"".join(segs), starts


def test_the_host_walk_yields_the_models_slots_and_the_decode_of_the_walked_messages(fake):
    raw, starts = segments()
    m = model(raw, starts)
    assert m["seg_stop"] == [CLEAN, CLEAN, TAIL, TOO_MANY_SEGMENTS, TOO_LARGE, CLEAN, TAIL]
    c = Ctx(fake)
    rc, r = call(fake, c, raw, starts)
    assert rc == 0 and r["path"] == L.FG_PATH_FRAME_CAPNP_MULTI_HOST == 14
    assert r["n"] == m["n"] and list(r["offsets"]) == m["offsets"] and list(r["kind"]) == m["kind"]
    assert list(r["seg_first"]) == m["seg_first"] and list(r["seg_consumed"]) == m["seg_consumed"] and list(r["seg_stop"]) == m["seg_stop"]
    got = snapshot(r["tables"], r["n"])
    fr, ca = np.nonzero(r["kind"] == FRAME)[0], np.nonzero(r["kind"] == CARRY)[0]
    msgs = [raw[m["offsets"][i]:m["offsets"][i + 1]] for i in fr]
    offs = np.zeros(len(msgs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(x) for x in msgs])
    want = device_reference(fake, np.frombuffer(b"".join(msgs), np.uint8).copy(), offs, len(raw) // 2 + 1024)
    assert len(ca) == 4 and int(want["ent_count"].sum()) > 100
    for col in H.COLS:
        assert np.array_equal(got[col][fr], want[col][:len(fr)]), col
    for j, i in enumerate(fr):
        fa, fb, k = int(got["ent_first"][i]), int(want["ent_first"][j]), int(got["ent_count"][i])
        for col in ("ent_name", "ent_val", "ent_type", "ent_flags"):
            assert np.array_equal(got[col][fa:fa + k], want[col][fb:fb + k]), (col, int(i))
    assert ((got["meta"][ca] & 0xFF) == L.FG_ST_BAD_UTF8).all() and (got["ent_count"][ca] == 0).all()
    # a second call on the same ctx, without frames and without segments
    rc, r = call(fake, c, B.msg(3)[:16], [0, 16])
    assert rc == 0 and r["n"] == 1 and list(r["kind"]) == [CARRY] and list(r["seg_stop"]) == [TAIL] and list(r["seg_first"]) == [0, 1]
    rc, r = call(fake, c, b"", [0])
    assert rc == 0 and r["n"] == 0
    c.close()


def test_a_misaligned_or_non_tiling_list_is_an_argument_error(fake):
    c = Ctx(fake)
    raw = B.msg(1) * 4
    for starts in ([8, len(raw)], [0, len(raw) - 8], [0, 32, 16, len(raw)], [0, len(raw) + 8], [0, 12, len(raw)], [0, 16, 17, len(raw)]):
        assert call(fake, c, raw, starts)[0] == L.FG_ERR_ARG
    assert call(fake, c, raw[:-3], [0, 16, len(raw) - 3])[0] == 0  # (only the end may lie off a word)
    c.close()
