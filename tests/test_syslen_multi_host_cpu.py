"""CPU: fg_frame_decode_syslen_multi_batch (flowgger_amd/csrc/fg_host_pipeline.cpp) on the fake runtime of test_host_pipeline_cpu.py.
The fake launchers have no octet-counted framer, so the device entry answers FG_ERR_UNSUPPORTED and the call takes its host hop,
segment by segment: the segments must be the model's, and the decode that of the hopped messages."""
import ctypes as C

import numpy as np

from flowgger_amd import _lib as L
from syslen_binding import BAD_LEN, CLEAN, TAIL
from syslen_multi_model import model
from test_host_pipeline_cpu import Ctx, corpus, device_reference, fake, same_lines, snapshot  # noqa: F401  (fake: the fixture)

u64, vp = C.c_uint64, C.c_void_p


def wrap(msgs):
    return b"".join(b"%d %s" % (len(m), m) for m in msgs)


def call(lib, ctx, fmt, raw, starts):
    lib.fg_frame_decode_syslen_multi_batch.argtypes = [vp, C.c_int, vp, u64, vp, u64, C.POINTER(L.fg_tables), C.POINTER(vp), C.POINTER(vp),
                                                       C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    lib.fg_last_host_path.argtypes = [vp]
    buf = np.frombuffer(raw + bytes(32), np.uint8)
    s = np.asarray(starts, np.uint64)
    st = L.fg_tables()
    fs, first, cons, stop, n = vp(), vp(), vp(), vp(), u64()
    rc = lib.fg_frame_decode_syslen_multi_batch(ctx.h, fmt, buf.ctypes.data, len(raw), s.ctypes.data, len(starts) - 1, C.byref(st), C.byref(fs),
                                                C.byref(first), C.byref(cons), C.byref(stop), C.byref(n))
    if rc != 0:
        return rc, None
    k, nf = len(starts) - 1, int(n.value)
    arr = lambda p, t, cnt: np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), (cnt,)).copy() if cnt else np.zeros(0, t)
    return 0, {"n": nf, "tables": st, "starts": arr(fs, C.c_uint64, nf), "seg_first": arr(first, C.c_uint64, k + 1),
               "seg_consumed": arr(cons, C.c_uint64, k), "seg_stop": arr(stop, C.c_uint8, k), "path": lib.fg_last_host_path(ctx.h)}


def segments(rng):
    msgs = corpus(400, rng)
    segs = [wrap(msgs[0:100]), b"", wrap(msgs[100:180]) + b"12", b" x", wrap(msgs[180:181]) + b"700 short", b"7", wrap(msgs[181:400]),
            b"1 a" + b"0" * 40 + b"2 bc" + b"3 de"]  # (a prefix of 42 bytes: the host hop reads prefixes of any length)
    starts = [0]
    for s in segs:
        starts.append(starts[-1] + len(s))
    return b"".join(segs), starts


def test_the_host_hop_yields_the_models_segments_and_the_decode_of_the_hopped_messages(fake):
    raw, starts = segments(np.random.default_rng(3))
    m = model(raw, starts, None)
    assert m["seg_stop"] == [CLEAN, CLEAN, TAIL, BAD_LEN, TAIL, TAIL, CLEAN, TAIL]
    c = Ctx(fake)
    rc, r = call(fake, c, 0, raw, starts)
    assert rc == 0 and r["path"] == L.FG_PATH_FRAME_SYSLEN_MULTI_HOST
    assert r["n"] == m["n"] and list(r["starts"]) == m["starts"]
    assert list(r["seg_first"]) == m["seg_first"] and list(r["seg_consumed"]) == m["seg_consumed"] and list(r["seg_stop"]) == m["seg_stop"]
    got = snapshot(r["tables"], r["n"])
    packed, offs = np.frombuffer(m["packed"], np.uint8).copy(), np.asarray(m["offsets"], np.uint64)
    want = device_reference(fake, packed, offs, len(packed) // 8 + 1024)
    same_lines(got, want, r["n"])
    # a second call on the same ctx, without frames and without segments
    rc, r = call(fake, c, 0, b"5 ab", [0, 4])
    assert rc == 0 and r["n"] == 0 and list(r["seg_stop"]) == [TAIL] and list(r["seg_first"]) == [0, 0]
    rc, r = call(fake, c, 0, b"", [0])
    assert rc == 0 and r["n"] == 0
    c.close()


def test_argument_errors(fake):
    c = Ctx(fake)
    raw = wrap([b"<1>a", b"<2>b"])
    for starts in ([1, len(raw)], [0, len(raw) - 1], [0, 5, 3, len(raw)], [0, len(raw) + 1]):
        assert call(fake, c, 0, raw, starts)[0] == L.FG_ERR_ARG
    assert call(fake, c, L.FG_CAPNP, raw, [0, len(raw)])[0] == L.FG_ERR_ARG
    assert call(fake, c, 0, raw, [0, len(raw)])[0] == 0
    c.close()
