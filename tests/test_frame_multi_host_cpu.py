"""CPU: fg_frame_decode_multi_batch (flowgger_amd/csrc/fg_host_pipeline.cpp) on the fake runtime of test_host_pipeline_cpu.py, whose
fake segmented framer (tests/native/host_pipeline_fake.cpp: fg_launch_frame_multi) keeps the real launcher's contract.  This is the
DEVICE-SUCCESS branch of the segment stage that the three multi-connection entries share -- the per-segment and per-slot columns come
back from the device columns into the pinned mirror --, its capacity retry and the classic redo of fg_frame_multi_device.  The slots
and segments must be those of a split at the terminator, the rows of the FRAME slots those of one device call on the same lines."""
import ctypes as C

import numpy as np

import test_host_pipeline_cpu as H
from flowgger_amd import _lib as L
from test_host_pipeline_cpu import Ctx, corpus, device_reference, fake, pack, snapshot  # noqa: F401  (fake: the fixture)

u64, vp = C.c_uint64, C.c_void_p
FRAME, CARRY = L.FG_SLOT_FRAME, L.FG_SLOT_CARRY


def call(lib, ctx, raw, starts, final=None, fmt=0, framing=L.FG_FRAME_LINE, null=None):
    """null: the name of an output pointer to pass as NULL"""
    lib.fg_frame_decode_multi_batch.argtypes = [vp, C.c_int, C.c_int, vp, u64, vp, vp, u64, vp, vp, vp, vp, vp, vp]
    lib.fg_last_host_path.argtypes = [vp]
    buf = np.frombuffer(raw + bytes(32), np.uint8)
    s = None if starts is None else np.asarray(starts, np.uint64)
    k = 0 if starts is None else len(starts) - 1
    fin = None if final is None else np.asarray(final, np.uint8)
    st = L.fg_tables()
    o = {"tables": st, "offsets": vp(), "kind": vp(), "seg_first": vp(), "seg_consumed": vp(), "n": u64()}
    ref = lambda name: None if name == null else C.cast(C.pointer(o[name]), vp)
    rc = lib.fg_frame_decode_multi_batch(ctx.h, fmt, framing, buf.ctypes.data, len(raw), None if s is None else s.ctypes.data,
                                         None if fin is None else fin.ctypes.data, k if starts is not None else 1, ref("tables"), ref("offsets"),
                                         ref("kind"), ref("seg_first"), ref("seg_consumed"), ref("n"))
    if rc != 0:
        return rc, None
    ns = int(o["n"].value)
    arr = lambda p, t, cnt: np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), (cnt,)).copy() if cnt else np.zeros(0, t)
    return 0, {"n": ns, "tables": st, "offsets": arr(o["offsets"], C.c_uint64, ns + 1), "kind": arr(o["kind"], C.c_uint8, ns),
               "seg_first": arr(o["seg_first"], C.c_uint64, k + 1), "seg_consumed": arr(o["seg_consumed"], C.c_uint64, k),
               "path": lib.fg_last_host_path(ctx.h)}


def split(segs, final, delim=b"\n"):
    """what the call must report: every segment split at the terminator as a stream of its own; the unterminated tail of a segment
    is a FRAME when the segment is final, else a CARRY that does not count as consumed"""
    offsets, kind, first, cons, lines, at = [0], [], [], [], [], 0
    for seg, fin in zip(segs, final):
        first.append(len(kind))
        parts = seg.split(delim)
        tail = parts.pop()
        for p in parts:
            offsets.append(offsets[-1] + len(p) + 1)
            kind.append(FRAME)
            lines.append(p)
        if tail:
            offsets.append(at + len(seg))
            kind.append(FRAME if fin else CARRY)
            lines.append(tail)
        cons.append(len(seg) - (len(tail) if tail and not fin else 0))
        at += len(seg)
    first.append(len(kind))
    return {"offsets": offsets, "kind": kind, "seg_first": first, "seg_consumed": cons, "lines": lines}


def starts_of(segs):
    return [0] + np.cumsum([len(s) for s in segs]).tolist()


def same_as_split(r, want):
    assert r["n"] == len(want["kind"]) and list(r["offsets"]) == want["offsets"] and list(r["kind"]) == want["kind"]
    assert list(r["seg_first"]) == want["seg_first"] and list(r["seg_consumed"]) == want["seg_consumed"]


def segments(rng):
    ln = [x for x in corpus(300, rng) if x]
    text = lambda a, b: b"".join(x + b"\n" for x in ln[a:b])
    #       ends on the terminator | empty | one byte | final, unterminated | NOT final, unterminated | a terminator alone
    segs = [text(0, 100), b"", b"z", text(100, 180) + b"<1>tail a=1", text(180, 260) + b"<2>cut off b=", b"\n", text(260, 290)]
    return segs, [0, 0, 1, 1, 0, 0, 0]


def test_the_device_branch_yields_the_split_segments_and_the_decode_of_their_frames(fake):
    segs, final = segments(np.random.default_rng(11))
    raw, starts, want = b"".join(segs), starts_of(segs), split(segs, final)
    assert want["kind"].count(CARRY) == 1 and want["seg_consumed"][4] == len(segs[4]) - len(b"<2>cut off b=") and want["seg_first"][1] == want["seg_first"][2]
    c = Ctx(fake)
    rc, r = call(fake, c, raw, starts, final)
    assert rc == 0 and r["path"] == L.FG_PATH_FRAME_MULTI
    same_as_split(r, want)
    got = snapshot(r["tables"], r["n"])
    fr, ca = np.nonzero(r["kind"] == FRAME)[0], np.nonzero(r["kind"] == CARRY)[0]
    data, offs = pack([want["lines"][i] for i in fr])
    ref = device_reference(fake, data, offs, len(raw) // 2 + 1024)
    assert int(ref["ent_count"].sum()) > 100
    for col in H.COLS:
        assert np.array_equal(got[col][fr], ref[col][:len(fr)]), col
    for j, i in enumerate(fr):
        fa, fb, k = int(got["ent_first"][i]), int(ref["ent_first"][j]), int(got["ent_count"][i])
        for col in ("ent_name", "ent_val", "ent_type", "ent_flags"):
            assert np.array_equal(got[col][fa:fa + k], ref[col][fb:fb + k]), (col, int(i))
    assert ((got["meta"][ca] & 0xFF) == L.FG_ST_BAD_UTF8).all() and (got["ent_count"][ca] == 0).all()
    # without seg_final nothing is final: the tail of segment 3 and the lone byte are CARRY slots too
    rc, r = call(fake, c, raw, starts, None)
    assert rc == 0
    same_as_split(r, split(segs, [0] * len(segs)))
    assert list(r["kind"]).count(CARRY) == 3
    # a second shape on the same ctx: no segments and no bytes
    rc, r = call(fake, c, b"", [0])
    assert rc == 0 and r["n"] == 0 and r["path"] == L.FG_PATH_FRAME_MULTI and list(r["offsets"]) == [0] and list(r["seg_first"]) == [0]
    # ... segments, all of them empty
    rc, r = call(fake, c, b"", [0, 0, 0], [1, 0])
    assert rc == 0 and r["n"] == 0 and list(r["seg_first"]) == [0, 0, 0] and list(r["seg_consumed"]) == [0, 0]
    c.close()


def test_a_first_capacity_that_is_too_small_is_retried_with_the_exact_count(fake):
    """more one-byte lines than nbytes / 32 + n_segs + 1024: the device entry reports the count and writes nothing, the second launch fits"""
    segs = [b"\n" * 30000, b"\n" * 10959 + b"t"]
    raw, starts = b"".join(segs), starts_of(segs)
    assert len(raw) == 40960 and len(raw) > len(raw) // 32 + len(segs) + 1024
    c = Ctx(fake)
    rc, r = call(fake, c, raw, starts, [0, 0])
    assert rc == 0 and r["path"] == L.FG_PATH_FRAME_MULTI
    same_as_split(r, split(segs, [0, 0]))
    assert r["n"] == 40960 and list(r["seg_first"]) == [0, 30000, 40960] and list(r["seg_consumed"]) == [30000, 10959]
    meta = snapshot(r["tables"], r["n"])["meta"] & 0xFF
    assert (meta[:-1] == 1).all() and meta[-1] == L.FG_ST_BAD_UTF8  # (the fake decode: empty lines; the CARRY row)
    c.close()


def test_a_one_pass_scan_that_gives_up_is_redone_by_the_classic_form(fake):
    segs, final = segments(np.random.default_rng(12))
    raw, starts, want = b"".join(segs), starts_of(segs), split(segs, final)
    fake.fake_frame_abort_next.argtypes = [C.c_int]
    c = Ctx(fake)
    res = {}
    for abort in (0, 1):
        fake.fake_frame_abort_next(abort)
        rc, r = call(fake, c, raw, starts, final)
        assert rc == 0 and fake.fake_frame_classic_launches() == abort
        same_as_split(r, want)
        res[abort] = snapshot(r["tables"], r["n"])
    fake.fake_frame_abort_next(0)
    H.same_lines(res[0], res[1], len(want["kind"]))
    c.close()


def test_argument_errors(fake):
    c = Ctx(fake)
    raw = b"<1>a\n<2>b\n"
    ok = [0, 5, len(raw)]
    for name in ("tables", "offsets", "kind", "seg_first", "seg_consumed", "n"):
        assert call(fake, c, raw, ok, null=name)[0] == L.FG_ERR_ARG
    for framing in (L.FG_FRAME_NONE, L.FG_FRAME_SYSLEN, L.FG_FRAME_CAPNP):
        assert call(fake, c, raw, ok, framing=framing)[0] == L.FG_ERR_ARG
    assert call(fake, c, raw, ok, fmt=L.FG_CAPNP)[0] == L.FG_ERR_ARG
    assert call(fake, c, raw, None)[0] == L.FG_ERR_ARG  # (segments without a list)
    for starts in ([1, len(raw)], [0, len(raw) - 1], [0, 7, 5, len(raw)], [0, len(raw) + 1], [0]):
        assert call(fake, c, raw, starts)[0] == L.FG_ERR_ARG
    lib_null_ctx = Ctx.__new__(Ctx)
    lib_null_ctx.h = None
    assert call(fake, lib_null_ctx, raw, ok)[0] == L.FG_ERR_ARG
    assert call(fake, c, raw, ok, framing=L.FG_FRAME_NUL)[0] == 0
    rc, r = call(fake, c, raw, ok)
    assert rc == 0 and r["n"] == 2 and list(r["seg_first"]) == [0, 1, 2]
    c.close()
