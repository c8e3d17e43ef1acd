"""The segmented framer on the GPU (flowgger_amd/csrc/fg_frame_multi.hip) through the C ABI: fg_frame_multi_device,
fg_frame_decode_multi_batch and MultiStreamSplitter against the model of tests/frame_multi_model.py (every segment framed by the
oracle as a stream of its own).  Both forms -- the one-pass scan with its boundary hook and the classic form with the patch kernel
between scan and prefix (FG_LO_FRAME_CLASSIC) -- must give identical slots."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

from flowgger_amd import (FlushPolicy, GelfDecoder, LTSVDecoder, MultiStreamSplitter, RFC3164Decoder, RFC5424Decoder, synth, tzdb)
from flowgger_amd import _lib as L
from flowgger_amd.record import DecodeError, parse_canonical
from frame_multi_model import LINE, NUL, SLOT_BAD_UTF8, SLOT_CARRY, SLOT_FRAME, model, term_of
from oracle_binding import Oracle
from test_gpu_round6 import check_rows, strip
from utf8_hazards import cuts, kinds

pytestmark = pytest.mark.gpu

FRAMING = {LINE: L.FG_FRAME_LINE, NUL: L.FG_FRAME_NUL}
IDS = {LINE: "line", NUL: "nul"}
GUARD = 8
G64, G8 = 0x5A5A5A5A5A5A5A5A, 0xA5
BLK, TILE = 16384, 131072


@pytest.fixture(scope="module")
def oracle():
    o = Oracle()
    o.set_rfc3164(2026, tzdb.default_table())
    return o


@pytest.fixture(scope="module")
def dec():
    d = RFC5424Decoder()
    yield d
    d.set_launch_opts()


class Out:
    pass


def run_multi(dec, raw, starts, final, framing, classic, cap=None):
    """fg_frame_multi_device on device arrays with guard words behind each; what lies behind the buffer's end inside its last
    16 bytes is terminators on purpose"""
    import torch

    dev = torch.device("cuda", dec.device)
    n, K = len(raw), len(starts) - 1
    host = np.full(((n + 15) & ~15) + 16, 0x0A if framing == LINE else 0, np.uint8)
    host[:n] = np.frombuffer(raw, np.uint8)
    d_bytes = torch.from_numpy(host).to(dev)
    d_starts = torch.from_numpy(np.array(starts, np.uint64).view(np.int64)).to(dev)
    d_final = torch.from_numpy(np.array(final, np.uint8)).to(dev) if final is not None and K else None
    cap = n + 1 if cap is None else cap
    d_off = torch.full((cap + 1 + GUARD,), G64, dtype=torch.int64, device=dev)
    d_kind = torch.full((cap + GUARD,), G8, dtype=torch.uint8, device=dev)
    d_first = torch.full((K + 1 + GUARD,), G64, dtype=torch.int64, device=dev)
    d_cons = torch.full((K + GUARD,), G64, dtype=torch.int64, device=dev)
    ns = C.c_uint64()
    dec.set_launch_opts(frame_classic=classic)
    o = Out()
    o.rc = L.lib().fg_frame_multi_device(dec._ctx, FRAMING[framing], d_bytes.data_ptr(), n, d_starts.data_ptr(),
                                         d_final.data_ptr() if d_final is not None else None, K, d_off.data_ptr(), d_kind.data_ptr(), cap,
                                         d_first.data_ptr(), d_cons.data_ptr(), C.byref(ns), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    torch.cuda.synchronize(dev)
    o.n = int(ns.value)
    off, kind = d_off.cpu().numpy().view(np.uint64), d_kind.cpu().numpy()
    first, cons = d_first.cpu().numpy().view(np.uint64), d_cons.cpu().numpy().view(np.uint64)
    o.guards_ok = bool((off[cap + 1:] == G64).all() and (kind[cap:] == G8).all() and (first[K + 1:] == G64).all() and (cons[K:] == G64).all())
    o.off_all, o.kind_all = off[:cap + 1], kind[:cap]
    m = min(o.n, cap)
    o.offsets, o.kind, o.first, o.cons = off[:m + 1], kind[:m], first[:K + 1], cons[:K]
    return o


def assert_model(oracle, dec, raw, starts, final, framing, ctx=""):
    want = model(oracle, raw, starts, final, framing)
    outs = []
    for classic in (False, True):
        o = run_multi(dec, raw, starts, final, framing, classic)
        c = f"{ctx} classic={classic}"
        assert o.rc == L.FG_OK and o.guards_ok, c
        assert o.n == len(want.kind), (c, o.n, len(want.kind))
        assert np.array_equal(o.offsets, want.offsets), (c, first_diff(o.offsets, want.offsets))
        assert np.array_equal(o.kind, want.kind), (c, first_diff(o.kind, want.kind))
        assert np.array_equal(o.first, want.seg_first), (c, first_diff(o.first, want.seg_first))
        assert np.array_equal(o.cons, want.seg_consumed), (c, first_diff(o.cons, want.seg_consumed))
        outs.append(o)
    a, b = outs
    assert np.array_equal(a.offsets, b.offsets) and np.array_equal(a.kind, b.kind) and np.array_equal(a.first, b.first) and np.array_equal(a.cons, b.cons)
    return want


def first_diff(a, b):
    n = min(len(a), len(b))
    d = np.flatnonzero(a[:n] != b[:n])
    return f"lengths {len(a)} / {len(b)}" if not len(d) else f"index {int(d[0])}: {int(a[d[0]])} != {int(b[d[0]])}"


def text_stream(framing, nbytes, seed):
    """lines of ASCII and multi-byte text, a few invalid ones, cut at exactly nbytes"""
    rng = random.Random(seed)
    t = term_of(framing)
    words = [b"alpha", b"caf\xc3\xa9", b"\xe2\x82\xac uro", b"\xf0\x9f\x98\x80", b"x" * 37, b"\xc3", b"\x80", b"\xe2\x82", b"", b"\r"]
    out = bytearray()
    while len(out) < nbytes:
        out += b" ".join(rng.choice(words) for _ in range(rng.randint(0, 9))) + t
    return bytes(out[:nbytes])


# ---- 1. one final segment is fg_frame_device ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("classic", [False, True], ids=["onepass", "classic"])
@pytest.mark.parametrize("framing", [LINE, NUL], ids=["line", "nul"])
def test_one_final_segment_equals_frame_device(dec, framing, classic):
    import torch

    dev = torch.device("cuda", dec.device)
    for size in (1, 15, BLK - 1, BLK, BLK + 1, TILE + 17):
        for seed in (1, 2):
            raw = text_stream(framing, size, seed) if seed == 1 else text_stream(framing, size - 1, seed) + term_of(framing)
            assert len(raw) == size
            o = run_multi(dec, raw, [0, size], [1], framing, classic)
            host = np.zeros(((size + 15) & ~15) + 16, np.uint8)
            host[:size] = np.frombuffer(raw, np.uint8)
            d_bytes = torch.from_numpy(host).to(dev)[:size]
            dec.set_launch_opts(frame_classic=classic)
            d_off, d_bad, n = dec.frame_device(d_bytes, FRAMING[framing])
            assert o.rc == L.FG_OK and o.guards_ok and o.n == n, (size, seed, o.n, n)
            assert np.array_equal(o.offsets, d_off.cpu().numpy()[:n + 1].view(np.uint64)), (size, seed)
            assert np.array_equal(o.kind, d_bad.cpu().numpy()[:n]), (size, seed)
            assert int(o.first[0]) == 0 and int(o.first[1]) == n and int(o.cons[0]) == size


# ---- 2. the boundary sweep ----------------------------------------------------------------------------------------------------------
SWEEP_BYTES = 300 * 1024  # three 128 KiB tiles: the look-back crosses two tile edges
OFFS = (0, 1, -1, 2, -2, 3, -3)
RES16 = (0, 1, 2, 3, 13, 14, 15)
C_EDGES = [m * BLK for m in range(1, 18) if m % 8]  # 16 KiB edges that are no tile edges


def classes_of(p):
    out = set()
    if p % 16 in RES16 and 16 <= p % 1024 <= 1008:
        out.add("chunk")
    if p % 1024 == 0:
        out.add("row")
    if min(p % BLK, BLK - p % BLK) <= 3:
        out.add("block")
    if min(p % TILE, TILE - p % TILE) <= 3:
        out.add("tile")
    return out


def sweep_plan(framing):
    """-> per buffer a list of (position, kind, cut): two placements at tile edges, 15 at block edges, 15 at row edges and 15 inside
    rows; every (kind, cut) comes by every class"""
    kcs = cuts(kinds(framing))
    N = len(kcs)
    bufs = []
    for b in range((N + 1) // 2):
        pl = []
        for e, edge in enumerate((TILE, 2 * TILE)):
            if 2 * b + e < N:
                pl.append((edge + OFFS[(2 * b + e) % 7], *kcs[2 * b + e]))
        for j, edge in enumerate(C_EDGES):
            pl.append((edge + OFFS[(b + j) % 7], *kcs[(15 * b + j) % N]))
            pl.append((edge + 1024 * (2 + (b + j) % 11), *kcs[(15 * b + j + 5) % N]))
            pl.append((edge + 14 * 1024 + 16 * (3 + j) + RES16[(b + j) % 7], *kcs[(15 * b + j + 11) % N]))
        bufs.append(sorted(pl, key=lambda x: x[0]))
    return bufs


def sweep_buffer(pl, framing, seed):
    """ASCII lines up to each placement; the hazard stands in a slot of its own: a terminator, two bytes, the hazard (the boundary
    `cut` bytes into it), two bytes, a terminator.  -> (raw, seg_starts, seg_final)"""
    t = term_of(framing)
    rng = random.Random(seed)
    out = bytearray()

    def fill_to(target):
        while len(out) < target:
            ln = min(target - len(out), rng.randint(1, 200))
            out.extend(b"f" * (ln - 1) + t)

    for pos, kind, cut in pl:
        fill_to(pos - cut - 2)
        assert len(out) == pos - cut - 2, "placements too close"
        out.extend(b"pq" + kind.data + b"rs" + t)
    fill_to(SWEEP_BYTES - 6)
    out.extend(b"tail\xe2\x82")  # the buffer's own end: an unterminated, cut-off tail
    starts = [0] + [p for p, _, _ in pl] + [len(out)]
    final = [rng.randint(0, 1) for _ in range(len(starts) - 1)]
    return bytes(out), starts, final


def test_sweep_plan_covers_every_hazard_at_every_position_class():
    """(no launch: the plan of test_boundary_sweep) every (kind, cut) meets each of the four position classes"""
    for framing in (LINE, NUL):
        want = {(k.name, c) for k, c in cuts(kinds(framing))}
        seen = {cls: set() for cls in ("chunk", "row", "block", "tile")}
        for pl in sweep_plan(framing):
            for pos, kind, cut in pl:
                for cls in classes_of(pos):
                    seen[cls].add((kind.name, cut))
        for cls, have in seen.items():
            assert have == want, (IDS[framing], cls, sorted(want - have)[:5])


@pytest.mark.parametrize("part", range(4))
@pytest.mark.parametrize("framing", [LINE, NUL], ids=["line", "nul"])
def test_boundary_sweep(oracle, dec, framing, part):
    plan = sweep_plan(framing)
    for b in range(part, len(plan), 4):
        raw, starts, final = sweep_buffer(plan[b], framing, 100 * b + framing)
        want = assert_model(oracle, dec, raw, starts, final, framing, f"{IDS[framing]} buffer {b}")
        assert SLOT_CARRY in want.kind and SLOT_BAD_UTF8 in want.kind


# ---- 3. short and empty segments ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("framing", [LINE, NUL], ids=["line", "nul"])
def test_short_and_empty_segments(oracle, dec, framing):
    t = term_of(framing)
    alphabet = [t, b"a", b"\xc3", b"\xa9", b"\xe2", b"\x82", b"\xac", b"\xf0"]
    for seed in (7, 8):
        rng = random.Random(seed + 10 * framing)
        lens = [rng.randint(0, 5) for _ in range(4096)]
        if seed == 8:  # ... with empty segments at both ends
            lens[:3] = [0, 0, 0]
            lens[-3:] = [0, 0, 0]
        raw = b"".join(rng.choice(alphabet) for _ in range(sum(lens)))
        starts = np.concatenate([[0], np.cumsum(lens)]).tolist()
        final = [rng.randint(0, 1) for _ in lens]
        want = assert_model(oracle, dec, raw, starts, final, framing, f"seed {seed}")
        assert {int(k) for k in want.kind} == {SLOT_FRAME, SLOT_BAD_UTF8, SLOT_CARRY}


# ---- 4. capacity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("classic", [False, True], ids=["onepass", "classic"])
def test_capacity_one_too_small(oracle, dec, classic):
    for framing in (LINE, NUL):
        for tail in (b"", b"unterminated"):
            raw = text_stream(framing, 40000, 5) + term_of(framing) + tail
            starts = [0, 100, 100, 20000, 33333, len(raw)]
            final = [0, 1, 0, 1, 0]
            want = model(oracle, raw, starts, final, framing)
            need = len(want.kind)
            o = run_multi(dec, raw, starts, final, framing, classic, cap=need - 1)
            assert o.rc == L.FG_ERR_ENT_OVERFLOW and o.n == need and o.guards_ok
            assert (o.first == G64).all() and (o.cons == G64).all()  # (the per-segment outputs are not written)
            o = run_multi(dec, raw, starts, final, framing, classic, cap=need)
            assert o.rc == L.FG_OK and o.n == need and o.guards_ok
            assert np.array_equal(o.offsets, want.offsets) and np.array_equal(o.kind, want.kind)
            assert np.array_equal(o.first, want.seg_first) and np.array_equal(o.cons, want.seg_consumed)


# ---- 5. decode parity ---------------------------------------------------------------------------------------------------------------
def format_case(name):
    if name == "rfc5424":
        return RFC5424Decoder(), None, synth.rfc5424_lines(300, cfg=2)
    if name == "ltsv":
        return LTSVDecoder(synth.LTSV_CONFIG), synth.LTSV_CONFIG, synth.ltsv_lines(300)
    if name == "gelf":
        return GelfDecoder(), None, synth.gelf_lines(300)
    return RFC3164Decoder({"rfc3164": {"current_year": 2026}}), None, synth.rfc3164_lines(300)


@pytest.mark.parametrize("name", ["rfc5424", "ltsv", "gelf", "rfc3164"])
def test_decode_parity(oracle, name):
    d, cfg, lines = format_case(name)
    rng = random.Random(len(name))
    for framing in (LINE, NUL):
        t = term_of(framing)
        parts = []
        for i, ln in enumerate(lines):
            ln = ln.replace(b"\0", b" ").replace(b"\n", b" ")
            if i % 41 == 7:
                ln = ln[:20] + b"\xe2\x82" + ln[20:]  # invalid UTF-8
            parts.append(ln + (b"\r\n" if framing == LINE and i % 5 == 0 else t))
        raw = b"".join(parts)
        cutpos = sorted(rng.randrange(1, len(raw)) for _ in range(36))
        starts = [0] + cutpos + [len(raw)]
        final = [rng.randint(0, 1) for _ in range(37)]
        want = model(oracle, raw, starts, final, framing)
        for classic in (False, True):
            d.set_launch_opts(frame_classic=classic)
            tab, offsets, kind, first, cons = d.frame_decode_multi(raw, starts, final, FRAMING[framing])
            assert d.last_host_path() == L.FG_PATH_FRAME_MULTI
            assert np.array_equal(offsets, want.offsets) and np.array_equal(kind, want.kind)
            assert np.array_equal(first, want.seg_first) and np.array_equal(cons, want.seg_consumed)
            assert SLOT_CARRY in kind and SLOT_BAD_UTF8 in kind
            n = len(kind)
            assert tab.n == n
            # FRAME rows equal the oracle's decode of that frame; BAD_UTF8 and CARRY rows have FG_ST_BAD_UTF8
            check_rows(oracle, d.fmt, cfg, d._cfg, raw, FRAMING[framing], offsets[:-1], offsets[1:], (kind == SLOT_FRAME).astype(np.uint8), tab, offsets)
            assert (tab.status[:n][kind != SLOT_FRAME] == L.FG_ST_BAD_UTF8).all()
    d.set_launch_opts()


# ---- 6. carry-over through MultiStreamSplitter --------------------------------------------------------------------------------------
RUST_WS = "\t\n\x0b\x0c\r \x85\xa0\u1680\u2000\u2001\u2002\u2003\u2004\u2005\u2006\u2007\u2008\u2009\u200a\u2028\u2029\u202f\u205f\u3000"  # char::is_whitespace


def whole_stream(oracle, fmt, raw, framing):
    """what LineSplitter::run / NulSplitter::run make of one connection's whole stream: Oracle.frame + decode"""
    frames = oracle.frame(raw, "line" if framing == LINE else "nul")
    good = [body for _, _, body, valid in frames if valid]
    blob, offs = oracle.decode_batch(fmt, *synth.pack(good)) if good else (None, None)
    out, j = [], 0
    for _, _, body, valid in frames:
        if not valid:
            out.append("Invalid UTF-8 input")
            continue
        r = parse_canonical(blob[int(offs[j]):int(offs[j + 1])].tobytes())
        j += 1
        if isinstance(r, DecodeError):
            text = body.decode("utf-8").strip(RUST_WS)
            if framing == NUL and not text:
                continue  # nul_splitter.rs:41-46
            r = f"{r}: [{text}]"
        out.append(r)
    return out


@pytest.mark.parametrize("framing", [LINE, NUL], ids=["line", "nul"])
def test_carry_over_of_eight_connections(oracle, framing):
    d = RFC5424Decoder()
    t = term_of(framing)
    rng = random.Random(77 + framing)
    lines = synth.rfc5424_lines(8 * 90, cfg=2)
    streams = []
    for c in range(8):
        mine = [ln.replace(b"\0", b" ") for ln in lines[c * 90:(c + 1) * 90]]
        if c == 2:  # a line longer than any chunk
            mine[30] = mine[30] + b" " + b"L" * 6000
        if c == 5:  # an invalid sequence (split across a chunk cut below), a valid one likewise, empty frames
            mine[10] = mine[10][:40] + b"\xf0\x9f\x98" + mine[10][40:]
            mine[11] = mine[11] + b" \xf0\x9f\x98\x80"
            mine[12] = b""
            mine[13] = b"   "
        raw = b"".join(ln + (b"\r\n" if framing == LINE and i % 7 == 0 else t) for i, ln in enumerate(mine))
        if c % 2:
            raw += b"<13>1 2015-08-05T15:53:45Z host app 1 - - the last line has no terminator"
        streams.append(raw)
    want = [whole_stream(oracle, d.fmt, s, framing) for s in streams]
    ms = MultiStreamSplitter(d, FRAMING[framing], FlushPolicy(max_bytes=1 << 30, max_latency_ms=1e9))
    got = [[] for _ in streams]
    pos = [0] * 8
    bad_at = streams[5].index(b"\xf0\x9f\x98")
    flushes = 0
    while any(pos[c] < len(streams[c]) for c in range(8)):
        for c in rng.sample(range(8), 8):
            if pos[c] >= len(streams[c]):
                continue
            step = rng.randint(1, 3000)
            if c == 5 and pos[c] < bad_at + 1 < pos[c] + step:
                step = bad_at + 1 - pos[c]  # the chunk ends inside the invalid sequence
            assert ms.push(c, streams[c][pos[c]:pos[c] + step]) == []
            pos[c] += step
            if pos[c] >= len(streams[c]):
                ms.close(c)
        for c, res in ms.flush():
            got[c] += res
        flushes += 1
    for c, res in ms.flush():
        got[c] += res
    assert flushes >= 5
    for c in range(8):
        have = [str(r) if isinstance(r, DecodeError) else r for r in got[c]]
        assert len(have) == len(want[c]), (c, len(have), len(want[c]))
        for i, (a, b) in enumerate(zip(have, want[c])):
            assert a == b, (c, i, a, b)
    assert "Invalid UTF-8 input" in want[5] and any(isinstance(x, str) and x.endswith(": []") for x in want[5]) == (framing == LINE)


# ---- 7. arguments -------------------------------------------------------------------------------------------------------------------
def test_arguments(dec):
    raw = b"one\ntwo\n"
    for fr in (L.FG_FRAME_SYSLEN, L.FG_FRAME_CAPNP, L.FG_FRAME_NONE):
        with pytest.raises(L.FgError) as e:
            dec.frame_decode_multi(raw, [0, 4, 8], [1, 1], fr)
        assert e.value.code == L.FG_ERR_ARG
    o = Out()
    import torch

    dev = torch.device("cuda", dec.device)
    d_bytes = torch.zeros(32, dtype=torch.uint8, device=dev)
    d_starts = torch.tensor([0, 8], dtype=torch.int64, device=dev)
    d_off = torch.zeros(16, dtype=torch.int64, device=dev)
    d_kind = torch.zeros(16, dtype=torch.uint8, device=dev)
    ns = C.c_uint64()
    for fr in (L.FG_FRAME_SYSLEN, L.FG_FRAME_CAPNP):
        o.rc = L.lib().fg_frame_multi_device(dec._ctx, fr, d_bytes.data_ptr(), 8, d_starts.data_ptr(), None, 1, d_off.data_ptr(), d_kind.data_ptr(), 8,
                                             d_off.data_ptr(), d_off.data_ptr(), C.byref(ns), None)
        assert o.rc == L.FG_ERR_ARG
    # FG_CAPNP has no line decoder
    st = L.fg_tables()
    vp = [C.c_void_p() for _ in range(4)]
    buf = np.frombuffer(raw, np.uint8)
    starts = np.array([0, 4, 8], np.uint64)
    rc = L.lib().fg_frame_decode_multi_batch(dec._ctx, L.FG_CAPNP, L.FG_FRAME_LINE, buf.ctypes.data, 8, starts.ctypes.data, None, 2, C.byref(st),
                                             *[C.byref(v) for v in vp], C.byref(ns))
    assert rc == L.FG_ERR_ARG
    # a list that does not tile is an error on the host entry
    for bad in ([1, 4, 8], [0, 4, 7], [0, 5, 4, 8], [0, 9, 8]):
        with pytest.raises(L.FgError):
            dec.frame_decode_multi(raw, bad, None, L.FG_FRAME_LINE)
    # nothing in, nothing out
    tab, offsets, kind, first, cons = dec.frame_decode_multi(b"", [0], None, L.FG_FRAME_LINE)
    assert tab is None and len(kind) == 0 and [int(x) for x in first] == [0]
    tab, offsets, kind, first, cons = dec.frame_decode_multi(b"", [0, 0, 0], [1, 0], L.FG_FRAME_NUL)
    assert tab is None and len(kind) == 0 and [int(x) for x in first] == [0, 0, 0] and [int(x) for x in cons] == [0, 0]
    o = run_multi(dec, b"", [0, 0, 0], [0, 1], LINE, False)
    assert o.rc == L.FG_OK and o.n == 0 and o.guards_ok and [int(x) for x in o.first] == [0, 0, 0] and [int(x) for x in o.cons] == [0, 0]
    # ... and the tables of a good call
    tab, offsets, kind, first, cons = dec.frame_decode_multi(raw, [0, 4, 8], [1, 1], L.FG_FRAME_LINE)
    assert tab.n == 2 and [int(x) for x in offsets] == [0, 4, 8] and dec.last_host_path() == L.FG_PATH_FRAME_MULTI
